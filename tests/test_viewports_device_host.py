"""The host side of pwn_viewports_layout / pwn_trace_viewports_device on the CPU (tools/sanitize/viewports_device_driver.cpp):
pwn_viewports_device.cpp compiled with g++ against the stand-in HIP runtime and stand-ins for its three kinds of launch (the set-up
launch's is the algorithm itself, run sequentially), in a stand-alone program under AddressSanitizer + UBSan.  What each launch is
handed (records in rising-units order, perm a permutation, pitch = the layout's W, a skip-ahead table long enough for the widest
view, the records of the right ticket set over 10 calls on one and on two streams), the baked records word for word against the
host form's, every refusal with nothing launched and nothing written, free and a freed layout refused, 100 layouts created and
freed, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_viewports_device_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "viewports_device", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "viewports_device_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
