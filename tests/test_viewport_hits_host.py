"""The host side of pwn_trace_viewport_hits / pwn_trace_viewport_hits_device on the CPU (tools/sanitize/viewport_hits_driver.cpp):
pwn_calls.cpp and pwn_viewports_device.cpp compiled with g++ against the stand-in HIP runtime and stand-in launches (the trace
launch's writes every word it is handed), in a stand-alone program under AddressSanitizer + UBSan; no library is preloaded.  What
each launch is handed (the records byte for byte the colour call's for the same rectangles and cameras but for the time, the three
plane pointers), 0 outside the rectangles from the host form and nothing written there by the device form, the staging as it grows,
planes left out, the ticket sets over calls on one and two streams mixed with pwn_trace_viewports_device calls of the same layout,
no allocation, synchronisation or host wait after the first device call, every refusal with nothing launched or written,
pwn_viewports_layout_free waiting for a hits call's use, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_viewport_hits_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "viewport_hits", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "viewport_hits_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
