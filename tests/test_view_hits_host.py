"""The host side of pwn_trace_view_hits / pwn_trace_view_hits_device on the CPU (tools/sanitize/view_hits_driver.cpp): pwn_calls.cpp
and pwn_launch.cpp compiled with g++ against the stand-in HIP runtime and a stand-in trace launch that writes every word of the
planes it is handed, under AddressSanitizer + UBSan.  Batches against one view at a time, the staging as it grows, planes left
out, both forms, every refusal with nothing launched and nothing written, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_view_hits_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "view_hits", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "view_hits_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
