"""The host side of pwn_trace_reach / pwn_trace_reach_device / pwn_trace_reach_hide_device on the CPU (tools/sanitize/reach_driver.cpp): a
stand-alone program with its own main drives pwn_reach.cpp, compiled with g++ against the stand-in HIP runtime and a stand-in launcher,
under AddressSanitizer + UBSan.  The host form's arrays there and back as its staging grows through pwn_trace_hits' buffers, n = 0,
where the launch finds records, reaches and hits, which launcher a call goes to, every refusal and the overlap rules with nothing
launched and nothing written, no leak behind pwn_destroy.  Nothing is loaded into Python; no GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_reach_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "reach", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "reach_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
