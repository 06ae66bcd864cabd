"""The host side of pwn_upload_spheres_device on the CPU (tools/sanitize/spheres_device_driver.cpp): pwn_spheres_device.cpp compiled with
g++ against the stand-in HIP runtime and a stand-in for the build's launches that reads and writes exactly the ranges the kernels do,
in a stand-alone program under AddressSanitizer + UBSan.  Every pointer and size inside what was reserved for growing and shrinking
n / max_pairs, the tables a launch reads walked as the kernels walk them, the copies' rotation, the overflow tables, every refusal
with nothing launched, who owns the tables, the base copy once per level, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_spheres_device_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "spheres_device", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(out_dir, "spheres_device_asan")], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
