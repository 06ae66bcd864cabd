"""The host side of pwn_upload_level_device on the CPU (tools/sanitize/level_device_driver.cpp): pwn_level_device.cpp compiled with g++
against the stand-in HIP runtime and a stand-in for the bake's launch that runs the kernel's algorithm sequentially over level_bake.h,
in a stand-alone program under AddressSanitizer + UBSan.  Every refusal with nothing launched, the launch count of a call, four
calls going round the table copies, the walk buffer chosen never one another copy refers to, the tables and the walk table a launch
reads afterwards against the host's of the same level, a refused table, pwn_upload_spheres_device keeping the device level, a host
upload putting the host's level back with the base copy marked stale, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_level_device_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "level_device", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(out_dir, "level_device_asan")], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
