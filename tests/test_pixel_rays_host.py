"""The host side of pwn_pixel_rays_device on the CPU (tools/sanitize/pixel_rays_driver.cpp): pwn_pixel_rays.cpp compiled with g++ against
the stand-in HIP runtime and stand-ins for its two launches, in a stand-alone program under AddressSanitizer + UBSan.  What the two
launches are handed in both layouts of the pixels and for the whole frame, with and without seeds, every refusal with nothing
launched and nothing written, PWN_OK before a level, pwn_stats and pwn_launch_order_waits untouched, no leak behind pwn_destroy.
No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_pixel_rays_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "pixel_rays", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "pixel_rays_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
