"""The host side of pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device and pwn_trace_rays_hide_device on the CPU
(tools/sanitize/hide_viewports_driver.cpp): pwn_viewports_device.cpp, pwn_calls.cpp and pwn_launch.cpp compiled with g++ against the
stand-in HIP runtime and stand-in launches, in a stand-alone program under AddressSanitizer + UBSan; no library is preloaded.
d_hide reaches the set-up launcher and the records carry hide[perm[j]] + 1; a plain call after a hide call in the same record set
passes none and leaves 0; which trace launcher a call goes to; every refusal (NULL, misaligned, overlap with each written range) with
nothing launched or written; the ticket sets over mixed plain and hide calls on one and two streams; no allocation, synchronisation or
host wait after the first device call; the layout-use event of a hide call, which pwn_viewports_layout_free waits for; no leak behind
pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_hide_viewports_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "hide_viewports", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "hide_viewports_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
