"""The host side of pwn_players_step / pwn_players_step_device on the CPU (tools/sanitize/players_driver.cpp): pwn_players.cpp and
pwn_tables.cpp compiled with g++ against the stand-in HIP runtime and a stand-in step, under AddressSanitizer + UBSan.  The host form's
arrays there and back as its staging grows, the walk table every step is handed -- the level in force through level uploads, more
sphere uploads than there are copies of the tables and a repack -- an upload's wait for the steps that read the copy it fills, every
refusal with nothing launched and nothing written, pwn_stats untouched, no leak behind pwn_destroy.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_players_host_side_under_sanitizers(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "players", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "players_asan"), level], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out, out[-4000:]
