"""The sphere tables' device-memory form as the host packs it, read the way the kernels read it -- on the CPU, under AddressSanitizer
+ UBSan, against the stand-in HIP runtime (tools/sanitize/tables_driver.cpp): every cell's word, ordinal and liststart entry, every
record up to its list's end mark, the read-ahead record behind the last one, which[] and the spheres against the context's own bins
and object table, for tables that grow, shrink, change form, are refused (PWN_ETOOBIG leaves the previous ones in force) and change
under frames in flight.  No GPU needed."""
import os
import subprocess

from conftest import ROOT


def test_global_tables_are_what_the_walk_reads(tmp_path):
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "tables", "OUT=" + out_dir], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(out_dir, "tables_asan")], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out and "CHECK FAILED" not in out, out[-4000:]
    assert "refused rc -7 state same 1" in out
