"""level_bake.h on the CPU: the rules that the device's level builder (level_bake.hip) derives, checks and bakes a level with,
compiled with gcc into tests/level_bake_driver.c and held to level_host.c -- the verdict against pwn_check_portals and against
baked_scenes.table_is_taken (a rule derived from the reference's tests, not from the library's), the 65 x 65 words and the 52
records against pwn_bake_cells byte for byte, the derived table against pwn_parse_level on the grid's own bytes.  Hostile
coordinates run in the same stand-alone program under AddressSanitizer + UBSan.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import level_device_cases as lc
from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
GIVEN, DERIVED, DERIVED_RAW = 1, 0, 2


def _compile(d, name, extra):
    exe = str(d / name)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "level_bake_driver.c"),
                           os.path.join(CSRC, "level_host.c"), "-o", exe, "-lm"])
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("level_bake")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    return _compile(d, "level_bake_driver", []), _compile(d, "level_bake_driver_san", san), d


def run(exe, d, cases):
    """cases: (mode, data, pmap or None) -> per case dict(verdict, letter, host_check, nrec, host_nrec, words, recs, table, pmap)"""
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for mode, data, pm in cases:
            f.write(np.int32(mode).tobytes())
            f.write(np.ascontiguousarray(data, np.uint8).tobytes())
            f.write(np.ascontiguousarray(pm if pm is not None else np.zeros((26, 7)), np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.returncode, p.stderr[-3000:])
    lines = p.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(cases) + 1
    out = []
    for line in lines[:-1]:
        v = [int(x) for x in line.split()]
        out.append(dict(zip(("verdict", "letter", "host_check", "nrec", "host_nrec", "words", "recs", "table"), v[:8]), pmap=np.array(v[8:], np.int32).reshape(26, 7)))
    return out


def test_given_tables_verdict_and_bake_equal_the_hosts(drivers):
    exe, _, d = drivers
    rand = lc.random_levels()
    lc.both_kinds_occur(rand)
    assert sum(1 for lv in rand if lv[3]) == 37 and sum(1 for lv in rand if not lv[3]) == 11
    levels = [(n, a, p, t) for n, a, p, t in rand] + [(n, a, p, False) for n, a, p in lc.refused_tables()] + \
             [(n, a, p, True) for n, a, p in lc.shipped_levels()]
    res = run(exe, d, [(GIVEN, a, p) for _, a, p, _ in levels])
    for (name, data, pm, taken), r in zip(levels, res):
        assert (r["verdict"] == 0) == taken == bool(r["host_check"]), (name, r)
        assert (r["pmap"] == pm).all(), name
        assert (r["verdict"], r["letter"]) == lc.expected_verdict(data, pm), name          # (the restatement the GPU tests expect by)
        if taken:
            assert r["words"] == 1 and r["recs"] == 1 and r["nrec"] == r["host_nrec"] and r["letter"] == 26, (name, r)
        else:
            # nothing baked; the letter is one whose row offends
            assert r["words"] == -1 and r["nrec"] == 0 and 0 <= r["letter"] < 26, (name, r)
            if r["verdict"] == 1:
                row = pm[r["letter"], :4]
                assert ((row < -1) | (row > 63)).any() and not ((pm[:r["letter"], :4] < -1) | (pm[:r["letter"], :4] > 63)).any(), name
    named = dict((n, r) for (n, _, _, _), r in zip(levels, res))
    assert named["coordinate_out_of_range"]["verdict"] == 1 and named["coordinate_out_of_range"]["letter"] == 25
    assert [named[n]["verdict"] for n, _, _ in lc.refused_tables()[:-1]] == [2] * 6
    assert [named[n]["letter"] for n, _, _ in lc.refused_tables()[:-1]] == [0, 1, 2, 3, 3, 4]


def test_derived_tables_equal_pwn_parse_level(drivers):
    exe, _, d = drivers
    rand = lc.random_levels()
    lc.both_kinds_occur(rand)
    grids = [(n, a) for n, a, _, _ in rand] + [(n, a) for n, a, _ in lc.shipped_levels()] + lc.derived_grids()
    for name, a in grids:          # what the equality with the parser is stated for
        assert not np.isin(a, [10, 13, ord('*')] + list(range(ord('a'), ord('z')))).any(), name
    res = run(exe, d, [(DERIVED, a, None) for _, a in grids])
    for (name, a), r in zip(grids, res):
        # a derived table always passes, and its bake is the host's bake of the parser's table
        assert r["table"] == 1 and r["verdict"] == 0 and r["host_check"] == 1 and r["words"] == 1 and r["recs"] == 1 and r["nrec"] == r["host_nrec"], (name, r)
        assert (r["pmap"] == lc.parse_level(a.tobytes())[1]).all(), name
    # the hand-made grids, spelled out
    pm = dict((n, r["pmap"]) for (n, _), r in zip(grids, res))["aliasing_4095_sightings"]
    A, B, C, D, E, F, G = (pm[i] for i in range(7))
    assert tuple(A) == (63, 5, 0, 6, 2, ord('A'), ord('.'))               # no open neighbour: both fall back to +x, for the first the OTHER
    assert tuple(B) == (63, 10, 20, 20, 3, ord(';'), ord('$'))            # +x of column 63 is column 0 of the next row; +z
    assert tuple(C) == (30, 30, 63, 63, 2, ord('"'), ord('#'))            # -x; -x (cell 4095: +x and +z are outside the array)
    assert tuple(D[:4]) == (3, 40, 9, 40) and tuple(E[:4]) == (40, 3, 44, 3)
    assert tuple(F) == (50, 50, 55, 55, 2, ord('.'), ord('.'))
    assert tuple(G) == (8, 58, -1, -1, 0, ord(';'), ord(';'))
    assert (pm[7:, :4] == -1).all()


def test_hostile_coordinates_and_bytes_under_sanitizers(drivers):
    exe, san, d = drivers
    hostile = lc.hostile_coordinate_tables()
    cases = [(GIVEN, a, p) for _, a, p in hostile] + [(DERIVED_RAW, lc.all_bytes_grid(), None), (GIVEN, lc.all_bytes_grid(), lc.hostile_coordinate_tables()[-1][2])]
    cases += [(GIVEN, a, p) for _, a, p, _ in lc.random_levels()] + [(GIVEN, a, p) for _, a, p in lc.refused_tables()] + [(DERIVED, a, None) for _, a in lc.derived_grids()]
    res = run(san, d, cases)
    for x, y in zip(res, run(exe, d, cases)):          # (the plain build computes the same)
        assert (x["pmap"] == y["pmap"]).all() and all(x[k] == y[k] for k in x if k != "pmap")
    for (name, _, pm), r in zip(hostile, res):
        # verdict 1, nothing touched: no bake, and the ruler refuses too
        assert r["verdict"] == 1 and r["host_check"] == 0 and r["words"] == -1 and r["recs"] == -1 and r["nrec"] == 0, (name, r)
        assert r["letter"] == (0 if name == "all_hostile" else 10), (name, r)
    raw = res[len(hostile)]
    assert (raw["pmap"] == lc.derive_table(lc.all_bytes_grid())).all() and (raw["pmap"][:, 2] != -1).all()
    for (_, a), r in zip(lc.derived_grids(), res[-len(lc.derived_grids()):]):
        assert (r["pmap"] == lc.derive_table(a)).all()
    assert raw["verdict"] == 0 and raw["host_check"] == 1 and raw["words"] == 1 and raw["recs"] == 1
    assert res[len(hostile) + 1]["verdict"] == 1
