"""pwn_bake_cells (pwnfps_amd/csrc/level_host.c, cell_bake.h): what the walk's portal arms ask of a cell, decided once
per level, against a literal restatement of the reference's own tests (tests/baked_scenes.py: trace.h:404-413,
508-559).  Every entry of the 65 x 65 table is compared, the clamp copies in row and column 64 for several
coordinates outside the grid each; every endpoint record too.  The hand-made levels of the GPU test are checked
here as well, and on them the oracle against the compiled reference where that is built."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import baked_scenes as bs
import refharness
from conftest import GOLD, ROOT

EP_MAX = 52


def _lib():
    lib = C.CDLL(os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so"))
    lib.pwn_bake_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pwn_bake_cells.restype = C.c_int
    lib.pwn_check_portals.argtypes = [C.c_void_p, C.c_void_p]
    lib.pwn_check_portals.restype = C.c_int
    lib.pwn_parse_level.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


REC = np.dtype([("dx", np.float16), ("dz", np.float16)])       # cell_bake.h: what is added to the position, two half floats
PROT_SHIFT = 13


def _bake(lib, data, pmap):
    data = np.ascontiguousarray(data, np.uint8)
    pmap = np.ascontiguousarray(pmap, np.int32)
    low = np.full((65, 65), 0xAAAA, np.uint16)
    recs = np.zeros(EP_MAX, REC)
    n = lib.pwn_bake_cells(data.ctypes.data, pmap.ctypes.data, low.ctypes.data, recs.ctypes.data)
    assert 0 <= n <= EP_MAX
    return low, recs, n


def _taken(lib, data, pmap):
    data = np.ascontiguousarray(data, np.uint8)
    pmap = np.ascontiguousarray(pmap, np.int32)
    return lib.pwn_check_portals(data.ctypes.data, pmap.ctypes.data) == 1


def _check(lib, data, pmap, tag):
    low, recs, n = _bake(lib, data, pmap)
    used = set()
    seen = {"wall": 0, "magenta": 0, "go": 0, "copy_of_endpoint": 0, "lt2": 0, "ltdq": 0}
    for uz in range(65):
        for ux in range(65):
            want_low, step = bs.expected_cell(data, pmap, ux, uz)
            got = int(low[uz, ux])
            assert got & ~(0xff | (3 << PROT_SHIFT)) == 0, (tag, ux, uz, got)            # nothing where the class bits go
            rot_bits, got = got >> PROT_SHIFT, got & 0xff
            assert rot_bits == 0 or isinstance(step, tuple), (tag, ux, uz)
            assert got & 3 == want_low, (tag, ux, uz, got, want_low)
            seen["lt2"] += want_low & 1
            seen["ltdq"] += want_low >> 1
            st = got >> 2
            if step is None:
                assert st == 0, (tag, ux, uz, got)
            elif step == "wall":
                assert st == bs.PST_WALL, (tag, ux, uz, got)
                seen["wall"] += 1
            elif step == "magenta":
                assert st == bs.PST_MAGENTA, (tag, ux, uz, got)
                seen["magenta"] += 1
                if ux == 64 or uz == 64:
                    seen["copy_of_endpoint"] += int((low[uz % 64, ux % 64] & 0xff) >> 2 >= bs.PST_REC0)
            else:
                assert ux < 64 and uz < 64
                k = st - bs.PST_REC0
                assert 0 <= k < n and k not in used, (tag, ux, uz, got, n)
                used.add(k)
                _, x, z, dx, dz, rot = step
                r = recs[k]
                # exact, the sign of a zero included: the reference adds from endpoint 1 and subtracts from endpoint 2
                assert np.float32(r["dx"]).view(np.uint32) == np.float32(dx).view(np.uint32), (tag, ux, uz)
                assert np.float32(r["dz"]).view(np.uint32) == np.float32(dz).view(np.uint32), (tag, ux, uz)
                # the other endpoint's cell as the kernel forms it: this cell plus the same numbers, in fp32
                assert (int(np.float32(ux) + np.float32(r["dx"])), int(np.float32(uz) + np.float32(r["dz"]))) == (x, z), (tag, ux, uz)
                assert rot_bits == rot, (tag, ux, uz)
                seen["go"] += 1
    assert used == set(range(n)), tag
    return seen, n


def _parse(lib, path):
    raw = open(path, "rb").read()
    cells = np.zeros(4096, np.uint8); pmap = np.zeros((26, 7), np.int32); spawn = np.zeros(2, np.int32)
    assert lib.pwn_parse_level(raw, len(raw), cells.ctypes.data, pmap.ctypes.data, spawn.ctypes.data) == 0
    return cells.reshape(64, 64), pmap


def test_golden_levels():
    lib = _lib()
    paths = sorted(glob.glob(os.path.join(GOLD, "levels", "*.txt")))
    assert len(paths) >= 3
    shaped = 0
    for p in paths:
        data, pmap = _parse(lib, p)
        assert _taken(lib, data, pmap)
        seen, n = _check(lib, data, pmap, os.path.basename(p))
        assert seen["go"] == n
        # the same level as the reference's level_load leaves its table: z of endpoints never seen 0, or left over
        rng = np.random.default_rng(len(p))
        for stale in (None, rng.integers(0, 64, (26, 2)), np.full((26, 2), 63)):
            pm = bs.as_level_load_leaves_it(pmap, stale)
            shaped += int((pm[:, 1] != pmap[:, 1]).any() or (pm[:, 3] != pmap[:, 3]).any())
            assert bs.table_is_taken(data, pm) and _taken(lib, data, pm), (p, stale is None)
            again, n2 = _check(lib, data, pm, os.path.basename(p))
            assert (again, n2) == (seen, n)
    assert shaped >= 3          # level.txt pairs 21 of its 26 letters: its table does differ that way


def test_random_levels_with_the_hostile_cases():
    lib = _lib()
    rng = np.random.default_rng(20240607)
    total = dict.fromkeys(("wall", "magenta", "go", "copy_of_endpoint", "lt2", "ltdq"), 0)
    taken = refused = 0
    for it in range(400):
        data, pmap = bs.random_level(rng, it)
        # which tables pwn_upload_level takes: the library's check against what the reference's tests say (a table is
        # taken if and only if every entry of row / column 64 has one answer for all the cells that read it, -1 included);
        # what is taken is baked to that answer; what is refused is never baked
        ok = bs.table_is_taken(data, pmap)
        assert _taken(lib, data, pmap) == ok, it
        if not ok:
            refused += 1
            continue
        taken += 1
        seen, n = _check(lib, data, pmap, it)
        for k in total:
            total[k] += seen[k]
    assert taken >= 300 and refused >= 20, (taken, refused)
    # the cases are really there: unpaired letters, letters off their endpoints, endpoints in row / column 0 whose
    # copies read as non-endpoints
    assert all(v > 100 for v in total.values()), total


def test_hand_made_levels_and_their_hostile_tables():
    import oracle
    lib = _lib()
    for sc in bs.scenes(oracle.SPHERE_DTYPE):
        assert _taken(lib, sc.data, sc.pmap), sc.name
        _check(lib, sc.data, sc.pmap, sc.name)
    # x2 == -1 with the ray standing on endpoint 1: looked through at c2 all the same, and a plain wall to walk into
    sc = next(s for s in bs.scenes(oracle.SPHERE_DTYPE) if s.name == "unpaired_far_hash")
    low, _, _ = _bake(lib, sc.data, sc.pmap)
    assert low[9, 14] == bs.LT2 | (bs.PST_WALL << 2) and low[4, 14] == bs.LT2 | (bs.PST_WALL << 2)
    # both endpoints in one cell: endpoint 1's record (the rotation negated)
    sc = next(s for s in bs.scenes(oracle.SPHERE_DTYPE) if s.name == "both_endpoints_one_cell")
    low, recs, _ = _bake(lib, sc.data, sc.pmap)
    r = recs[((low[2, 14] & 0xff) >> 2) - bs.PST_REC0]
    assert (r["dx"].view(np.uint16), r["dz"].view(np.uint16), int(low[2, 14]) >> PROT_SHIFT) == (0, 0, 3)


def test_tables_that_are_refused():
    """-1 in a portal table is compared with the ray's cell like any coordinate (trace.h:404-413, 508-559), and cells at
    coordinate -1 read row / column 0: on each of these tables the reference's answer for an entry of row / column 64
    depends on WHICH outside cell reads it, which one table entry cannot say.  pwn_upload_level refuses them."""
    lib = _lib()
    for name, data, pmap in bs.refused_tables():
        assert not bs.table_is_taken(data, pmap), name
        assert not _taken(lib, data, pmap), name
        if name == "coordinate_out_of_range":
            continue
        split = 0
        for uz in range(65):
            for ux in range(65):
                try:
                    bs.expected_cell(data, pmap, ux, uz)
                except AssertionError:
                    split += 1
        assert split > 0, name
    # the same letters with a table a loader writes are taken
    for name, data, pmap in bs.refused_tables():
        pm = bs.empty_pmap()
        assert bs.table_is_taken(data, pm) and _taken(lib, data, pm), name


@pytest.mark.skipif(not refharness.available("tab"), reason="oracle/_ref not built")
def test_oracle_equals_the_reference_on_the_hand_made_levels(oracle_lib):
    """the judge of tests/test_gpu_baked_cells.py, pinned on the same scenes against the reference's own code"""
    R = refharness.RefHarness("tab")
    portals = 0
    for sc in bs.scenes(oracle_lib.SPHERE_DTYPE):
        O = oracle_lib.Oracle()
        R.set_level(sc.data, sc.pmap)
        O.set_level(sc.data, sc.pmap)
        R.set_spheres(sc.spheres)
        O.set_spheres(sc.spheres)
        for blur in (0, 1):
            a, za = R.render(bs.W, bs.H, sc.cam, sec=sc.sec, blur=blur)
            b, zb, st = O.render(bs.W, bs.H, sc.cam, sec=sc.sec, blur=blur, stats=True)
            assert (a == b).all(), (sc.name, blur, int((a != b).sum()))
            assert (za.view(np.uint32) == zb.view(np.uint32)).all(), (sc.name, blur)
        assert st.steps > 0
        portals += st.portals
    assert portals > 10000
