"""The step-limit fixture (tests/step_limit.py, tools/gen_step_limit.py) pinned without a GPU: what it stores is what the oracle
computes, the frame holds every kind of pixel the GPU test needs, and the compiled reference renders the same frame."""
import ctypes as C

import numpy as np
import pytest

import hit_chain as HC
import refharness
import step_limit as SL


def _oracle(oracle_lib, f):
    O = oracle_lib.Oracle()
    O.load_level_text(f.text)
    O.set_spheres(f.sph)
    return O


def test_fixture_is_the_oracle_and_holds_every_kind(oracle_lib):
    f = SL.fixture()
    assert (f.w, f.h) == (64, 16)
    O = _oracle(oracle_lib, f)
    smap = np.zeros((f.h, f.w, 3), np.uint16)
    zb = np.full((f.h, f.w), SL.SENTINEL, np.uint32).view(np.float32)
    O.L.pwno_step_map.argtypes = [C.c_void_p]
    O.L.pwno_step_map(smap.ctypes.data)
    try:
        sb, zb, st = O.trace_rows(f.w, f.h, 0, f.h, f.cam, sec=np.float32(f.sec), threads=1, zb=zb)
    finally:
        O.L.pwno_step_map(None)
    assert (sb == f.pre).all() and (zb.view(np.uint32) == f.z).all() and (smap == f.smap).all()
    assert (st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted) == f.stats
    assert st.steps == int(smap.sum(dtype=np.int64))

    none = SL.none_mask(f)
    s0 = smap[:, :, 0]
    assert int(s0.max()) == SL.LIMIT and (s0[none] == SL.LIMIT).all()
    # the primary segment: an event in iteration 999, one in iteration 1000, and 1000 iterations without an event (what would have
    # been an event in iteration 1001 or later) -- the three that may not be missing
    assert ((s0 == SL.LIMIT - 1) & ~none).sum() >= 1
    assert ((s0 == SL.LIMIT) & ~none).sum() >= 1
    assert none.sum() >= 1
    # a segment other than the primary one out of steps: the frame's count beyond the primary rays', and a later segment at the limit
    assert st.exhausted > int(none.sum())
    assert (smap[:, :, 1:] == SL.LIMIT).any()

    # the stored records: PWN_HIT_NONE exactly where the primary ray runs out of steps, elsewhere the depth plane's distance
    hits = f.hits.reshape(f.h, f.w)
    assert ((hits["kind"] == HC.NONE) == none).all()
    assert (HC._bits(hits["dist"])[~none] == f.z[~none]).all()
    for name in HC.HIT_DTYPE.names:
        assert (hits[name][none] == (-1 if name in ("face", "object") else 0)).all(), name
    # a side-wall event and a floor / ceiling event in iteration 1000
    last = (s0 == SL.LIMIT) & ~none
    assert (last & (hits["kind"] == HC.WALL) & np.isin(hits["face"], (HC.FXP, HC.FZP, HC.FXN, HC.FZN))).sum() >= 1
    assert (last & (hits["kind"] == HC.WALL) & np.isin(hits["face"], (HC.FYP, HC.FYN))).sum() >= 1

    # ... are the oracle's event chains: every other pixel that ends in iteration 999 or 1000, every eighth of the others
    idx = np.concatenate([np.flatnonzero(((s0 >= SL.LIMIT - 1) & ~none).ravel())[::2], np.flatnonzero(none.ravel())[::8],
                          np.flatnonzero((s0 < SL.LIMIT - 1).ravel())[::8]])
    assert len(idx) >= 40
    xy = HC.all_pixels(f.w, f.h)[idx]
    ref = HC.Reader(O).pixels(f.w, f.h, f.cam, xy)
    assert len(HC.mismatches(ref.want, f.hits[idx], f.cmp_dy[idx])) == 0
    assert (ref.cmp_dy == f.cmp_dy[idx]).all() and (ref.steps == s0.ravel()[idx]).all()


@pytest.mark.skipif(not refharness.available("tab"), reason="oracle/_ref not built")
def test_oracle_equals_the_compiled_reference(oracle_lib, tmp_path):
    f = SL.fixture()
    path = str(tmp_path / "step_limit.txt")
    with open(path, "w", newline="") as fh:
        fh.write(f.text)
    R = refharness.RefHarness("tab")
    R.load_level(path)
    R.set_spheres(f.sph)
    O = _oracle(oracle_lib, f)
    for blur in (0, 1):
        a, za = R.render(f.w, f.h, f.cam, sec=f.sec, blur=blur)
        b, zb = O.render(f.w, f.h, f.cam, sec=f.sec, blur=blur)
        assert (a == b).all(), (blur, int((a != b).sum()))
        assert (za.view(np.uint32) == zb.view(np.uint32)).all(), blur
    # (the frame the fixture stores: no blur, and zero depth where the stored plane keeps its sentinel)
    a, za = R.render(f.w, f.h, f.cam, sec=f.sec, blur=0)
    none = SL.none_mask(f)
    assert (a == f.pre).all()
    assert (za.view(np.uint32)[~none] == f.z[~none]).all() and (za.view(np.uint32)[none] == 0).all()
