"""The hard scenes (tests/hard_scenes.py) as inputs of the sphere lists' device-memory form (tables.h PWN_LF_GLOBAL), the part
that needs no GPU.  The GPU tests send every hard scene through that form by PWN_SPHERE_LISTS=global: here pwn_sphere_tables_plan
-- host only -- says that the variable forces the form for every one of them, and the oracle's binning says that the corpus
holds the list shapes those tests count on: a one-record list, a list of 300, boxes that leave the grid, two equal spheres in
one cell, r * r of zero and a denormal one.

Inequalities are asserted, no exact counts: an edit of the corpus that removes a shape fails here instead of weakening the GPU
tests in silence."""
import numpy as np
import pytest

import hard_scenes as HS
from oracle import SPHERE_DTYPE

SCENES = HS.scenes(SPHERE_DTYPE)
IDS = [s.name for s in SCENES]
FLT_MIN = np.float32(1.17549435e-38)


@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_the_variable_forces_the_form(sc, monkeypatch):
    """form 2 with PWN_SPHERE_LISTS=global -- a scene without spheres or with none in a cell too --, a form on chip without"""
    import pwnfps_amd
    monkeypatch.delenv("PWN_SPHERE_LISTS", raising=False)
    free = pwnfps_amd.sphere_tables_plan(sc.spheres)
    assert free["form"] in (0, 1) and free["device_bytes"] == 0, (sc.name, free)
    monkeypatch.setenv("PWN_SPHERE_LISTS", "global")
    forced = pwnfps_amd.sphere_tables_plan(sc.spheres)
    assert forced["form"] == 2, (sc.name, forced)
    # the same lists either way; the records, one spare behind them, which[] and the spheres lie in device memory
    assert [forced[k] for k in ("pairs", "cells", "longest")] == [free[k] for k in ("pairs", "cells", "longest")]
    assert forced["device_bytes"] >= 16 * (forced["pairs"] + 1) + 4 * forced["pairs"] + 32 * len(sc.spheres)
    # any other word leaves the choice to the size rules
    monkeypatch.setenv("PWN_SPHERE_LISTS", "globl")
    assert pwnfps_amd.sphere_tables_plan(sc.spheres)["form"] == free["form"]


_shapes = {}


def _shape(oracle_lib, sc):
    """what the oracle's binning (level.h:1-39 with the cells outside the grid skipped) makes of the scene's spheres"""
    if sc.name not in _shapes:
        O = oracle_lib.Oracle()
        HS.load_oracle(O, sc)
        counts, idx = O.get_bins()
        counts = counts.astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts)])
        s = sc.spheres
        geom = np.stack([s[f] for f in ("r", "x", "y", "z")], 1).astype(np.float32).view(np.uint32)
        colour = np.stack([s[f] for f in ("refl", "cb", "cg", "cr")], 1).astype(np.float32).view(np.uint32)
        # two spheres of one list whose r, x, y, z are the same bits and whose shading is not: which of them a ray keeps shows
        twins = 0
        for c in np.flatnonzero(counts >= 2):
            members = idx[off[c]:off[c + 1]]
            _, group = np.unique(geom[members], axis=0, return_inverse=True)
            group = group.reshape(-1)
            for g in np.flatnonzero(np.bincount(group) >= 2):
                twins += int(len(np.unique(colour[members[group == g]], axis=0)) >= 2)
        # the cells of every sphere's box, in the grid or not (float32 sums, truncated as the C conversion does)
        lo_x, hi_x = np.trunc(s["x"] - s["r"]), np.trunc(s["x"] + s["r"])
        lo_z, hi_z = np.trunc(s["z"] - s["r"]), np.trunc(s["z"] + s["r"])
        box_cells = int((np.maximum(hi_x - lo_x + 1, 0) * np.maximum(hi_z - lo_z + 1, 0)).sum())
        outside = int(((lo_x < 0) | (hi_x > 63) | (lo_z < 0) | (hi_z > 63)).sum())
        with np.errstate(under="ignore"):
            r2 = (s["r"] * s["r"]).astype(np.float32)
        binned = np.zeros(len(s), bool)
        binned[idx] = True
        _shapes[sc.name] = {"pairs": int(counts.sum()), "cells": int((counts > 0).sum()), "longest": int(counts.max()),
                            "twins": twins, "box_cells": box_cells, "outside": outside,
                            "r2_zero": int(((r2 == 0) & binned).sum()),
                            "r2_denormal": int(((r2 != 0) & (np.abs(r2) < FLT_MIN) & binned).sum())}
    return _shapes[sc.name]


def _with(oracle_lib, pred):
    return [sc.name for sc in SCENES if pred(_shape(oracle_lib, sc))]


def test_plan_agrees_with_the_oracles_binning(oracle_lib, monkeypatch):
    import pwnfps_amd
    monkeypatch.setenv("PWN_SPHERE_LISTS", "global")
    for sc in SCENES:
        p, q = pwnfps_amd.sphere_tables_plan(sc.spheres), _shape(oracle_lib, sc)
        assert (p["pairs"], p["cells"], p["longest"]) == (q["pairs"], q["cells"], q["longest"]), (sc.name, p, q)


def test_corpus_has_one_record_lists(oracle_lib):
    """the first record is the last one: its end mark is set, and the read-ahead lands on the spare record behind the table"""
    names = _with(oracle_lib, lambda q: q["longest"] == 1 and q["pairs"] >= 1)
    assert len(names) >= 1, names
    # ... among them lists whose one record is all the table holds
    assert len(_with(oracle_lib, lambda q: q["longest"] == 1 and q["pairs"] == q["cells"] == 1)) >= 1


def test_corpus_has_a_list_of_300(oracle_lib):
    names = _with(oracle_lib, lambda q: q["longest"] >= 300)
    assert len(names) >= 1, names
    # on tiny and ragged frames too: fewer pixels than a wave has lanes, a width that is no multiple of 4 or 16
    sizes = {(sc.w, sc.h) for sc in SCENES if sc.name in names}
    assert any(w * h < 64 for w, h in sizes) and any(w % 4 != 0 for w, h in sizes) and any(w * h >= 64 * 256 for w, h in sizes)


def test_corpus_has_boxes_that_leave_the_grid(oracle_lib):
    """... and the cells outside got no entry: fewer pairs than the boxes have cells"""
    names = _with(oracle_lib, lambda q: q["outside"] >= 1 and q["pairs"] < q["box_cells"])
    assert len(names) >= 1, names
    for sc in SCENES:
        q = _shape(oracle_lib, sc)
        assert q["pairs"] <= q["box_cells"] and (q["outside"] > 0 or q["pairs"] == q["box_cells"]), (sc.name, q)


def test_corpus_has_equal_spheres_in_one_cell(oracle_lib):
    assert len(_with(oracle_lib, lambda q: q["twins"] >= 1)) >= 1


def test_corpus_has_a_zero_and_a_denormal_square_of_the_radius(oracle_lib):
    """the end mark is the sign bit of r * r, which the host flushes to zero below FLT_MIN as the reference build does: the
    record of either sphere holds -0.0, and the walk has to mask the bit before the sphere test"""
    assert len(_with(oracle_lib, lambda q: q["r2_zero"] >= 1)) >= 1
    assert len(_with(oracle_lib, lambda q: q["r2_denormal"] >= 1)) >= 1
