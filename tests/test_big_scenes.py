"""Sphere tables that outgrow LDS, the part that needs no GPU: the scenes of tests/big_scenes.py are what they are meant to be (each
breaks one of the rules that kept a sphere set on chip, and shows in the frame), and pwn_sphere_tables_plan -- host only -- reports
the form, the sizes and the shape of the tables an upload would make.

The scenes come from numpy's seeded generator.  Inequalities are asserted, no exact counts: a numpy whose stream differs makes a
scene fail here, not a kernel elsewhere."""
import ctypes as C

import numpy as np
import pytest

import big_scenes as BS
import hit_chain as HC
from conftest import level_path, load_spheres

PWN_OK, PWN_EINVAL, PWN_ETOOBIG = 0, -1, -7
T_BINIDX, BLOB_MAX, LIST_END, LDS_EXTRA = 25824, 72 * 1024, 0xffff, 16      # tables.h, pwn_internal.h, trace_kernel.hip


def _pad16(v):
    return (v + 15) & ~15


def _indexed_bytes(nbin, n):
    return _pad16(T_BINIDX + _pad16(2 * nbin) + 32 * n)


def _inline_bytes(pairs, n):
    return _pad16(T_BINIDX + 16 * pairs + _pad16(2 * pairs) + 32 * n)


@pytest.mark.parametrize("name", BS.NAMES)
def test_scene_breaks_its_rule_and_shows(oracle_lib, name):
    sc = BS.scene(name, oracle_lib)
    n = len(sc.spheres)
    pairs, cells, longest, nbin = BS.bins(sc, oracle_lib)
    offsets_16bit = n * 32 >= LIST_END
    blob = _indexed_bytes(nbin, n) > BLOB_MAX
    entries = nbin > 32767
    if name in ("swarm_near", "swarm_all"):
        assert offsets_16bit and blob, (n, nbin)
        assert n == (2100 if name == "swarm_near" else 10000)
    elif name == "fat":
        assert entries and not offsets_16bit and n == 800, (n, nbin)
        assert longest > 100                       # long lists: the end marks and the read-ahead get their turn
    else:
        # one sphere over: the first k load on chip, k + 1 do not
        under, over = BS.one_over_pair(oracle_lib)
        assert len(over.spheres) == len(under.spheres) + 1 == n
        p_u, _, _, nbin_u = BS.bins(under, oracle_lib)
        assert not (len(under.spheres) * 32 >= LIST_END or nbin_u > 32767 or _indexed_bytes(nbin_u, len(under.spheres)) > BLOB_MAX)
        assert offsets_16bit or blob or entries
    # every camera sees the spheres: a good part of the frame differs from the empty level's, and no ray runs out of steps
    O = BS.oracle_for(sc, oracle_lib)
    E = oracle_lib.Oracle()
    E.load_level(level_path(sc.level))
    for cam in BS.cameras(sc.spawn, oracle_lib):
        sb, _, st = O.render(160, 120, cam, blur=0, stats=True)
        eb, _ = E.render(160, 120, cam, blur=0)
        assert st.exhausted == 0
        assert (sb != eb).mean() > 0.25, (name, float((sb != eb).mean()))


def test_swarm_all_first_hits_reach_objects_past_2048(oracle_lib):
    """the object numbers that 16-bit byte offsets cannot name are among the first hits of all three 32 x 24 views"""
    sc = BS.scene("swarm_all", oracle_lib)
    rd = HC.Reader(BS.oracle_for(sc, oracle_lib))
    for cam in BS.cameras(sc.spawn, oracle_lib):
        ref = rd.pixels(32, 24, cam, HC.all_pixels(32, 24))
        assert (ref.want["object"] >= 2048).sum() > 0


def test_plan_on_the_scenes_that_load_on_chip():
    """t0, synth64, synth256: the form pwn_i_pack_blob picks for them (inline, inline, indexed by its comment) and that blob's bytes"""
    import pwnfps_amd
    for key, form in (("t0", 1), ("synth64", 1), ("synth256", 0)):
        sph = load_spheres(key)
        p = pwnfps_amd.sphere_tables_plan(sph)
        assert p["form"] == form and p["device_bytes"] == 0, (key, p)
        nbin = p["pairs"] + p["cells"]
        want = _inline_bytes(p["pairs"], len(sph)) if form == 1 else _indexed_bytes(nbin, len(sph))
        assert p["lds_bytes"] == want + LDS_EXTRA, (key, p, want)
    p = pwnfps_amd.sphere_tables_plan(load_spheres("none"))
    assert p == {"form": 0, "lds_bytes": T_BINIDX + LDS_EXTRA, "device_bytes": 0, "pairs": 0, "cells": 0, "longest": 0}


@pytest.mark.parametrize("name", BS.NAMES)
def test_plan_on_the_big_scenes(oracle_lib, name):
    import pwnfps_amd
    sc = BS.scene(name, oracle_lib)
    n = len(sc.spheres)
    pairs, cells, longest, _ = BS.bins(sc, oracle_lib)
    p = pwnfps_amd.sphere_tables_plan(sc.spheres)
    assert p["form"] == 2
    assert (p["pairs"], p["cells"], p["longest"]) == (pairs, cells, longest)
    assert p["device_bytes"] == 16 * (pairs + 1) + _pad16(4 * pairs) + 32 * n
    assert p["device_bytes"] - (20 * pairs + 16 + 32 * n) in range(0, 16)
    assert p["lds_bytes"] == T_BINIDX + _pad16(4 * cells) + LDS_EXTRA
    assert p["lds_bytes"] <= 25824 + 4 * 4096 + 16
    if name == "one_over":
        under, _ = BS.one_over_pair(oracle_lib)
        assert pwnfps_amd.sphere_tables_plan(under.spheres)["form"] <= 1


def test_plan_refuses_and_rejects():
    import pwnfps_amd
    from pwnfps_amd import _lib
    big = np.zeros(4096, BS.SPHERE_DTYPE)
    big["r"] = 100.0
    big["x"] = big["z"] = 32.0
    big["y"] = 0.5
    out = (C.c_uint64 * 6)()
    assert _lib.lib.pwn_sphere_tables_plan(big.ctypes.data, len(big), out) == PWN_ETOOBIG
    assert out[0] == 2 and out[3] == 4096 * 4096 and out[2] > _lib.PWN_TABLES_MAX        # 16.8 M pairs: what would not fit is reported
    with pytest.raises(pwnfps_amd.PwnError) as e:
        pwnfps_amd.sphere_tables_plan(big)
    assert e.value.code == PWN_ETOOBIG
    assert _lib.lib.pwn_sphere_tables_plan(None, 4, out) == PWN_EINVAL
    assert _lib.lib.pwn_sphere_tables_plan(None, 0, out) == PWN_EINVAL
    assert _lib.lib.pwn_sphere_tables_plan(big.ctypes.data, -1, out) == PWN_EINVAL
    assert _lib.lib.pwn_sphere_tables_plan(big.ctypes.data, _lib.PWN_OBJ_MAX + 1, out) == PWN_EINVAL
    assert _lib.lib.pwn_sphere_tables_plan(big.ctypes.data, 4, None) == PWN_EINVAL
    assert _lib.lib.pwn_sphere_tables_state(None, out) == PWN_EINVAL
    # the largest table there can be of small spheres: PWN_OBJ_MAX spheres of 3 x 3 cells each, about 2 MB
    rng = np.random.default_rng(3)
    s = np.zeros(_lib.PWN_OBJ_MAX, BS.SPHERE_DTYPE)
    s["x"], s["z"] = rng.uniform(2, 62, len(s)), rng.uniform(2, 62, len(s))
    s["r"] = 1.0
    p = pwnfps_amd.sphere_tables_plan(s)
    assert p["form"] == 2 and 9 * len(s) * 20 <= p["device_bytes"] - 32 * len(s) <= 9 * len(s) * 20 + 48
    assert b"PWN_TABLES_MAX" in _lib.lib.pwn_strerror(PWN_ETOOBIG)
    # spheres piled into one cell: a list of PWN_LIST_MAX loads, a longer one is refused as it always was
    pile = np.zeros(5000, BS.SPHERE_DTYPE)
    pile["r"], pile["x"], pile["y"], pile["z"] = 0.1, 9.5, 0.3, 5.5
    assert _lib.lib.pwn_sphere_tables_plan(pile.ctypes.data, 5000, out) == PWN_ETOOBIG and out[5] == 5000
    p = pwnfps_amd.sphere_tables_plan(pile[:4096])
    assert p["form"] == 2 and p["longest"] == 4096 and p["cells"] == 1
