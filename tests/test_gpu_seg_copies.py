"""The units kernel holds a ray segment's text once per bounce depth (trace_segment.inc): three different programs, and lanes of one
wave leave the ray in each of them.  The frames of tests/golden/seg_copies.npz (tools/gen_seg_copies.py, which reads every pixel's
exits off the oracle's event chain before it writes them) are 64 x 16 -- four units across, four rows of units -- and hold
    sphere      a sphere of reflectivity 0 met by the primary ray, behind a wall mirror and behind the floor, one unit with all depths;
    fog         the same in fog cells: fog behind rays of depth 0, 1 and 2 and in both entries of the composite stack;
    corridors   rays out of steps in the first, the second and the third segment;
    mixed       one unit whose lanes end on the sphere, out of steps and in the last copy, fog behind them.
Colour, depth and the counting variants' counters equal the oracle's bit for bit: the 3-lane and the 4-lane variant, the three
forms of the sphere lists, tile pairs on and off, and once each the views, viewports and rays calls at the same size."""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
from conftest import GOLD

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7fc12345)          # a NaN pattern no computation makes
LANES = {"lanes3": {}, "lanes4": {"PWN_DBG_FORCE_HASW": "1"}}
LISTS = ("indexed", "inline", "global")
# what tools/gen_seg_copies.py found in each frame, asked for again here (its `holds` of the fixture)
NEED = {"sphere": ("refl0_0", "refl0_1_wall", "refl0_1_floor", "last", "units_all_depths"),
        "fog": ("fog_end_0", "fog_end_1", "fog_end_2", "fog_a_1", "fog_a_2", "fog_b_2", "units_all_depths"),
        "corridors": ("steps_0", "steps_1", "steps_2", "last"),
        "mixed": ("units_all_kinds", "units_all_depths", "steps_0", "fog_a_1", "fog_b_2")}
_cache = {}


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _scenes():
    """{name: dict(text, sph, cam, sec, pre, z, stats, holds)}, w, h"""
    if "s" not in _cache:
        from oracle import SPHERE_DTYPE
        k = np.load(os.path.join(GOLD, "seg_copies.npz"))
        w, h = (int(v) for v in k["wh"])
        out = {}
        for name in (str(n) for n in k["names"]):
            out[name] = dict(text=str(k[name + "_text"]), sph=np.ascontiguousarray(k[name + "_sph"], SPHERE_DTYPE),
                             cam=np.ascontiguousarray(k[name + "_cam"], np.float32), sec=float(k[name + "_sec"]),
                             pre=k[name + "_pre"], z=k[name + "_z"], stats=tuple(int(v) for v in k[name + "_stats"]),
                             holds={str(a): int(b) for a, b in k[name + "_holds"]})
        _cache["s"] = (out, w, h)
    return _cache["s"]


def test_fixture_holds_every_exit():
    """(no GPU work: the fixture is the one the generator checked)"""
    scenes, w, h = _scenes()
    assert (w, h) == (64, 16) and set(scenes) == set(NEED)
    for name, need in NEED.items():
        for key in need:
            assert scenes[name]["holds"][key] > 0, (name, key)
        assert scenes[name]["pre"].shape == (h, w) and scenes[name]["z"].shape == (h, w)
    assert (scenes["corridors"]["z"] == SENTINEL).sum() == scenes["corridors"]["holds"]["steps_0"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _renderer(w, h, lanes, lists, pairs):
    import pwnfps_amd
    with _env(PWN_SPHERE_LISTS=lists, PWN_TILE_PAIRS=pairs, **LANES[lanes]):
        r = pwnfps_amd.Renderer(w, h)
    r.set_blur_passes(0)
    r.set_call_strips(0)
    return r


def _load(r, s, lists):
    r.level_load_text(s["text"])
    r.set_objects(s["sph"])
    if lists == "global":
        assert r.sphere_tables()["form"] == 2, r.sphere_tables()


def _frame(r, s, w, h, what):
    """the device rows into planes filled with the sentinel, without and with the counters: colour, depth, counters"""
    import torch
    for count in (False, True):
        r.set_counters(count)
        d_sb = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        d_zb = torch.full((h, w), int(SENTINEL), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.trace_rows_device(s["cam"], s["sec"], 0, h, d_sb.data_ptr(), d_zb.data_ptr())
        torch.cuda.synchronize()
        sb = d_sb.cpu().numpy().view(np.uint32)
        z = d_zb.cpu().numpy().view(np.uint32)
        bad = sb != s["pre"]
        assert not bad.any(), (what, count, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        badz = z != s["z"]
        assert not badz.any(), (what, count, int(badz.sum()), np.argwhere(badz)[:4].tolist())
        if count:
            st = r.stats()
            assert HS.stats5(st) == s["stats"], (what, HS.stats5(st), s["stats"])


@pytest.mark.parametrize("lists", LISTS)
@pytest.mark.parametrize("lanes", list(LANES))
def test_frames(lanes, lists):
    scenes, w, h = _scenes()
    for pairs in (2, 0):
        r = _renderer(w, h, lanes, lists, pairs)
        for name, s in scenes.items():
            _load(r, s, lists)
            _frame(r, s, w, h, (name, lanes, lists, pairs))
        r.close()


@pytest.mark.parametrize("lanes", list(LANES))
def test_views_viewports_rays(lanes):
    """the same frames through the batch calls: every scene as a batch of two views (the second one's time differs: its pixels are
    not compared), as one viewport that fills the frame, and as caller-supplied rays in the order of the frame's units"""
    import pwnfps_amd
    scenes, w, h = _scenes()
    r = _renderer(w, h, lanes, "indexed", 1)
    for name, s in scenes.items():
        _load(r, s, "indexed")
        none = s["z"] == SENTINEL
        for count in (False, True):
            r.set_counters(count)
            sb, zb = r.trace_views(np.stack([s["cam"], s["cam"]]), np.array([s["sec"], s["sec"] + 0.5], np.float32))
            assert (sb[0] == s["pre"]).all(), (name, lanes, count, "views")
            assert (_bits(zb[0])[~none] == s["z"][~none]).all(), (name, lanes, count, "views")
            sb, zb = r.trace_viewports(np.array([[0, 0, w, h]], np.int32), s["cam"][None], np.array([s["sec"]], np.float32))
            assert (sb == s["pre"]).all(), (name, lanes, count, "viewports")
            assert (_bits(zb)[~none] == s["z"][~none]).all(), (name, lanes, count, "viewports")
            rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, s["cam"], order="units")
            idx = xy[:, 1] * w + xy[:, 0]
            z = np.full(len(rays), SENTINEL, np.uint32).view(np.float32)
            col, z = r.trace_rays(rays, seeds, s["sec"], depth=z)
            assert (col == s["pre"].ravel()[idx]).all(), (name, lanes, count, "rays")
            assert (_bits(z) == s["z"].ravel()[idx]).all(), (name, lanes, count, "rays")
            if count:
                assert HS.stats5(r.stats()) == s["stats"], (name, lanes, "rays")
    r.close()
