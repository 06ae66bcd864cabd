"""Tile pairs (trace_kernel.hip; PWN_TILE_PAIRS): a ticket of a frame's launch stands for a 32-pixel tile, and the wave that draws it
traces the tile's left unit and then its right one, whose add chain starts from what the left one put aside.  Every frame here is
rendered with pairs forced on (PWN_TILE_PAIRS=2) and off (0), twice through the same context -- the second launch runs on the
ticket set the first one cleared -- with the blur off and on, and must equal the oracle bit for bit in colour and in depth.  A
second launch of the same camera finds its answer in the planes already, so two frames of a camera walk follow (tests/handout.py):
no unit of those keeps what the planes held, and a launch that skipped one would show.
The shapes are one way each for the pairing to go wrong (the table at SHAPES)."""
import contextlib
import os

import numpy as np
import pytest

import step_limit as SL
from conftest import GOLD

pytestmark = pytest.mark.gpu

SEC = 1.25
SHAPES = [
    (32, 4),        # one tile, both halves
    (16, 4),        # odd units per row: the only tile has no right half
    (48, 8),        # odd units per row: a last tile with no right half
    (40, 5),        # the last tile's LEFT half partial, the bottom unit partial
    (56, 9),        # the right half partial (24 of the tile's 32 pixels)
    (2080, 36),     # 65 tiles per row: more than queues, rows go out middle-out
    (64, 4096),     # two tiles per row, many rows
    (4, 64),        # one tile per row: the division's shift-below-zero branch
]
BIG = (1000, 260)   # with one workgroup per CU: 2 080 tiles for 1 024 waves -- static first tickets, drawn tickets and the help path
BIG_VARIANTS = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "indexed": {"PWN_SPHERE_LISTS": "indexed"}, "global": {"PWN_SPHERE_LISTS": "global"}}
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


def _scene():
    if "scene" not in _cache:
        import oracle
        import pwnfps_amd
        oracle.build()
        level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
        sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
        O = oracle.Oracle()
        O.load_level(level)
        O.set_spheres(sph)
        _, _, spawn = O.get_level()
        # yawed and pitched: no row and no column of rays is special
        cam = pwnfps_amd.spawn_camera(spawn, ang_y=0.6, ang_x=-0.25)
        _cache["scene"] = (O, level, sph, cam)
    return _cache["scene"]


def _want(w, h):
    """the oracle's frame, computed once per shape: (pre-blur colour, blurred colour, depth as uint32)"""
    if (w, h) not in _cache:
        O, _, _, cam = _scene()
        pre, z = O.render(w, h, cam, sec=SEC, blur=0)
        post, z1 = O.render(w, h, cam, sec=SEC, blur=1)
        assert (z.view(np.uint32) == z1.view(np.uint32)).all()
        for a in (pre, post, z):
            a.setflags(write=False)
        _cache[(w, h)] = (pre, post, z.view(np.uint32))
    return _cache[(w, h)]


def _walked(w, h):
    """the oracle's frames of the eight launches of _check_frames on one depth plane -- per blur setting the fixed camera twice, then
    frames 1 and 2 of the walk -- as (colour, depth as uint32), computed once per shape"""
    if ("walked", w, h) not in _cache:
        import handout as H
        O, _, _, cam = _scene()
        plane = H.Shown(O, w, h)
        out = []
        for blur in (0, 1):
            for k in range(4):
                c, sec = (cam, SEC) if k < 2 else H.walk("pwnfps_level", k - 1)
                sb, z = plane.show(c, sec, blur, again=k == 1)
                sb.setflags(write=False)
                out.append((sb, z.view(np.uint32).copy()))
        _cache[("walked", w, h)] = out
    return _cache[("walked", w, h)]


def _renderer(w, h, pairs, **env):
    import pwnfps_amd
    _, level, sph, _ = _scene()
    with _env(PWN_TILE_PAIRS=pairs, **env):
        r = pwnfps_amd.Renderer(w, h)
    r.level_load(level)
    r.set_objects(sph)
    r.set_call_strips(0)             # one launch per pass: the whole frame's tiles in one set of queues
    return r


def _check_frames(w, h, **env):
    import handout as H
    pre, post, z = _want(w, h)
    walked = _walked(w, h)
    cam = _scene()[3]
    for pairs in (2, 0):
        r = _renderer(w, h, pairs, **env)
        if env.get("PWN_SPHERE_LISTS") == "global":
            assert r.sphere_tables()["form"] == 2, r.sphere_tables()
        for blur, want in ((0, pre), (1, post)):
            r.set_blur_passes(blur)
            for k in range(2):
                sb, zb = r.trace_screen_centred(cam, SEC)
                bad = sb != want
                assert not bad.any(), (w, h, pairs, blur, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
                badz = zb.view(np.uint32) != z
                assert not badz.any(), (w, h, pairs, blur, k, int(badz.sum()), np.argwhere(badz)[:4].tolist())
            # ... and two frames that the planes do not hold yet
            for k in (2, 3):
                wcam, wsec = H.walk("pwnfps_level", k - 1)
                sb, zb = r.trace_screen_centred(wcam, wsec)
                H.same((w, h, pairs, blur, k), sb, zb, *walked[4 * blur + k])
        r.close()


@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(w, h):
    assert w % 4 == 0        # (the blur runs on every shape here)
    _check_frames(w, h)


@pytest.mark.parametrize("variant", list(BIG_VARIANTS))
def test_more_tiles_than_waves(variant):
    """one workgroup per CU: the waves' static first tickets, the drawn ones and the help path all hand out tiles; the 4-lane
    kernels and the three forms of the sphere lists"""
    _check_frames(*BIG, PWN_DBG_BLOCKS_PER_CU=1, **BIG_VARIANTS[variant])


def test_default_rule_single_units_first():
    """PWN_TILE_PAIRS=1, the default, on a launch long enough for it (16 640 units for the 1 024 waves of one workgroup per CU): the
    first round goes out as single units -- four rows of them -- and the tiles behind; the counters see right halves rebuilt, but
    not in every tile of the frame"""
    w, h = 4096, 260
    pre, _, z = _want(w, h)
    cam = _scene()[3]
    for pairs in (1, 0):
        r = _renderer(w, h, pairs, PWN_DBG_BLOCKS_PER_CU=1)
        r.set_blur_passes(0)
        for k in range(2):
            sb, zb = r.trace_screen_centred(cam, SEC)
            assert (sb == pre).all() and (zb.view(np.uint32) == z).all(), (pairs, k)
        r.set_counters(True)
        sb, zb = r.trace_screen_centred(cam, SEC)
        st = r.stats()
        assert (sb == pre).all() and (zb.view(np.uint32) == z).all(), pairs
        assert st["regions"][13] == 256 * 65, st["regions"][13]
        if pairs:
            assert 0 < st["regions"][26] < 128 * 65 and st["regions"][17] == 128 * 65 - st["regions"][26], (st["regions"][17], st["regions"][26])
        else:
            assert st["regions"][26] == 0 and st["regions"][17] == 128 * 65, (st["regions"][17], st["regions"][26])
        r.close()


def test_strip_of_device_rows():
    """a strip whose rows are no multiples of 4 and that does not hold the frame's middle row, into poisoned planes: the strip's
    rows are the frame's, every other row keeps the poison"""
    import torch
    w, h = 56, 64
    pre, _, z = _want(w, h)
    cam = _scene()[3]
    poison_s, poison_z = 0x5a5a5a5a, 0x7fc12345
    for pairs in (2, 0):
        r = _renderer(w, h, pairs)
        for y0, y1 in ((5, 19), (37, 63)):
            for k in range(2):
                # (fresh poison for every launch: the second one must not find the first one's rows in the planes)
                d_sb = torch.full((h, w), poison_s, dtype=torch.int32, device="cuda")
                d_zb = torch.full((h, w), poison_z, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                r.trace_rows_device(cam, SEC, y0, y1, d_sb.data_ptr(), d_zb.data_ptr())
                torch.cuda.synchronize()
                sb = d_sb.cpu().numpy().view(np.uint32)
                zb = d_zb.cpu().numpy().view(np.uint32)
                inside = np.zeros((h, w), bool)
                inside[y0:y1] = True
                assert (sb[inside] == pre[inside]).all() and (zb[inside] == z[inside]).all(), (pairs, y0, y1, k)
                assert (sb[~inside] == poison_s).all() and (zb[~inside] == poison_z).all(), (pairs, y0, y1, k)
        r.close()


def test_counters_do_not_see_the_pairing():
    """a unit is 64 lanes in lock step either way: rays, sphere tests, wave steps and wave paths are the same with pairs on and
    off; the region counters tell the two apart (regions[17] = a right half's 16 adds, regions[26] = a right half rebuilt)"""
    w, h = 2080, 36
    cam = _scene()[3]
    seen = {}
    for pairs in (2, 0):
        r = _renderer(w, h, pairs)
        r.set_blur_passes(0)
        r.set_counters(True)
        sb, zb = r.trace_screen_centred(cam, SEC)
        st = r.stats()
        assert (sb == _want(w, h)[0]).all() and (zb.view(np.uint32) == _want(w, h)[2]).all(), pairs
        seen[pairs] = (st["rays"], st["sphere_tests"], st["wave_steps"], tuple(st["wave_paths"]))
        units = 130 * 9
        assert st["regions"][13] == units, (pairs, st["regions"][13])
        if pairs:
            assert st["regions"][17] == 0 and st["regions"][26] == units // 2, (st["regions"][17], st["regions"][26])
        else:
            assert st["regions"][17] == units // 2 and st["regions"][26] == 0, (st["regions"][17], st["regions"][26])
        r.close()
    assert seen[2] == seen[0], seen


@pytest.mark.parametrize("pairs", [2, 0])
def test_wave_steps_of_the_step_limit_frame(pairs):
    """tests/golden/step_limit.npz: the frame, its five counters and its wave steps as the fixture's step map gives them"""
    import pwnfps_amd
    import hard_scenes as HS
    f = SL.fixture()
    with _env(PWN_TILE_PAIRS=pairs):
        r = pwnfps_amd.Renderer(f.w, f.h)
    r.level_load_text(f.text)
    r.set_objects(f.sph)
    r.set_blur_passes(0)
    r.set_call_strips(0)
    r.set_counters(True)
    none = SL.none_mask(f)
    for k in range(2):
        sb, zb = r.trace_screen_centred(f.cam, f.sec)
        st = r.stats()
        assert (sb == f.pre).all(), k
        zu = np.ascontiguousarray(zb, np.float32).view(np.uint32)
        assert (zu[~none] == f.z[~none]).all(), k
        assert HS.stats5(st) == f.stats, (k, HS.stats5(st), f.stats)
        assert st["wave_steps"] == SL.wave_steps(SL.frame_units(f.smap)), k
    r.close()
