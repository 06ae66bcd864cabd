"""The oracle trick that pins the GPU ray tests, checked on the oracle alone (no GPU).

A camera whose x and y rows are zero, whose z row is D and whose w row is O gives every pixel of its frame the ray (O, D) exactly:
rayb = (0 + D) + (h/w)*0 and rdx = rdy = -0, so no add of the chain changes D (a -0 component of D becomes +0).  Pixel (x, y) of
that frame has the seed of pixel (x, y) of any frame of the same width.  So for a pixel of a real frame, the trick frame on the
pixel's record from pwn_pixel_rays must give the real frame's colour and depth at that pixel -- which makes the oracle a reference
for any ray that carries a pixel seed.
"""
import numpy as np
import pytest

import hard_scenes as HS
from conftest import level_path, load_spheres
from oracle import SPHERE_DTYPE

SCENES = HS.scenes(SPHERE_DTYPE)


def _trick_cam(rec):
    cam = np.zeros((4, 4), np.float32)
    cam[2] = rec[4:]
    cam[3] = rec[:4]
    return cam


def _check(O, w, h, cam, sec, rng, k, name):
    import pwnfps_amd
    sb, zb, _ = O.trace_rows(w, h, 0, h, cam, sec=np.float32(sec))
    xy = np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], 1).astype(np.int32)
    xy[0] = (w - 1, h - 1)
    rays, seeds, _ = pwnfps_amd.pixel_rays(w, h, cam, xy)
    checked = 0
    for (x, y), rec, seed in zip(xy, rays, seeds):
        assert seed == O.L.pwno_pixel_seed(int(x), int(y), w)
        if (np.signbit(rec[4:]) & (rec[4:] == 0)).any():
            continue                               # (the trick gives +0 where the frame's ray has -0)
        tsb, tzb, _ = O.trace_rows(w, y + 1, y, y + 1, _trick_cam(rec), sec=np.float32(sec), threads=1)
        assert tsb[y, x] == sb[y, x], (name, int(x), int(y))
        assert HS.bits(tzb[y, x:x + 1])[0] == HS.bits(zb[y, x:x + 1])[0], (name, int(x), int(y))
        checked += 1
    assert checked >= k // 2, name


def test_trick_on_golden_cameras(oracle_lib, cases):
    rng = np.random.default_rng(4242)
    Os = {}
    done = 0
    for c in cases:
        if c["w"] * c["h"] > 1280 * 720:
            continue
        key = (c["level"], c["spheres"])
        if key not in Os:
            O = oracle_lib.Oracle()
            O.load_level(level_path(c["level"]))
            O.set_spheres(load_spheres(c["spheres"]))
            Os[key] = O
        _check(Os[key], c["w"], c["h"], np.array(c["cam"], np.float32).reshape(4, 4), c["sec"], rng, 12, c["name"])
        done += 1
    assert done >= 15


@pytest.mark.parametrize("sc", SCENES, ids=[s.name for s in SCENES])
def test_trick_on_hard_scene_cameras(oracle_lib, sc):
    O = HS.oracle(oracle_lib, sc)
    _check(O, sc.w, sc.h, sc.cam, sc.sec, np.random.default_rng(len(sc.name)), 8, sc.name)
