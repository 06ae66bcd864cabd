"""tests/golden/step_limit.npz (tools/gen_step_limit.py): a 64 x 16 frame of a hall of portal-closed corridors whose rays end around
the walk's step limit (trace.h:250: 1000 cell steps) -- events in iteration 999 and 1000 of the primary segment, primary rays out of
steps, and a later segment out of steps.  The fixture holds the scene and what the oracle made of it: the pre-blur colour, the depth
over a sentinel-filled plane, the step map, the five counters and every pixel's first-hit record (tests/hit_chain.py).
tests/test_step_limit.py pins all of that on the oracle; the GPU tests compare with the stored arrays."""
import os
from collections import namedtuple

import numpy as np

import hit_chain as HC
from conftest import GOLD

SENTINEL = np.uint32(0x7fc12345)          # a NaN pattern no computation makes
LIMIT = 1000                              # trace.h:250
Fixture = namedtuple("Fixture", "text cam sph sec w h pre z smap stats hits cmp_dy")
_cache = {}


def fixture():
    if "f" not in _cache:
        from oracle import SPHERE_DTYPE
        k = np.load(os.path.join(GOLD, "step_limit.npz"))
        w, h = (int(v) for v in k["wh"])
        _cache["f"] = Fixture(str(k["text"]), np.ascontiguousarray(k["cam"], np.float32), np.ascontiguousarray(k["sph"], SPHERE_DTYPE),
                              float(k["sec"]), w, h, k["pre"], k["z"], k["smap"], tuple(int(v) for v in k["stats"]),
                              np.ascontiguousarray(k["hits"], HC.HIT_DTYPE), k["cmp_dy"])
    return _cache["f"]


def none_mask(f):
    """(h, w): the pixels whose primary ray runs out of steps -- the depth plane keeps its sentinel there"""
    return f.z == SENTINEL


def wave_steps(steps):
    """the kernel's wave_steps counter from per-lane, per-segment walk iterations (n_units, 64, segments): a wave walks its 64 lanes
    in lock step segment by segment, so a unit costs the sum over the segments of the longest lane (tools/unit_shapes.py)"""
    return int(steps.max(axis=1).sum(dtype=np.int64))


def frame_units(smap):
    """(h, w, 3) step map -> (n_units, 64, 3): the frame's 16 x 4-pixel units (h % 4 == 0 and w % 16 == 0 here)"""
    h, w, s = smap.shape
    return smap.reshape(h // 4, 4, w // 16, 16, s).transpose(0, 2, 1, 3, 4).reshape(-1, 64, s)


def batch_units(steps):
    """(n, segments) walk iterations of a batch of rays in the caller's order -> (n_units, 64, segments), the last unit padded"""
    n, s = steps.shape
    pad = (-n) % 64
    return np.concatenate([steps, np.zeros((pad, s), steps.dtype)]).reshape(-1, 64, s)
