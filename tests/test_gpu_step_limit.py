"""The walk's step limit (trace.h:250) on the GPU: the frame of tests/step_limit.py -- primary segments that end on an event in
iteration 999 and in iteration 1000, primary and later segments that run out of steps -- through the blocking call, the device
rows, the refill scheduler and, as caller-supplied rays, pwn_trace_rays and pwn_trace_hits, in every variant a context can pick.
Colour, depth, counters and hit records equal the oracle's (stored in the fixture, pinned in tests/test_step_limit.py) bit for
bit; a primary ray out of steps leaves the depth it found (trace.h:677)."""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
import hit_chain as HC
import step_limit as SL

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "inline": {"PWN_SPHERE_LISTS": "inline"},
            "indexed": {"PWN_SPHERE_LISTS": "indexed"}, "global": {"PWN_SPHERE_LISTS": "global"}}


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


def _renderer(f, variant, scheduler=None):
    import pwnfps_amd
    with _env(**VARIANTS[variant]):
        r = pwnfps_amd.Renderer(f.w, f.h)
    r.level_load_text(f.text)
    r.set_objects(f.sph)
    if variant == "global":
        assert r.sphere_tables()["form"] == 2, r.sphere_tables()
    r.set_blur_passes(0)
    if scheduler is not None:
        r.set_scheduler(scheduler)
    r.set_counters(True)
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(f, r, units_scheduler):
    """the blocking call twice on the context's own plane (zero where nothing was hit), then the device rows twice into a plane
    filled with the sentinel: colour, depth, counters"""
    import torch
    none = SL.none_mask(f)
    for k in range(2):
        sb, zb = r.trace_screen_centred(f.cam, f.sec)
        st = r.stats()
        bad = sb != f.pre
        assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (_bits(zb)[~none] == f.z[~none]).all() and (_bits(zb)[none] == 0).all(), k
        assert HS.stats5(st) == f.stats, (k, HS.stats5(st), f.stats)
        if units_scheduler:
            assert st["wave_steps"] == SL.wave_steps(SL.frame_units(f.smap)), k
    d_sb = torch.zeros((f.h, f.w), dtype=torch.int32, device="cuda")
    d_zb = torch.full((f.h, f.w), int(SL.SENTINEL), dtype=torch.int32, device="cuda")
    for k in range(2):
        torch.cuda.synchronize()
        r.trace_rows_device(f.cam, f.sec, 0, f.h, d_sb.data_ptr(), d_zb.data_ptr())
        torch.cuda.synchronize()
        assert (d_sb.cpu().numpy().view(np.uint32) == f.pre).all(), k
        z = d_zb.cpu().numpy().view(np.uint32)
        assert (z == f.z).all(), (k, int((z != f.z).sum()))
        assert (z[none] == SL.SENTINEL).all() and int(none.sum()) >= 1
        st = r.stats()
        assert HS.stats5(st) == f.stats, (k, HS.stats5(st), f.stats)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_frame(variant):
    """the blocking call and the device rows: the default variant, the 4-lane one, the three forms of the sphere lists"""
    f = SL.fixture()
    r = _renderer(f, variant)
    _frames(f, r, True)
    r.close()


@pytest.mark.parametrize("variant", ["plain", "force_hasw"])
def test_frame_refill_scheduler(variant):
    """the refill kernel keeps a step count per lane (trace_refill.hip): the same frame, steps and exhausted rays"""
    f = SL.fixture()
    r = _renderer(f, variant, scheduler="refill")
    _frames(f, r, False)
    r.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rays_and_hits(variant):
    """the frame's pixels as caller-supplied rays, in row order and in the order of the frame's units: pwn_trace_rays into a depth
    array filled with the sentinel, twice; pwn_trace_hits: PWN_HIT_NONE exactly where the oracle runs out of steps"""
    import pwnfps_amd
    f = SL.fixture()
    r = _renderer(f, variant)
    none = SL.none_mask(f)
    for order in ("rows", "units"):
        rays, seeds, xy = pwnfps_amd.pixel_rays(f.w, f.h, f.cam, order=order)
        idx = xy[:, 1] * f.w + xy[:, 0]
        steps = f.smap[xy[:, 1], xy[:, 0]]
        z = np.full(len(rays), SL.SENTINEL, np.uint32).view(np.float32)
        for k in range(2):
            col, z = r.trace_rays(rays, seeds, f.sec, depth=z)
            st = r.stats()
            assert (col == f.pre.ravel()[idx]).all(), (order, k)
            assert (_bits(z) == f.z.ravel()[idx]).all(), (order, k)
            assert (_bits(z)[none.ravel()[idx]] == SL.SENTINEL).all()
            assert HS.stats5(st) == f.stats, (order, k, HS.stats5(st), f.stats)
            assert st["wave_steps"] == SL.wave_steps(SL.batch_units(steps)), (order, k)
        hits = r.trace_hits(rays)
        st = r.stats()
        want = f.hits[idx]
        bad = HC.mismatches(hits, want, f.cmp_dy[idx])
        assert len(bad) == 0, (order, len(bad), [(int(i), hits[i].tolist(), want[i].tolist()) for i in bad[:3]])
        assert ((hits["kind"] == HC.NONE) == none.ravel()[idx]).all()
        assert st["rays"] == len(rays) and st["steps"] == int(steps[:, 0].sum(dtype=np.int64)), order
        assert st["exhausted"] == int(none.sum()), order
        assert st["wave_steps"] == SL.wave_steps(SL.batch_units(steps[:, :1])), order
    r.close()
