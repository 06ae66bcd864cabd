"""pwn_trace_hits_hide_device: ray i does not see sphere hide[i].  Every record is the 48 bytes pwn_trace_hits_device writes for that ray
on a context whose table lacks entry hide[i], with `object` in the FULL table's numbering.  The rays: the pixel rays of the three
cameras of tests/hide_scenes.py and hand-made rays that start inside sphere 0; each ray draws its own hidden sphere."""
import ctypes as C
import functools

import numpy as np
import pytest

import hide_scenes as S

pytestmark = pytest.mark.gpu

PWN_EINVAL = -1
KS = (-1, 0, 1, 5, 13)
NMAX = 4097


@functools.lru_cache(maxsize=None)
def _pool():
    """4097 rays, the hand-made ones first (so that n = 1 and n = 63 hold some), and each ray's hidden sphere"""
    import pwnfps_amd
    s = S.spheres_t0()
    c0 = np.array([s["x"][0], s["y"][0], s["z"][0]], np.float32)
    hand = np.zeros((8, 8), np.float32)
    hand[:, 3] = 1.0
    for j, (off, d) in enumerate((((0.1, 0.05, 0.0), (-1, 0, 0)), ((0.1, 0.05, 0.0), (1, 0, 0)), ((0.0, 0.0, 0.0), (0, 0, 1)), ((-0.2, 0.1, 0.1), (1, -0.5, -0.5)),
                                  ((0.0, 0.25, 0.0), (0, -1, 0)), ((0.05, 0.0, -0.25), (0, 0.2, 1)), ((0.29, 0.0, 0.0), (-1, 0.1, 0)), ((0.0, -0.1, 0.0), (0.3, 1, 0.3)))):
        hand[j, 0:3] = c0 + np.array(off, np.float32)
        hand[j, 4:7] = d
    px = np.concatenate([pwnfps_amd.pixel_rays(S.W, S.H, cam)[0] for cam in S.cameras()])
    rng = np.random.default_rng(20261020)
    px = px[rng.permutation(len(px))]
    rays = np.concatenate([hand, px, px])[:NMAX]
    assert rays.shape == (NMAX, 8)
    hide = rng.choice(np.array(KS, np.int32), NMAX).astype(np.int32)
    hide[:8] = (0, 0, 0, 0, -1, 1, 0, 13)
    return np.ascontiguousarray(rays), hide


def _hits(r, rays, hide=None):
    """trace_hits_device (hide given: pwn_trace_hits_hide_device) on a non-default stream -> (n, 48) bytes"""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_rays = torch.from_numpy(rays.copy()).to(dev)
        t_hits = torch.full((len(rays), 12), S.POISON, dtype=torch.int32, device=dev)
        t_hide = torch.from_numpy(np.ascontiguousarray(hide, np.int32).copy()).to(dev) if hide is not None else None
        r.trace_hits_device(t_rays, t_hits, hide=t_hide)
        out = t_hits.cpu().numpy()
    s.synchronize()
    return out.view(np.uint8).reshape(len(rays), 48)


@functools.lru_cache(maxsize=None)
def _reference(k):
    """pwn_trace_hits_device of the whole pool on the table without entry k, `object` in the full table's numbering -> (4097, 48) bytes"""
    import pwnfps_amd
    rays, _ = _pool()
    with S.renderer(None, S.without(S.spheres_t0(), k)) as r:
        rec = _hits(r, rays).copy().view(pwnfps_amd.HIT_DTYPE).reshape(len(rays))
    rec["object"] = S.full_numbers(rec["object"], k)
    return rec.view(np.uint8).reshape(len(rays), 48)


def _expected(n):
    rays, hide = _pool()
    want = np.zeros((n, 48), np.uint8)
    for k in KS:
        m = hide[:n] == k
        want[m] = _reference(k)[:n][m]
    return want


def test_hiding_changes_the_records():
    """teeth, on the references: hundreds of the pool's rays end on something else once their sphere is gone, and some references
    name an object above the hidden one"""
    import pwnfps_amd
    rays, hide = _pool()
    full, want = _reference(-1), _expected(NMAX)
    assert int((full != want).any(axis=1).sum()) >= 100
    assert (full[[0, 3]] != want[[0, 3]]).any(axis=1).all()          # hand-made rays inside sphere 0, its centre in front of them, that hide it
    obj = want.copy().view(pwnfps_amd.HIT_DTYPE).reshape(NMAX)["object"]
    assert ((obj > hide) & (hide >= 0)).any()


@pytest.mark.parametrize("n,force_hasw", [(1, False), (63, False), (65, False), (65, True), (4097, False)])
@pytest.mark.parametrize("form", S.FORMS)
def test_records_equal_the_reduced_tables(form, n, force_hasw):
    rays, hide = _pool()
    want = _expected(n)
    with S.renderer(form, S.spheres_t0(), force_hasw=force_hasw) as r:
        got = _hits(r, rays[:n], hide[:n])
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (form, n, bad[:8], hide[bad[:8]])
        # values that hide nothing: the un-hidden call's records
        none = _hits(r, rays[:n], np.resize(np.array([-1, -7, 14, 10000, 2 ** 31 - 1], np.int32), n))
        assert (none == _hits(r, rays[:n])).all()


def test_counters_are_the_reduced_tables():
    rays, hide = _pool()
    n = 65
    want = [0, 0, 0, 0]
    for k in KS:
        m = hide[:n] == k
        if m.any():
            with S.renderer(None, S.without(S.spheres_t0(), k), counters=True) as r:
                _hits(r, rays[:n][m])
                want = [a + b for a, b in zip(want, S.stats4(r.stats()))]
    with S.renderer(None, S.spheres_t0(), counters=True) as r:
        _hits(r, rays[:n], hide[:n])
        assert list(S.stats4(r.stats())) == want


def test_a_bad_hide_array_is_refused_and_nothing_is_written():
    import torch
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    rays, _ = _pool()
    n = 65
    with S.renderer(None, S.spheres_t0()) as r:
        t_rays = torch.from_numpy(rays[:n].copy()).to(dev)
        t_hits = torch.full((n, 12), S.POISON, dtype=torch.int32, device=dev)
        t_hide = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        hits = t_hits.data_ptr()
        for hide in (None, t_hide.data_ptr() + 2, hits, hits + 48 * n - 4, hits - 4 * n + 4):
            rc = _lib.lib.pwn_trace_hits_hide_device(r._ctx, n, C.c_void_p(t_rays.data_ptr()), C.c_void_p(hide), 0, C.c_void_p(hits), None)
            assert rc == PWN_EINVAL, hide
        torch.cuda.synchronize()
        assert bool((t_hits == S.POISON).all())
        # an empty batch needs no array
        assert _lib.lib.pwn_trace_hits_hide_device(r._ctx, 0, None, None, 0, None, None) == 0
