"""pwn_trace_rays_hide_device: ray i does not see sphere hide[i], on any of its segments.  Colour and depth of ray i are bit-identical
to ray i of pwn_trace_rays_device on a context whose table is the same spheres with entry hide[i] taken out -- one reference per hide
value -- for batches of 1, 63, 65 and 4097 rays (one lane, a unit but one, a unit and one, more than one workgroup's units and an odd
tail), every form of the sphere tables, the 3-lane and the 4-lane kernels.  The rays are the pixel rays and seeds of the three cameras
plus hand-made rays that start inside sphere 0; per-ray hide from {-1, 0, 1, 5, 13}; sec_current 1.25; depth in / out from 3.5.
The pool, the calls and the references: tests/hide_vp_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hide_scenes as S
import hide_vp_scenes as V

pytestmark = pytest.mark.gpu

PWN_EINVAL = -1
SIZES = (1, 63, 65, 4097)


def _want(hide, n):
    col, z = np.empty(n, np.uint32), np.empty(n, np.uint32)
    for v in V.RAY_HIDES:
        rc, rz = V.ray_reference(v)
        m = hide[:n] == v
        col[m], z[m] = rc[:n][m], rz[:n][m]
    return col, z


def test_hiding_changes_the_rays():
    """teeth, on the references: of the rays that hide sphere 0, 1 or 5, at least a tenth come out differently without it (the pixel
    rays of a camera see its sphere in about half of the pixels; every hand-made ray starts inside sphere 0) -- and the first ray, all
    that a batch of one traces, is one of them"""
    _, _, hide = V.ray_pool()
    full = V.ray_reference(S.HIDE_NONE)[0]
    want = _want(hide, V.RAY_POOL)[0]
    hiding = np.isin(hide, (0, 1, 5))
    differ = int((want[hiding] != full[hiding]).sum())
    print("rays that hiding changes:", differ, "of", int(hiding.sum()))
    assert differ * 10 >= int(hiding.sum())
    assert hide[0] == 0 and want[0] != full[0]


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
@pytest.mark.parametrize("form", S.FORMS)
def test_rays_equal_the_reduced_tables(form, force_hasw):
    rays, seeds, hide = V.ray_pool()
    with V.context(form, S.spheres_t0(), force_hasw=force_hasw) as r:
        for n in SIZES:
            col, z = V.rays_call(r, rays[:n], seeds[:n], hide=hide[:n])
            want, want_z = _want(hide, n)
            bad = int((col != want).sum())
            assert bad == 0, (form, n, bad)
            assert (z == want_z).all(), (form, n)


@pytest.mark.parametrize("form", S.FORMS)
def test_values_that_hide_nothing_and_the_counters(form):
    rays, seeds, hide = V.ray_pool()
    n = 4097
    with V.context(form, S.spheres_t0(), counters=True) as r:
        want = V.rays_call(r, rays, seeds)
        want_st = S.stats5(r.stats())
        for v in (-1, -7, 14, 10000, 2 ** 31 - 1):
            got = V.rays_call(r, rays, seeds, hide=np.full(n, v, np.int64).astype(np.int32))
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), v
            assert S.stats5(r.stats()) == want_st, v
        # rays, steps, portals, exhausted of a hide call: the sum over the groups, each group traced on its reduced table
        V.rays_call(r, rays, seeds, hide=hide)
        got_st = S.stats4(r.stats())
    total = [0, 0, 0, 0]
    for v in V.RAY_HIDES:
        m = hide == v
        with V.context(None, S.without(S.spheres_t0(), v), counters=True) as ref:
            V.rays_call(ref, rays[m], seeds[m])
            total = [a + b for a, b in zip(total, S.stats4(ref.stats()))]
    assert got_st == tuple(total), form


def test_hits_and_colour_calls_interleaved_without_a_wait():
    """rotation: ten calls, colour rays with and without hide and first hits with and without hide in turn, on one stream and on two,
    nothing waited for in between; each call's output equals that of the same call made alone"""
    import torch
    dev = torch.device("cuda", 0)
    rays, seeds, hide = V.ray_pool()
    n = 4097
    with V.context(None, S.spheres_t0()) as r:
        t_rays = torch.from_numpy(rays).to(dev)
        t_seeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
        t_hide = torch.from_numpy(hide.copy()).to(dev)

        def call(kind, hid):
            if kind == "col":
                out = torch.full((n,), V.POISON, dtype=torch.int32, device=dev)
                z = torch.full((n,), V.RAY_DEPTH0, dtype=torch.float32, device=dev)
                r.trace_rays_device(t_rays, out, z, seeds=t_seeds, sec_current=V.RAY_SEC, hide=t_hide if hid else None)
            else:
                out = torch.full((n, 12), V.POISON, dtype=torch.int32, device=dev)
                r.trace_hits_device(t_rays, out, hide=t_hide if hid else None)
            return out

        alone = {}
        for kind in ("col", "hits"):
            for hid in (True, False):
                alone[(kind, hid)] = call(kind, hid).cpu().numpy()
        assert not (alone[("col", True)] == alone[("col", False)]).all() and not (alone[("hits", True)] == alone[("hits", False)]).all()
        torch.cuda.synchronize()
        for streams in ([torch.cuda.Stream(dev)], [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]):
            plan = [("hits" if (k // 2) & 1 else "col", k % 2 == 0 if k < 5 else k % 2 == 1) for k in range(10)]
            outs = []
            for k, (kind, hid) in enumerate(plan):
                with torch.cuda.stream(streams[k % len(streams)]):
                    outs.append(call(kind, hid))
            torch.cuda.synchronize()
            for k, (kind, hid) in enumerate(plan):
                assert (outs[k].cpu().numpy() == alone[(kind, hid)]).all(), (len(streams), k, kind, hid)


def test_a_bad_hide_array_is_refused_and_nothing_is_written():
    import torch
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    L = _lib.lib
    rays, seeds, _ = V.ray_pool()
    n = 65
    with V.context(None, S.spheres_t0()) as r:
        t_rays = torch.from_numpy(rays[:n]).to(dev)
        t_col = torch.full((n,), V.POISON, dtype=torch.int32, device=dev)
        t_z = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
        t_hide = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        col, z = t_col.data_ptr(), t_z.data_ptr()
        last = n * 4 - 4
        for hide in (None, t_hide.data_ptr() + 2, col, col + last, z + 8, z - 4 * n + 4):
            rc = L.pwn_trace_rays_hide_device(r._ctx, n, C.c_void_p(t_rays.data_ptr()), None, C.c_void_p(hide), C.c_float(0.0), 0,
                                              C.c_void_p(col), C.c_void_p(z), None)
            assert rc == PWN_EINVAL, hide
        torch.cuda.synchronize()
        assert bool((t_col == V.POISON).all()) and bool((t_z == -1.0).all())
        # the empty batch needs no array; the same array, well placed, is taken
        assert L.pwn_trace_rays_hide_device(r._ctx, 0, None, None, None, C.c_float(0.0), 0, None, None, None) == 0
        rc = L.pwn_trace_rays_hide_device(r._ctx, n, C.c_void_p(t_rays.data_ptr()), None, C.c_void_p(t_hide.data_ptr()), C.c_float(0.0), 0,
                                          C.c_void_p(col), C.c_void_p(z), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert not bool((t_col == V.POISON).any())
