"""pwn_trace_views_hide_device: view i does not see sphere hide[i].  View i is bit-identical, colour and depth, to view i of
pwn_trace_views_device on a context whose table is the same spheres with entry hide[i] taken out -- for every form of the sphere
tables, with blur off and on, through the 3-lane and the 4-lane kernels; the counters of the contract are the references' sums.
The scene, the cameras and the references: tests/hide_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hide_scenes as S

pytestmark = pytest.mark.gpu

PWN_EINVAL = -1
HIDES = ([0, 1, 5], [0, S.HIDE_NONE, 13])


def test_hiding_changes_the_picture():
    """teeth: the camera inside sphere 0 sees another picture without it (the CPU oracle: 530 of 1040 pixels) -- judged on the
    REFERENCES, so it says that the scene can tell a hidden sphere from a visible one; the tests below hold the hide call to them"""
    full, gone = S.reference_views(S.HIDE_NONE)[(0, "col")][0], S.reference_views(0)[(0, "col")][0]
    assert int((full != gone).sum()) >= 100


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
@pytest.mark.parametrize("form", S.FORMS)
def test_views_equal_the_reduced_tables(form, force_hasw):
    cams, spheres = S.cameras(), S.spheres_t0()
    with S.renderer(form, spheres, force_hasw=force_hasw) as r:
        for hide in HIDES:
            for blur in (0, 1):
                r.set_blur_passes(blur)
                sb, z = S.views_call(r, cams, S.SECS, hide=hide, blur=blur)
                for i, k in enumerate(hide):
                    ref = S.reference_views(k)
                    bad = int((sb[i] != ref[(blur, "col")][i]).sum())
                    assert bad == 0, (form, hide, blur, i, bad)
                    assert (z[i] == ref[(blur, "z")][i]).all(), (form, hide, blur, i)
            # teeth, on the call itself: view 0 hidden against the same view of the un-hidden call
            if hide[0] == 0:
                r.set_blur_passes(0)
                sb, _ = S.views_call(r, cams, S.SECS, hide=hide)
                plain, _ = S.views_call(r, cams, S.SECS)
                assert int((sb[0] != plain[0]).sum()) >= 100
            # rays, steps, portals, exhausted: the sum of the references'
            r.set_blur_passes(0)
            r.set_counters(True)
            S.views_call(r, cams, S.SECS, hide=hide)
            got = S.stats4(r.stats())
            r.set_counters(False)
            want = tuple(sum(S.reference_views(k)[("stats", i)][j] for i, k in enumerate(hide)) for j in range(4))
            assert got == want, (form, hide)


@pytest.mark.parametrize("form", S.FORMS)
def test_identity_is_the_number_not_the_value(form):
    """a 15th sphere equal to sphere 0 in r, x, y, z with another colour: hiding 0 shows the other colour and equals the table
    without entry 0; hiding 14 equals the original 14"""
    cams, s14 = S.cameras(), S.spheres_t0()
    s15 = np.concatenate([s14, s14[:1]])
    s15["cb"][14], s15["cg"][14], s15["cr"][14] = 0.1, 0.9, 0.2
    with S.renderer(None, S.without(s15, 0)) as r:
        want0, want0_z = S.views_call(r, cams, S.SECS)
    orig = S.reference_views(S.HIDE_NONE)
    with S.renderer(form, s15) as r:
        sb0, z0 = S.views_call(r, cams, S.SECS, hide=[0, 0, 0])
        sb14, z14 = S.views_call(r, cams, S.SECS, hide=[14, 14, 14])
    assert (sb0 == want0).all() and (z0 == want0_z).all()
    assert (sb14 == orig[(0, "col")]).all() and (z14 == orig[(0, "z")]).all()
    assert int((sb0[0] != sb14[0]).sum()) >= 100            # the other colour shows


@pytest.mark.parametrize("form", S.FORMS)
def test_values_that_hide_nothing(form):
    """-1, -7, the live count, 10000 and INT_MAX: planes and all five counters as pwn_trace_views_device gives them"""
    cams, spheres = S.cameras(), S.spheres_t0()
    with S.renderer(form, spheres, counters=True) as r:
        want, want_z = S.views_call(r, cams, S.SECS)
        want_st = S.stats5(r.stats())
        for v in (-1, -7, 14, 10000, 2 ** 31 - 1):
            sb, z = S.views_call(r, cams, S.SECS, hide=[v] * 3)
            assert (sb == want).all() and (z == want_z).all(), v
            assert S.stats5(r.stats()) == want_st, v
        r.set_counters(False)
        r.set_blur_passes(1)
        want, want_z = S.views_call(r, cams, S.SECS, blur=1)
        sb, z = S.views_call(r, cams, S.SECS, hide=[S.HIDE_NONE, -2 ** 31, 14], blur=1)
        assert (sb == want).all() and (z == want_z).all()


def test_a_bad_hide_array_is_refused_and_nothing_is_written():
    import torch
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    with S.renderer(None, S.spheres_t0(), blur=1) as r:
        n = 3
        t_cams = torch.from_numpy(S.cameras().reshape(n, 16).copy()).to(dev)
        t_secs = torch.from_numpy(S.SECS.copy()).to(dev)
        planes = [torch.full((n, S.H, S.W), S.POISON, dtype=torch.int32, device=dev) for _ in range(3)]
        t_hide = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        work, sb, z = (p.data_ptr() for p in planes)
        last = n * S.H * S.W * 4 - 4
        for hide in (None, t_hide.data_ptr() + 2, sb, sb + last, z + 8, work + last - 4, sb - 8):
            rc = _lib.lib.pwn_trace_views_hide_device(r._ctx, n, C.c_void_p(t_cams.data_ptr()), C.c_void_p(t_secs.data_ptr()), C.c_void_p(hide), 0,
                                                      C.c_void_p(work), C.c_void_p(sb), C.c_void_p(z), None)
            assert rc == PWN_EINVAL, hide
        torch.cuda.synchronize()
        for p in planes:
            assert bool((p == S.POISON).all())
        # (the same array, well placed, is taken)
        rc = _lib.lib.pwn_trace_views_hide_device(r._ctx, n, C.c_void_p(t_cams.data_ptr()), C.c_void_p(t_secs.data_ptr()), C.c_void_p(t_hide.data_ptr()), 0,
                                                  C.c_void_p(work), C.c_void_p(sb), C.c_void_p(z), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert not bool((planes[1] == S.POISON).all())
