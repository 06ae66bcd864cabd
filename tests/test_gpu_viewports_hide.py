"""pwn_trace_viewports_hide_device and pwn_trace_viewport_hits_hide_device: rectangle i does not see sphere hide[i].  Rectangle i is
bit-identical -- colour and depth, label, cell and dist -- to rectangle i of the call without `_hide` on a context whose table is the
same spheres with entry hide[i] taken out, object numbers still those of the full table; for every form of the sphere tables, with
blur off and on, through the 3-lane and the 4-lane kernels; nothing outside the rectangles is written; the counters of the contract
are the references' sums.  The layout, the cameras, the calls and the references: tests/hide_vp_scenes.py.

Teeth (the CPU oracle, tests/oracle.py, at the rectangles' sizes, blur off, with and without the hidden sphere): rectangle 0 (camera
0 inside sphere 0, 40 x 26) differs in 530 of 1040 pixels, rectangle 1 (camera 1 inside sphere 1, 56 x 16) in 886 of 896, rectangle
2 (camera 2 next to sphere 5, 96 x 12) in 521 of 1152 -- against thresholds of 100, a tenth of 896 and a tenth of 1152."""
import ctypes as C

import numpy as np
import pytest

import hide_scenes as S
import hide_vp_scenes as V

pytestmark = pytest.mark.gpu

PWN_EINVAL = -1
TEETH = (100, -(-56 * 16 // 10), -(-96 * 12 // 10))


def _outside_untouched(plane, poison):
    return bool((plane[~V.inside_mask()] == np.uint32(poison)).all())


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
@pytest.mark.parametrize("form", S.FORMS)
def test_rectangles_equal_the_reduced_tables(form, force_hasw):
    cams = V.cameras()
    with V.context(form, S.spheres_t0(), force_hasw=force_hasw) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        for hide in V.HIDES:
            for blur in (0, 1):
                r.set_blur_passes(blur)
                sb, z = V.viewports_call(r, lay, cams, V.SECS, hide=hide, blur=blur)
                for i, k in enumerate(hide):
                    ref = V.reference(k)
                    bad = int((V.rect(sb, i) != V.rect(ref[(blur, "col")], i)).sum())
                    assert bad == 0, (form, hide, blur, i, bad)
                    assert (V.rect(z, i) == V.rect(ref[(blur, "z")], i)).all(), (form, hide, blur, i)
                # every word outside the rectangles: the colour's poison, the depth's zero
                assert _outside_untouched(sb, 0xffffffff) and _outside_untouched(z, 0), (form, hide, blur)
            r.set_blur_passes(0)
            # first-hit planes, with cell and dist left out in the four combinations
            for cell, dist in ((True, True), (True, False), (False, True), (False, False)):
                got = V.viewport_hits_call(r, lay, cams, hide=hide, cell=cell, dist=dist)
                for name, plane in zip(("label", "cell", "dist"), got):
                    if plane is None:
                        continue
                    for i, k in enumerate(hide):
                        assert (V.rect(plane, i) == V.rect(V.reference(k)[name], i)).all(), (form, hide, name, i)
                    assert _outside_untouched(plane, 0xffffffff), (form, hide, name)
            # rays, steps, portals, exhausted: the sums of the references', each rectangle traced alone on its reduced table
            r.set_counters(True)
            V.viewports_call(r, lay, cams, V.SECS, hide=hide)
            got = S.stats4(r.stats())
            want = tuple(sum(V.reference(k)[("stats", i)][j] for i, k in enumerate(hide)) for j in range(4))
            assert got == want, (form, hide)
            V.viewport_hits_call(r, lay, cams, hide=hide)
            got = S.stats4(r.stats())
            want = tuple(sum(V.reference(k)[("hstats", i)][j] for i, k in enumerate(hide)) for j in range(4))
            assert got == want, (form, hide, "hits")
            r.set_counters(False)
        lay.free()


def test_rectangle_0_is_the_views_call_without_the_sphere():
    """across the families: rectangle 0 (40 x 26) equals view 0 of pwn_trace_views_device on a 40 x 26 context without sphere 0"""
    with V.context(None, S.spheres_t0()) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        for blur in (0, 1):
            r.set_blur_passes(blur)
            sb, z = V.viewports_call(r, lay, V.cameras(), V.SECS, hide=V.HIDES[0], blur=blur)
            ref = S.reference_views(0)
            assert (V.rect(sb, 0) == ref[(blur, "col")][0]).all(), blur
            assert (V.rect(z, 0) == ref[(blur, "z")][0]).all(), blur
        lay.free()


def test_hiding_changes_the_rectangles():
    """teeth, on the call itself: rectangles 0, 1 and 2 hidden against the same rectangles of the plain call; rectangle 3, with
    PWN_HIDE_NONE, equals the plain call's"""
    cams = V.cameras()
    with V.context(None, S.spheres_t0()) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        sb, z = V.viewports_call(r, lay, cams, V.SECS, hide=V.HIDES[0])
        plain, plain_z = V.viewports_call(r, lay, cams, V.SECS)
        lb, _, _ = V.viewport_hits_call(r, lay, cams, hide=V.HIDES[0])
        plain_lb, _, _ = V.viewport_hits_call(r, lay, cams)
        lay.free()
    differ = [int((V.rect(sb, i) != V.rect(plain, i)).sum()) for i in range(4)]
    differ_lb = [int((V.rect(lb, i) != V.rect(plain_lb, i)).sum()) for i in range(4)]
    print("pixels that hiding changes, colour:", differ, "labels:", differ_lb)
    for i in range(3):
        assert differ[i] >= TEETH[i], (i, differ)
    assert differ[3] == 0 and differ_lb[3] == 0 and (V.rect(z, 3) == V.rect(plain_z, 3)).all()
    assert differ_lb[0] > 0 and differ_lb[1] > 0


@pytest.mark.parametrize("form", S.FORMS)
def test_identity_is_the_number_not_the_value(form):
    """a 15th sphere equal to sphere 0 in r, x, y, z with another colour: hiding 0 leaves the clone visible and equals the table
    without entry 0; hiding 14 equals the original 14 spheres"""
    cams, s14 = V.cameras(), S.spheres_t0()
    s15 = np.concatenate([s14, s14[:1]])
    s15["cb"][14], s15["cg"][14], s15["cr"][14] = 0.1, 0.9, 0.2
    with V.context(None, S.without(s15, 0)) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        want0, want0_z = V.viewports_call(r, lay, cams, V.SECS)
        want0_lb = V.relabel(V.viewport_hits_call(r, lay, cams)[0], 0)
        lay.free()
    orig = V.reference(S.HIDE_NONE)
    with V.context(form, s15) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        sb0, z0 = V.viewports_call(r, lay, cams, V.SECS, hide=[0] * 4)
        sb14, z14 = V.viewports_call(r, lay, cams, V.SECS, hide=[14] * 4)
        lb0 = V.viewport_hits_call(r, lay, cams, hide=[0] * 4)[0]
        lb14 = V.viewport_hits_call(r, lay, cams, hide=[14] * 4)[0]
        lay.free()
    m = V.inside_mask()
    assert (sb0[m] == want0[m]).all() and (z0[m] == want0_z[m]).all() and (lb0[m] == want0_lb[m]).all()
    assert (sb14[m] == orig[(0, "col")][m]).all() and (z14[m] == orig[(0, "z")][m]).all() and (lb14[m] == orig["label"][m]).all()
    assert int((V.rect(sb0, 0) != V.rect(sb14, 0)).sum()) >= 100            # the other colour shows
    # (the clone reports as object 14 where sphere 0 reported as 0)
    import pwnfps_amd
    obj0, obj14 = pwnfps_amd.unpack_labels(V.rect(lb0, 0))[2], pwnfps_amd.unpack_labels(V.rect(lb14, 0))[2]
    assert (obj0 == 14).any() and not (obj0 == 0).any() and (obj14 == 0).any() and not (obj14 == 14).any()


@pytest.mark.parametrize("form", S.FORMS)
def test_values_that_hide_nothing(form):
    """-1, -7, the live count, 10000 and INT_MAX in every entry: the planes and all five counters of the plain calls"""
    cams = V.cameras()
    with V.context(form, S.spheres_t0(), counters=True) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        want = V.viewports_call(r, lay, cams, V.SECS)
        want_st = S.stats5(r.stats())
        want_h = V.viewport_hits_call(r, lay, cams)
        want_hst = S.stats5(r.stats())
        for v in (-1, -7, 14, 10000, 2 ** 31 - 1):
            got = V.viewports_call(r, lay, cams, V.SECS, hide=[v] * 4)
            assert all((g == w).all() for g, w in zip(got, want)), v
            assert S.stats5(r.stats()) == want_st, v
            got = V.viewport_hits_call(r, lay, cams, hide=[v] * 4)
            assert all((g == w).all() for g, w in zip(got, want_h)), v
            assert S.stats5(r.stats()) == want_hst, v
        r.set_counters(False)
        r.set_blur_passes(1)
        want = V.viewports_call(r, lay, cams, V.SECS, blur=1)
        got = V.viewports_call(r, lay, cams, V.SECS, hide=[S.HIDE_NONE, -2 ** 31, 14, 4096], blur=1)
        assert all((g == w).all() for g, w in zip(got, want))
        lay.free()


def test_ten_calls_without_a_wait_between_them():
    """rotation: hide and plain calls of the same layout alternate, colour and hits calls interleaved, nothing waited for in between,
    on one stream and on two; every call's planes are those of the same call made alone -- a hide word that stayed in a record set, or
    one that a set did not get, shows as a rectangle of the wrong table.  The hide calls take the two arrays of V.HIDES in turn, which
    name a sphere where the other says PWN_HIDE_NONE: calls k and k + 4 share a record set, and sets see A then B, and plain then A"""
    import torch
    dev = torch.device("cuda", 0)
    cams = V.cameras()
    with V.context(None, S.spheres_t0()) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        alone = {}
        for hid, hide in ((None, None), ("A", V.HIDES[0]), ("B", V.HIDES[1])):
            alone[("col", hid)] = V.viewports_call(r, lay, cams, V.SECS, hide=hide)[0]
            alone[("hits", hid)] = V.viewport_hits_call(r, lay, cams, hide=hide)[0]
        m = V.inside_mask()
        for kind in ("col", "hits"):
            assert not (alone[(kind, "A")][m] == alone[(kind, None)][m]).all() and not (alone[(kind, "A")][m] == alone[(kind, "B")][m]).all(), kind
        t_cams = torch.from_numpy(cams.reshape(4, 16).copy()).to(dev)
        t_secs = torch.from_numpy(V.SECS.copy()).to(dev)
        t_hides = {None: None, "A": torch.tensor(V.HIDES[0], dtype=torch.int32, device=dev), "B": torch.tensor(V.HIDES[1], dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        for streams in ([torch.cuda.Stream(dev)], [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]):
            # (colour, colour, hits, hits, ... against A, plain, B, plain, B, A, plain, A, plain, B: hide and plain calls of both kinds on
            # either stream, and in every record set a hide call behind another array's or behind a plain call)
            plan = [("hits" if (k // 2) & 1 else "col", hid) for k, hid in enumerate(("A", None, "B", None, "B", "A", None, "A", None, "B"))]
            outs = []
            for k, (kind, hid) in enumerate(plan):
                s = streams[k % len(streams)]
                with torch.cuda.stream(s):
                    out = torch.full((V.FH, V.FW), V.POISON, dtype=torch.int32, device=dev)
                    if kind == "col":
                        z = torch.zeros((V.FH, V.FW), dtype=torch.float32, device=dev)
                        r.trace_viewports_device(lay, t_cams, t_secs, out, z, hide=t_hides[hid])
                    else:
                        r.trace_viewport_hits_device(lay, t_cams, out, hide=t_hides[hid])
                    outs.append(out)
            torch.cuda.synchronize()
            for k, (kind, hid) in enumerate(plan):
                got = outs[k].cpu().numpy().view(np.uint32)
                assert (got[m] == alone[(kind, hid)][m]).all(), (len(streams), k, kind, hid)
        lay.free()


def test_a_bad_hide_array_is_refused_and_nothing_is_written():
    import torch
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    L = _lib.lib
    with V.context(None, S.spheres_t0(), blur=1) as r:
        lay = r.viewports_layout(V.FW, V.FH, V.RECTS)
        odd = r.viewports_layout(V.FW, V.FH, [(1, 0, 37, 21)])
        t_cams = torch.from_numpy(V.cameras().reshape(4, 16).copy()).to(dev)
        t_secs = torch.from_numpy(V.SECS.copy()).to(dev)
        planes = [torch.full((V.FH, V.FW), V.POISON, dtype=torch.int32, device=dev) for _ in range(3)]
        t_hide = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        a, b, d = (p.data_ptr() for p in planes)
        last = V.FH * V.FW * 4 - 4
        cp, sp = C.c_void_p(t_cams.data_ptr()), C.c_void_p(t_secs.data_ptr())
        for hide in (None, t_hide.data_ptr() + 2, a, b + last, d + 8, a + last - 4, b - 12):
            rc = L.pwn_trace_viewports_hide_device(r._ctx, lay._ptr, cp, sp, C.c_void_p(hide), 0, C.c_void_p(a), C.c_void_p(b), C.c_void_p(d), None)
            assert rc == PWN_EINVAL, ("viewports", hide)
            rc = L.pwn_trace_viewport_hits_hide_device(r._ctx, lay._ptr, cp, C.c_void_p(hide), 0, C.c_void_p(a), C.c_void_p(b), C.c_void_p(d), None)
            assert rc == PWN_EINVAL, ("viewport hits", hide)
        # a blur call on a layout not usable with blur: refused as its sibling is
        h = C.c_void_p(t_hide.data_ptr())
        assert L.pwn_trace_viewports_device(r._ctx, odd._ptr, cp, sp, 0, C.c_void_p(a), C.c_void_p(b), C.c_void_p(d), None) == PWN_EINVAL
        assert L.pwn_trace_viewports_hide_device(r._ctx, odd._ptr, cp, sp, h, 0, C.c_void_p(a), C.c_void_p(b), C.c_void_p(d), None) == PWN_EINVAL
        torch.cuda.synchronize()
        for p in planes:
            assert bool((p == V.POISON).all())
        # (the same array, well placed, is taken)
        assert L.pwn_trace_viewports_hide_device(r._ctx, lay._ptr, cp, sp, h, 0, C.c_void_p(a), C.c_void_p(b), C.c_void_p(d), None) == 0
        torch.cuda.synchronize()
        assert not bool((planes[1] == V.POISON).all())
        odd.free()
        lay.free()
