"""pwn_trace_view_hits_hide_device: the first-hit planes of views that do not see one sphere each.  Label, cell and dist of view i are
bit-identical to pwn_trace_view_hits_device's on a context whose table lacks entry hide[i], with the label's object field in the FULL
table's numbering (j -> j + (j >= hide[i])).  Scene, cameras and references: tests/hide_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hide_scenes as S

pytestmark = pytest.mark.gpu

PWN_EINVAL = -1
HIDES = ([0, 1, 5], [0, S.HIDE_NONE, 13])


def test_hiding_changes_the_labels():
    """teeth, on the references: under the camera inside sphere 0 at least 100 pixels have another label without it, and some
    reference labels name an object above the hidden one (the renumbering has something to do)"""
    import pwnfps_amd
    full, gone = S.reference_view_hits(S.HIDE_NONE)[0][0], S.reference_view_hits(0)[0][0]
    assert int((full != gone).sum()) >= 100
    assert (pwnfps_amd.unpack_labels(S.reference_view_hits(1)[0])[2] > 1).any()


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
@pytest.mark.parametrize("form", S.FORMS)
def test_planes_equal_the_reduced_tables(form, force_hasw):
    cams = S.cameras()
    with S.renderer(form, S.spheres_t0(), force_hasw=force_hasw) as r:
        for hide in HIDES:
            label, cell, dist = S.view_hits_call(r, cams, hide=hide)
            for i, k in enumerate(hide):
                want = S.reference_view_hits(k)
                for name, got, ref in (("label", label, want[0]), ("cell", cell, want[1]), ("dist", dist, want[2])):
                    bad = int((got[i] != ref[i]).sum())
                    assert bad == 0, (form, hide, i, name, bad)
        # the label plane alone: cell and dist may be NULL
        label, cell, dist = S.view_hits_call(r, cams, hide=HIDES[0], cell=False, dist=False)
        assert cell is None and dist is None
        for i, k in enumerate(HIDES[0]):
            assert (label[i] == S.reference_view_hits(k)[0][i]).all(), (form, i)
        # values that hide nothing: the un-hidden call's planes
        want = S.view_hits_call(r, cams)
        got = S.view_hits_call(r, cams, hide=[-7, 14, 2 ** 31 - 1])
        for a, b in zip(got, want):
            assert (a == b).all()


def test_counters_are_the_reduced_tables():
    """rays, steps, portals, exhausted of the primary segments: the sum over the views of the reduced tables' own"""
    cams = S.cameras()
    hide = HIDES[0]
    want = [0, 0, 0, 0]
    for i, k in enumerate(hide):
        with S.renderer(None, S.without(S.spheres_t0(), k), counters=True) as r:
            S.view_hits_call(r, cams[i:i + 1])
            want = [a + b for a, b in zip(want, S.stats4(r.stats()))]
    with S.renderer("inline", S.spheres_t0(), counters=True) as r:
        S.view_hits_call(r, cams, hide=hide)
        assert list(S.stats4(r.stats())) == want


def test_a_bad_hide_array_is_refused_and_nothing_is_written():
    import torch
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    with S.renderer(None, S.spheres_t0()) as r:
        n = 3
        t_cams = torch.from_numpy(S.cameras().reshape(n, 16).copy()).to(dev)
        planes = [torch.full((n, S.H, S.W), S.POISON, dtype=torch.int32, device=dev) for _ in range(3)]
        t_hide = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        label, cell, dist = (p.data_ptr() for p in planes)
        last = n * S.H * S.W * 4 - 4
        for hide in (None, t_hide.data_ptr() + 1, label, cell + last, dist + 16):
            rc = _lib.lib.pwn_trace_view_hits_hide_device(r._ctx, n, C.c_void_p(t_cams.data_ptr()), C.c_void_p(hide), 0,
                                                          C.c_void_p(label), C.c_void_p(cell), C.c_void_p(dist), None)
            assert rc == PWN_EINVAL, hide
        torch.cuda.synchronize()
        for p in planes:
            assert bool((p == S.POISON).all())
