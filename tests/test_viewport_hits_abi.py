"""pwn_trace_viewport_hits and pwn_trace_viewport_hits_device without a GPU: the exports, the bindings and the header's prototypes,
the new kernel mode's twelve variants in the built library, Renderer's argument checks with the library replaced by an object that
fails on any call, and the C entries' refusals that need no context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = {"pwn_trace_viewport_hits": 7, "pwn_trace_viewport_hits_device": 8}


def _lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    from pwnfps_amd import _lib as binding
    return binding.lib


def test_entries_are_exported_bound_and_declared():
    _lib()
    raw = C.CDLL(LIB)
    from pwnfps_amd import _lib as binding
    import pwnfps_amd
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    for entry, nargs in ENTRIES.items():
        assert hasattr(raw, entry), entry
        bound = [a for n, _, a in binding.ABI if n == entry]
        assert len(bound) == 1 and len(bound[0]) == nargs, entry
        decl = re.search(r"^int %s\(([^;]*)\);" % entry, hdr, re.M)
        assert decl and len(decl.group(1).split(",")) == nargs, entry
    assert re.search(r"^int pwn_trace_viewport_hits\(pwn_ctx \*ctx, int n, const pwn_viewport \*vp, const float \*cams,\n"
                     r"\tuint32_t \*label, uint32_t \*cell, float \*dist\);", hdr, re.M)
    assert re.search(r"^int pwn_trace_viewport_hits_device\(pwn_ctx \*ctx, const pwn_vp_layout \*layout, const void \*d_cams, int flags,\n"
                     r"\tvoid \*d_label, void \*d_cell, void \*d_dist, void \*stream\);", hdr, re.M)
    assert callable(pwnfps_amd.Renderer.trace_viewport_hits) and callable(pwnfps_amd.Renderer.trace_viewport_hits_device)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "pwnhip.h"\n'
                   'int main(void) {\n'
                   '\tint (*hf)(pwn_ctx *, int, const pwn_viewport *, const float *, uint32_t *, uint32_t *, float *) = pwn_trace_viewport_hits;\n'
                   '\tint (*df)(pwn_ctx *, const pwn_vp_layout *, const void *, int, void *, void *, void *, void *) = pwn_trace_viewport_hits_device;\n'
                   '\treturn hf == NULL || df == NULL;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")])


def test_library_holds_the_new_modes_kernels():
    """COUNT x HAS_W x the three forms of the sphere lists, ORDER off, MODE 6 (tables.h PWN_KM_VIEWPORT_HITS): the twelve kernels'
    names in the built library (the host side registers every kernel of its code object under its mangled name)"""
    _lib()
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    assert re.search(r"\bPWN_KM_VIEWPORT_HITS = 6\b", tab)
    blob = open(LIB, "rb").read()
    found = set(re.findall(rb"_Z16pwn_trace_kernelILb([01])ELb([01])ELb([01])ELi([0-9])ELi6EEv16pwn_trace_params", blob))
    want = {(c, w, b"0", l) for c in (b"0", b"1") for w in (b"0", b"1") for l in (b"0", b"1", b"2")}
    assert found == want, sorted(found)


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    rects = np.array([(0, 0, 16, 8), (16, 0, 16, 8)], np.int32)
    cams = np.tile(np.eye(4, dtype=np.float32).ravel(), (2, 1))
    planes = np.full((3, 8, 32), 7, np.uint32)
    p = [planes[i].ctypes.data for i in range(3)]
    assert lib.pwn_trace_viewport_hits(None, 2, rects.ctypes.data, cams.ctypes.data, p[0], p[1], p[2]) == PWN_EINVAL
    assert lib.pwn_trace_viewport_hits(None, 2, rects.ctypes.data, cams.ctypes.data, p[0], None, None) == PWN_EINVAL
    assert lib.pwn_trace_viewport_hits(None, 0, None, None, None, None, None) == PWN_EINVAL
    assert lib.pwn_trace_viewport_hits_device(None, None, cams.ctypes.data, 0, p[0], p[1], p[2], None) == PWN_EINVAL
    assert lib.pwn_trace_viewport_hits_device(None, C.c_void_p(16), cams.ctypes.data, 0, p[0], None, None, None) == PWN_EINVAL
    assert (planes == 7).all()


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _bare_renderer(monkeypatch=None):
    import pwnfps_amd
    from pwnfps_amd import render
    if monkeypatch is not None:
        monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 32, 8, 0, C.c_void_p()
    return r


RECTS = np.array([(0, 0, 16, 8), (16, 0, 16, 8)], np.int32)


@pytest.mark.parametrize("rects, cams", [
    (np.zeros((0, 4), np.int32), np.zeros((0, 16), np.float32)),
    (np.zeros((2, 3), np.int32), np.zeros((2, 16), np.float32)),
    (np.zeros(4, np.int32), np.zeros((1, 16), np.float32)),
    (np.zeros((1025, 4), np.int32), np.zeros((1025, 16), np.float32)),
    (RECTS, np.zeros((3, 16), np.float32)),
    (RECTS, np.zeros((2, 15), np.float32)),
    (RECTS, np.zeros((2, 3, 4), np.float32)),
    (RECTS, np.zeros(32, np.float32)),
])
def test_trace_viewport_hits_rejects_bad_shapes_before_the_call(monkeypatch, rects, cams):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_viewport_hits(rects, cams)


def test_trace_viewport_hits_passes_good_shapes_to_the_library():
    """(with no context behind it the library answers PWN_EINVAL: the call got through)"""
    import pwnfps_amd
    r = _bare_renderer()
    for cams, kw in ((np.zeros((2, 4, 4), np.float32), {}), (np.zeros((2, 16), np.float64), dict(want_cell=False, want_dist=False))):
        with pytest.raises(pwnfps_amd.PwnError) as e:
            r.trace_viewport_hits(RECTS, cams, **kw)
        assert e.value.code == PWN_EINVAL


def test_device_wrapper_refuses_before_the_library_is_entered(monkeypatch):
    import torch
    import pwnfps_amd
    r = _bare_renderer(monkeypatch)
    other = _bare_renderer(monkeypatch)
    live = pwnfps_amd.ViewportsLayout(r, C.c_void_p(16), 32, 8, 2)
    freed = pwnfps_amd.ViewportsLayout(r, None, 32, 8, 2)
    foreign = pwnfps_amd.ViewportsLayout(other, C.c_void_p(16), 32, 8, 2)
    cams = torch.zeros((2, 16))
    label = torch.zeros((8, 32), dtype=torch.int32)
    # layouts: not one, a freed one, another renderer's
    for lay in (None, 123, freed, foreign):
        with pytest.raises(ValueError, match="layout"):
            r.trace_viewport_hits_device(lay, cams, label)
    # tensors that are not on a GPU, numpy arrays, raw pointers
    for bad in (cams, np.zeros((2, 16), np.float32), 123, None):
        with pytest.raises(ValueError, match="cams"):
            r.trace_viewport_hits_device(live, bad, label)
# (what the wrapper says of shape, dtype, contiguity, the device and the alignment of GPU tensors needs GPU tensors:
# tests/test_gpu_viewport_hits.py test_refusals)
