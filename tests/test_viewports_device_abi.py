"""pwn_viewports_layout, _free, _info and pwn_trace_viewports_device without a GPU: the exports, the bindings and the header's
prototypes, every refusal that needs no context, Renderer's argument checks with the library replaced by an object that fails on
any call, and the new kernel in the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = {"pwn_viewports_layout": 6, "pwn_viewports_layout_free": 2, "pwn_viewports_layout_info": 2, "pwn_trace_viewports_device": 9}


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
        assert hasattr(raw, entry)
        bound = [a for n, _, a in binding.ABI if n == entry]
        assert len(bound) == 1 and len(bound[0]) == nargs
        decl = re.search(r"^int %s\(([^;]*)\);" % entry, hdr, re.M)
        assert decl and len(decl.group(1).split(",")) == nargs
    assert re.search(r"^typedef struct pwn_vp_layout pwn_vp_layout;", hdr, re.M)
    assert re.search(r"^int pwn_viewports_layout\(pwn_ctx \*ctx, int W, int H, int n, const pwn_viewport \*vp, pwn_vp_layout \*\*out\);", hdr, re.M)
    assert re.search(r"^int pwn_viewports_layout_free\(pwn_ctx \*ctx, pwn_vp_layout \*layout\);", hdr, re.M)
    assert re.search(r"^int pwn_viewports_layout_info\(const pwn_vp_layout \*layout, unsigned long long out\[6\]\);", hdr, re.M)
    assert re.search(r"^int pwn_trace_viewports_device\(pwn_ctx \*ctx, const pwn_vp_layout \*layout, const void \*d_cams, const void \*d_secs, int flags,\n"
                     r"\tvoid \*d_work, void \*d_sbuf, void \*d_zbuf, void \*stream\);", hdr, re.M)
    assert callable(pwnfps_amd.Renderer.viewports_layout) and callable(pwnfps_amd.Renderer.trace_viewports_device)
    assert callable(pwnfps_amd.ViewportsLayout.info) and callable(pwnfps_amd.ViewportsLayout.free)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "pwnhip.h"\n'
                   'int main(void) {\n'
                   '\tint (*mk)(pwn_ctx *, int, int, int, const pwn_viewport *, pwn_vp_layout **) = pwn_viewports_layout;\n'
                   '\tint (*fr)(pwn_ctx *, pwn_vp_layout *) = pwn_viewports_layout_free;\n'
                   '\tint (*nf)(const pwn_vp_layout *, unsigned long long *) = pwn_viewports_layout_info;\n'
                   '\tint (*tr)(pwn_ctx *, const pwn_vp_layout *, const void *, const void *, int, void *, void *, void *, void *) = pwn_trace_viewports_device;\n'
                   '\t_Static_assert(sizeof(pwn_viewport) == 16 && PWN_VIEWS_MAX == 1024 && PWN_VIEWS_HAS_W == 1, "what the contract names");\n'
                   '\treturn mk == NULL || fr == NULL || nf == NULL || tr == NULL;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")])


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    rects = np.array([(0, 0, 16, 8), (16, 0, 16, 8)], np.int32)
    out = C.c_void_p(7)
    assert lib.pwn_viewports_layout(None, 32, 8, 2, rects.ctypes.data, C.byref(out)) == PWN_EINVAL and out.value == 7
    assert lib.pwn_viewports_layout(None, 32, 8, 2, rects.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_viewports_layout_free(None, None) == PWN_EINVAL
    info = (C.c_uint64 * 6)(*([7] * 6))
    assert lib.pwn_viewports_layout_info(None, info) == PWN_EINVAL and list(info) == [7] * 6
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert lib.pwn_trace_viewports_device(None, None, p, p, 0, p, p, p, None) == PWN_EINVAL
    assert (buf == 0).all()


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _bare_renderer(monkeypatch):
    import pwnfps_amd
    from pwnfps_amd import render
    monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    return r


def test_python_refuses_before_the_library_is_entered(monkeypatch):
    import torch
    import pwnfps_amd
    r = _bare_renderer(monkeypatch)
    other = _bare_renderer(monkeypatch)
    # rectangles
    for rects in (np.zeros((0, 4), np.int32), np.zeros((3, 3), np.int32), np.zeros(4, np.int32), np.zeros((1025, 4), np.int32)):
        with pytest.raises(ValueError):
            r.viewports_layout(32, 8, rects)
    # layouts: not one, a freed one, another renderer's
    live = pwnfps_amd.ViewportsLayout(r, C.c_void_p(16), 32, 8, 2)
    freed = pwnfps_amd.ViewportsLayout(r, None, 32, 8, 2)
    foreign = pwnfps_amd.ViewportsLayout(other, C.c_void_p(16), 32, 8, 2)
    cams, secs = torch.zeros((2, 16)), torch.zeros(2)
    sb, zb = torch.zeros((8, 32), dtype=torch.int32), torch.zeros((8, 32))
    for lay in (None, 123, freed, foreign):
        with pytest.raises(ValueError, match="layout"):
            r.trace_viewports_device(lay, cams, secs, sb, zb)
    # tensors that are not on a GPU, numpy arrays, raw pointers
    for bad in (dict(cams=cams), dict(cams=np.zeros((2, 16), np.float32)), dict(cams=123), dict(cams=None)):
        with pytest.raises(ValueError, match="cams"):
            r.trace_viewports_device(live, bad["cams"], secs, sb, zb)
    with pytest.raises(ValueError):
        freed.info()
    freed.free()          # (a layout that is gone: nothing to do, and nothing called)
# (what the wrapper says of shape, dtype, contiguity, the device and the alignment of GPU tensors needs GPU tensors:
# tests/test_gpu_viewports_device.py test_refusals)


def test_library_holds_the_setup_kernel():
    """the kernel is registered under its mangled name, both new objects are in the Makefile's list, and the kernel's file is built
    without the denormal flush"""
    _lib()
    blob = open(LIB, "rb").read()
    assert re.search(rb"_Z25pwn_viewport_setup_kernelPK", blob)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    obj = re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert "viewport_setup.o" in obj and "pwn_viewports_device.o" in obj
    rule = re.search(r"^\$\(B\)/viewport_setup\.o:.*\n\t.*\n\t(.*)$", mk, re.M)
    assert rule and "$(VIEW_SETUP_FLAGS)" in rule.group(1)
