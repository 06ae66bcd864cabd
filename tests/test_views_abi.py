"""pwn_trace_views without a GPU: the export, the header's constant against the binding's, the C entry's argument check,
and Renderer.trace_views refusing badly shaped cameras before it calls into the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")


def _lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    return C.CDLL(LIB)


def test_trace_views_is_exported():
    assert hasattr(_lib(), "pwn_trace_views")
    from pwnfps_amd import _lib as binding
    assert "pwn_trace_views" in {n for n, _, _ in binding.ABI}


def test_views_max_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    m = re.search(r"^#define\s+PWN_VIEWS_MAX\s+(\d+)", hdr, re.M)
    assert m is not None
    from pwnfps_amd import _lib as binding
    assert int(m.group(1)) == binding.PWN_VIEWS_MAX == 1024


def test_null_context_is_einval():
    lib = _lib()
    lib.pwn_trace_views.restype = C.c_int
    lib.pwn_trace_views.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cams = np.tile(np.eye(4, dtype=np.float32).ravel(), (2, 1))
    secs = np.zeros(2, np.float32)
    sb = np.zeros((2, 4, 4), np.uint32)
    assert lib.pwn_trace_views(None, 2, cams.ctypes.data, secs.ctypes.data, sb.ctypes.data, None) == -1     # PWN_EINVAL


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


@pytest.mark.parametrize("cams,secs", [
    (np.zeros((2, 3, 4), np.float32), np.zeros(2, np.float32)),
    (np.zeros((2, 15), np.float32), np.zeros(2, np.float32)),
    (np.zeros(16, np.float32), np.zeros(1, np.float32)),
    (np.zeros((0, 16), np.float32), np.zeros(0, np.float32)),
    (np.zeros((1025, 16), np.float32), np.zeros(1025, np.float32)),
    (np.zeros((2, 4, 4), np.float32), np.zeros(3, np.float32)),
    (np.zeros((2, 16), np.float32), np.zeros((2, 1), np.float32)),
])
def test_renderer_rejects_bad_shapes_before_the_call(monkeypatch, cams, secs):
    import pwnfps_amd
    from pwnfps_amd import render
    monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    with pytest.raises(ValueError):
        r.trace_views(cams, secs)


def test_renderer_passes_good_shapes_to_the_library():
    """(with no context behind it the library answers PWN_EINVAL: the call got through)"""
    import pwnfps_amd
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    for cams in (np.zeros((3, 4, 4), np.float32), np.zeros((3, 16), np.float64)):
        with pytest.raises(pwnfps_amd.PwnError) as e:
            r.trace_views(cams, [0.0, 1.0, 2.0])
        assert e.value.code == -1
