"""pwn_trace_hits without a GPU: the exports and bindings, pwn_hit's layout in the header against HIT_DTYPE and the ctypes
structure, the header's constants against the binding's, the C entries' argument checks, Renderer's shape checks before it calls
into the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_trace_hits", "pwn_trace_hits_device", "pwn_get_object_ids")
FIELDS = ("kind", "face", "object", "portals", "dist", "x", "y", "z", "dx", "dy", "dz", "cell_x", "cell_z")
OFFSETS = (0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 46)


def _lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    from pwnfps_amd import _lib as binding
    return binding.lib


def test_entries_are_exported_and_bound():
    _lib()
    raw = C.CDLL(LIB)
    from pwnfps_amd import _lib as binding
    import pwnfps_amd
    names = {n for n, _, _ in binding.ABI}
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    for e in ENTRIES:
        assert hasattr(raw, e), e
        assert e in names, e
        assert re.search(r"^int %s\(" % e, hdr, re.M), e
    for m in ("trace_hits", "trace_hits_device", "object_ids"):
        assert callable(getattr(pwnfps_amd.Renderer, m)), m


def test_hit_record_layout(tmp_path):
    """sizeof(pwn_hit) == 48 == HIT_DTYPE.itemsize, every field at the same offset in the header, the dtype and the ctypes structure"""
    import pwnfps_amd
    from pwnfps_amd import _lib as binding
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwnhip.h"\nint main(void) {\n'
                   '\tprintf("%zu", sizeof(pwn_hit));\n' +
                   "".join('\tprintf(" %%zu", offsetof(pwn_hit, %s));\n' % f for f in FIELDS) +
                   '\tprintf(" %d %d %d\\n", PWN_HIT_NONE, PWN_HIT_WALL, PWN_HIT_SPHERE);\n\treturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == 48 == pwnfps_amd.HIT_DTYPE.itemsize == C.sizeof(binding.Hit)
    assert tuple(out[1:14]) == OFFSETS
    assert pwnfps_amd.HIT_DTYPE.names == FIELDS == tuple(n for n, _ in binding.Hit._fields_)
    for f, o in zip(FIELDS, OFFSETS):
        assert pwnfps_amd.HIT_DTYPE.fields[f][1] == o == getattr(binding.Hit, f).offset, f
    for f in FIELDS[:4]:
        assert pwnfps_amd.HIT_DTYPE[f] == np.dtype("<i4")
    for f in FIELDS[4:11]:
        assert pwnfps_amd.HIT_DTYPE[f] == np.dtype("<f4")
    for f in FIELDS[11:]:
        assert pwnfps_amd.HIT_DTYPE[f] == np.dtype("<i2")
    assert tuple(out[14:]) == (binding.PWN_HIT_NONE, binding.PWN_HIT_WALL, binding.PWN_HIT_SPHERE) == (0, 1, 2)


def test_c_entries_refuse_bad_arguments_without_a_context():
    lib = _lib()
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros(4 * 48 + 16, np.uint8)
    ids = np.zeros(4, np.int32)
    assert lib.pwn_trace_hits(None, 4, rays.ctypes.data, hits.ctypes.data) == PWN_EINVAL
    assert lib.pwn_trace_hits(None, 0, None, None) == PWN_EINVAL
    assert lib.pwn_trace_hits(None, -1, rays.ctypes.data, hits.ctypes.data) == PWN_EINVAL
    assert lib.pwn_trace_hits_device(None, 4, rays.ctypes.data, 0, hits.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_trace_hits_device(None, (1 << 28) + 1, rays.ctypes.data, 0, hits.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_get_object_ids(None, ids.ctypes.data, 4) == PWN_EINVAL


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


@pytest.mark.parametrize("rays", [
    np.zeros((3, 7), np.float32),
    np.zeros(8, np.float32),
    np.zeros((3, 8, 1), np.float32),
    (np.zeros((3, 3)), np.zeros((2, 3))),
    (np.zeros((3, 2)), np.zeros((3, 3))),
    (np.zeros((3, 3)), np.zeros((3, 5))),
    (np.zeros(3), np.zeros((3, 3))),
])
def test_trace_hits_rejects_bad_shapes_before_the_call(monkeypatch, rays):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_hits(rays)


@pytest.mark.parametrize("kw", [
    dict(rays=123, hits=456),                         # device pointers without n
    dict(rays=123, hits=456, n=-1),
    dict(rays=123, hits=456, n=(1 << 28) + 1),
    dict(rays=np.zeros((3, 8), np.float32), hits=456, n=3),       # one of each
    dict(rays=np.zeros((3, 8), np.float32), hits=np.zeros((3, 12), np.int32)),     # not GPU tensors
])
def test_trace_hits_device_rejects_bad_arguments_before_the_call(monkeypatch, kw):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_hits_device(**kw)
