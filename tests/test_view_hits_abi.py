"""pwn_trace_view_hits without a GPU: the exports and bindings, the header's PWN_LABEL_* macros against unpack_labels / pack_labels
on hand-made words, the C entries' argument checks, Renderer's shape and dtype checks before it calls into the library, and the
new kernel mode's twelve variants in the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_trace_view_hits", "pwn_trace_view_hits_device")
# (word, kind, face, object, portals): nothing; a wall of face 5 (FYN) behind 1000 portals; sphere 9999 (the last of PWN_OBJ_MAX); sphere 0
WORDS = [(0, 0, -1, -1, 0),
         (1 | (6 << 2) | (1000 << 19), 1, 5, -1, 1000),
         (2 | (10000 << 5), 2, -1, 9999, 0),
         (2 | (1 << 5), 2, -1, 0, 0)]


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
    for m in ("trace_view_hits", "trace_view_hits_device"):
        assert callable(getattr(pwnfps_amd.Renderer, m)), m
    assert callable(pwnfps_amd.unpack_labels) and callable(pwnfps_amd.pack_labels)


def test_label_macros_and_python_agree(tmp_path):
    """PWN_LABEL_KIND / _FACE / _OBJECT / _PORTALS of the header, unpack_labels and pack_labels on the hand-made words"""
    import pwnfps_amd
    src = tmp_path / "labels.c"
    src.write_text('#include <stdio.h>\n#include <stdint.h>\n#include "pwnhip.h"\nint main(void) {\n'
                   '\tstatic const uint32_t w[] = { %s };\n' % ", ".join("%uu" % v[0] for v in WORDS) +
                   '\tfor(int i = 0; i < %d; i++) printf("%%u %%d %%d %%u\\n", (unsigned)PWN_LABEL_KIND(w[i]), PWN_LABEL_FACE(w[i]), '
                   'PWN_LABEL_OBJECT(w[i]), (unsigned)PWN_LABEL_PORTALS(w[i]));\n\treturn 0;\n}\n' % len(WORDS))
    exe = tmp_path / "labels"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    from_c = [tuple(int(v) for v in ln.split()) for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    assert from_c == [v[1:] for v in WORDS]
    words = np.array([v[0] for v in WORDS], np.uint32)
    kind, face, obj, portals = pwnfps_amd.unpack_labels(words)
    assert list(zip(kind.tolist(), face.tolist(), obj.tolist(), portals.tolist())) == [v[1:] for v in WORDS]
    hits = np.zeros(len(WORDS), pwnfps_amd.HIT_DTYPE)
    hits["kind"], hits["face"], hits["object"], hits["portals"] = kind, face, obj, portals
    packed = pwnfps_amd.pack_labels(hits)
    assert packed.dtype == np.uint32 and packed.tolist() == words.tolist()
    # (shapes are kept, and the other fields of a record do not matter)
    hits["dist"], hits["cell_x"] = 3.5, -7
    assert (pwnfps_amd.pack_labels(hits.reshape(2, 2)) == words.reshape(2, 2)).all()
    assert all(a.shape == (2, 2) for a in pwnfps_amd.unpack_labels(words.reshape(2, 2)))
    with pytest.raises(ValueError):
        pwnfps_amd.pack_labels(np.zeros(4, np.uint32))


def test_c_entries_refuse_bad_arguments_without_a_context():
    lib = _lib()
    cams = np.tile(np.eye(4, dtype=np.float32).ravel(), (2, 1))
    planes = np.zeros((3, 2, 4, 4), np.uint32)
    p = [planes[i].ctypes.data for i in range(3)]
    assert lib.pwn_trace_view_hits(None, 2, cams.ctypes.data, p[0], p[1], p[2]) == PWN_EINVAL
    assert lib.pwn_trace_view_hits(None, 2, cams.ctypes.data, p[0], None, None) == PWN_EINVAL
    assert lib.pwn_trace_view_hits(None, 0, None, None, None, None) == PWN_EINVAL
    assert lib.pwn_trace_view_hits_device(None, 2, cams.ctypes.data, 0, p[0], p[1], p[2], None) == PWN_EINVAL
    assert lib.pwn_trace_view_hits_device(None, 2, cams.ctypes.data, 0, p[0], None, None, None) == PWN_EINVAL


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _bare_renderer(monkeypatch=None):
    import pwnfps_amd
    from pwnfps_amd import render
    if monkeypatch is not None:
        monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    return r


@pytest.mark.parametrize("cams", [
    np.zeros((2, 3, 4), np.float32),
    np.zeros((2, 15), np.float32),
    np.zeros(16, np.float32),
    np.zeros((0, 16), np.float32),
    np.zeros((1025, 16), np.float32),
    np.zeros((2, 4, 4, 1), np.float32),
])
def test_trace_view_hits_rejects_bad_shapes_before_the_call(monkeypatch, cams):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_view_hits(cams)


def test_trace_view_hits_passes_good_shapes_to_the_library():
    """(with no context behind it the library answers PWN_EINVAL: the call got through)"""
    import pwnfps_amd
    r = _bare_renderer()
    for cams, kw in ((np.zeros((3, 4, 4), np.float32), {}), (np.zeros((3, 16), np.float64), dict(want_cell=False, want_dist=False))):
        with pytest.raises(pwnfps_amd.PwnError) as e:
            r.trace_view_hits(cams, **kw)
        assert e.value.code == PWN_EINVAL


def _device_cases():
    import torch
    n, h, w = 2, 4, 8
    cams = torch.zeros((n, 16), dtype=torch.float32)
    label = torch.zeros((n, h, w), dtype=torch.int32)
    return [
        dict(cams=np.zeros((n, 16), np.float32), label=np.zeros((n, h, w), np.int32)),          # not tensors
        dict(cams=cams, label=label),                                                            # tensors, but not on a GPU
        dict(cams=123, label=456),                                                               # raw pointers are not taken
        dict(cams=cams, label=label, cell=np.zeros((n, h, w), np.int32)),
        dict(cams=cams, label=label, dist=label),
    ]


@pytest.mark.parametrize("case", range(5))
def test_trace_view_hits_device_rejects_bad_arguments_before_the_call(monkeypatch, case):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_view_hits_device(**_device_cases()[case])


def test_library_holds_the_new_modes_kernels():
    """COUNT x HAS_W x the three forms of the sphere lists, ORDER off, MODE 5 (tables.h PWN_KM_VIEW_HITS): the twelve kernels'
    names in the built library (the host side registers every kernel of its code object under its mangled name)"""
    _lib()
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    assert re.search(r"\bPWN_KM_VIEW_HITS = 5\b", tab)
    blob = open(LIB, "rb").read()
    found = set(re.findall(rb"_Z16pwn_trace_kernelILb([01])ELb([01])ELb([01])ELi([0-9])ELi5EEv16pwn_trace_params", blob))
    want = {(c, w, b"0", l) for c in (b"0", b"1") for w in (b"0", b"1") for l in (b"0", b"1", b"2")}
    assert found == want, sorted(found)
