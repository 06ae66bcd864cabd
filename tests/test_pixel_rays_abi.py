"""pwn_pixel_rays_device without a GPU: the export, the binding and the header entry, its two constants, the C entry's refusal of a
NULL context, Renderer's argument checks before it calls into the library, and the new kernel in the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRY = "pwn_pixel_rays_device"


def _lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    from pwnfps_amd import _lib as binding
    return binding.lib


def test_entry_is_exported_bound_and_declared():
    _lib()
    raw = C.CDLL(LIB)
    from pwnfps_amd import _lib as binding
    import pwnfps_amd
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    assert hasattr(raw, ENTRY)
    bound = [a for n, _, a in binding.ABI if n == ENTRY]
    assert len(bound) == 1 and len(bound[0]) == 12
    decl = re.search(r"^int %s\(([^;]*)\);" % ENTRY, hdr, re.M)
    assert decl and len(decl.group(1).split(",")) == 12
    assert callable(pwnfps_amd.Renderer.pixel_rays_device)
    assert pwnfps_amd.PWN_PIXELS_SHARED == 1 and pwnfps_amd.PWN_PIXEL_WORK_BYTES == 80


def test_constants(tmp_path):
    """a C program with the header: the two constants; and a camera's scratch is a view record (tables.h PWN_VIEWS_REC_BYTES)"""
    src = tmp_path / "consts.c"
    src.write_text('#include <stdint.h>\n#include "pwnhip.h"\n'
                   'int main(void) {\n'
                   '\t_Static_assert(PWN_PIXELS_SHARED == 1, "flag");\n'
                   '\t_Static_assert(PWN_PIXEL_WORK_BYTES == 80, "scratch per camera");\n'
                   '\t_Static_assert(PWN_PIXEL_WORK_BYTES * (long long)PWN_PLAYERS_MAX < (1ll << 31), "scratch of the largest batch");\n'
                   '\treturn 0;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "consts")])
    subprocess.check_call([str(tmp_path / "consts")])
    tables = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    rec = re.search(r"^#define PWN_VIEWS_REC_BYTES (\d+)u?\s*$", tables, re.M)
    assert rec and int(rec.group(1)) == 80
    # (and the kernel's file holds the two to each other when it is compiled)
    hip = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "pixel_rays.hip")).read()
    assert "static_assert(sizeof(pwn_view_rec) == PWN_PIXEL_WORK_BYTES" in hip


def test_c_entry_refuses_a_null_context():
    lib = _lib()
    n, m = 4, 3
    buf = np.zeros(1024, np.float32)          # 16-byte aligned at its start (numpy allocates so); room for every range
    base = buf.ctypes.data
    assert base % 16 == 0
    cams, xy, work, rays, seeds = base, base + 256, base + 512, base + 1024, base + 2048
    for args in [(None, 32, 16, n, cams, m, xy, 0, work, rays, seeds, None), (None, 32, 16, n, cams, m, xy, 1, work, rays, None, None),
                 (None, 32, 16, 0, None, 0, None, 0, None, None, None, None), (None, 4, 3, n, cams, 12, None, 1, work, rays, seeds, None)]:
        assert lib.pwn_pixel_rays_device(*args) == PWN_EINVAL, args
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


def _cases():
    import torch
    n, m = 3, 2
    t = dict(cams=torch.zeros((n, 16)), xy=torch.zeros((m, 2), dtype=torch.int32))
    return [
        dict(cams=np.zeros((n, 16), np.float32), xy=np.zeros((m, 2), np.int32)),          # numpy arrays are not taken
        t,                                                                                 # tensors, but not on a GPU
        dict(t, cams=123),                                                                 # raw pointers are not taken
        dict(t, cams=None),
        dict(cams=torch.zeros((n, 16))),                                                   # the whole frame, cameras not on a GPU
        dict(t, width=0), dict(t, height=40000), dict(t, shared=False), dict(t, shared=1),
        dict(t, rays=np.zeros((n * m, 8), np.float32)), dict(t, seeds=np.zeros(n * m, np.uint32)), dict(t, work=bytearray(80 * n)),
    ]
# (what the wrapper says of dtype, shape, contiguity, the device and the alignment of GPU tensors needs GPU tensors:
# tests/test_gpu_pixel_rays.py test_python_refuses_before_the_library_is_entered)


@pytest.mark.parametrize("case", range(12))
def test_pixel_rays_device_rejects_bad_arguments_before_the_call(monkeypatch, case):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.pixel_rays_device(**_cases()[case])


def test_library_holds_the_ray_kernel():
    """the kernel is registered under its mangled name, and both new objects are in the Makefile's list"""
    _lib()
    blob = open(LIB, "rb").read()
    assert re.search(rb"_Z21pwn_pixel_rays_kernelPK", blob)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    assert "pixel_rays.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0) and "pwn_pixel_rays.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0)
