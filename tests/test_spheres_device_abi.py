"""pwn_upload_spheres_device and pwn_spheres_device_state without a GPU: the exports, the bindings and the header's prototypes, every
refusal that needs no context, Renderer's argument checks with the library replaced by an object that fails on any call, and the
new kernels in the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = {"pwn_upload_spheres_device": 5, "pwn_spheres_device_state": 2}


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
    assert re.search(r"^int pwn_upload_spheres_device\(pwn_ctx \*ctx, int n, const void \*d_spheres, int max_pairs, void \*stream\);", hdr, re.M)
    assert re.search(r"^int pwn_spheres_device_state\(pwn_ctx \*ctx, unsigned long long out\[8\]\);", hdr, re.M)
    assert callable(pwnfps_amd.Renderer.upload_spheres_device) and callable(pwnfps_amd.Renderer.spheres_device_state)


def test_header_compiles_as_c_and_a_record_is_32_bytes(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "pwnhip.h"\n'
                   'int main(void) {\n'
                   '\tint (*up)(pwn_ctx *, int, const void *, int, void *) = pwn_upload_spheres_device;\n'
                   '\tint (*st)(pwn_ctx *, unsigned long long *) = pwn_spheres_device_state;\n'
                   '\t_Static_assert(sizeof(pwn_sphere) == 32 && offsetof(pwn_sphere, r) == 0 && offsetof(pwn_sphere, x) == 8 && offsetof(pwn_sphere, cr) == 28, "record");\n'
                   '\t_Static_assert(PWN_LIST_MAX == 4096 && PWN_OBJ_MAX == 10000, "limits the contract names");\n'
                   '\treturn up == NULL || st == NULL;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")])


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert p % 16 == 0
    for args in [(None, 4, p, 100, None), (None, 0, None, 0, None), (None, -1, p, 100, None), (None, 4, p, -1, None), (None, 4, None, 100, None),
                 (None, 4, p + 4, 100, None), (None, 10001, p, 100, None), (None, 4, p, 2 ** 31 - 1, None)]:
        assert lib.pwn_upload_spheres_device(*args) == PWN_EINVAL, args
    out = (C.c_uint64 * 8)(*([7] * 8))
    assert lib.pwn_spheres_device_state(None, out) == PWN_EINVAL and list(out) == [7] * 8
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
    t = torch.zeros((6, 8))
    return [
        (np.zeros((6, 8), np.float32), 10),                # numpy arrays are not taken
        (t, 10),                                           # a tensor, but not on a GPU
        (123, 10), (None, 10),                             # raw pointers are not taken
        (torch.zeros((6, 8), dtype=torch.float64), 10), (torch.zeros((48,)), 10), (torch.zeros((6, 7)), 10), (torch.zeros((6, 16))[:, ::2], 10),
    ]
# (what the wrapper says of shape, dtype, contiguity, the device, the alignment and max_pairs of GPU tensors needs GPU tensors:
# tests/test_gpu_spheres_device.py test_python_refuses_before_the_library_is_entered)


@pytest.mark.parametrize("case", range(8))
def test_upload_spheres_device_rejects_bad_arguments_before_the_call(monkeypatch, case):
    r = _bare_renderer(monkeypatch)
    sph, mp = _cases()[case]
    with pytest.raises(ValueError):
        r.upload_spheres_device(sph, mp)


def test_library_holds_the_builder_kernels():
    """the three kernels (the list pass in both instantiations) are registered under their mangled names, both new objects are in
    the Makefile's list, and the kernels' file is built without the denormal flush"""
    _lib()
    blob = open(LIB, "rb").read()
    assert re.search(rb"_Z23pwn_sphere_boxes_kernelPK", blob)
    assert re.search(rb"_Z22pwn_sphere_scan_kernelPK", blob)
    assert re.search(rb"_Z23pwn_sphere_lists_kernelILb0EEvPK", blob) and re.search(rb"_Z23pwn_sphere_lists_kernelILb1EEvPK", blob)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    obj = re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert "sphere_bins.o" in obj and "pwn_spheres_device.o" in obj
    rule = re.search(r"^\$\(B\)/sphere_bins\.o:.*\n\t.*\n\t(.*)$", mk, re.M)
    assert rule and "$(VIEW_SETUP_FLAGS)" in rule.group(1)
