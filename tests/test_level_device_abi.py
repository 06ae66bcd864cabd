"""pwn_upload_level_device, pwn_level_device_state and pwn_get_level_device without a GPU: the exports, the bindings and the header's
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
ENTRIES = {"pwn_upload_level_device": 4, "pwn_level_device_state": 2, "pwn_get_level_device": 3}


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
    assert re.search(r"^int pwn_upload_level_device\(pwn_ctx \*ctx, const void \*d_data, const void \*d_pmap, void \*stream\);", hdr, re.M)
    assert re.search(r"^int pwn_level_device_state\(pwn_ctx \*ctx, unsigned long long out\[8\]\);", hdr, re.M)
    assert re.search(r"^int pwn_get_level_device\(pwn_ctx \*ctx, uint8_t data\[4096\], pwn_portal pmap\[26\]\);", hdr, re.M)
    for m in ("upload_level_device", "level_device_state", "get_level_device"):
        assert callable(getattr(pwnfps_amd.Renderer, m))
    # the contract states the number of launches, which tools/sanitize/level_device_driver.cpp pins
    doc = hdr[hdr.index("The level's tables baked on the device"):hdr.index("int pwn_upload_level_device(")]
    assert "FIVE launches" in doc


def test_header_compiles_as_c_and_a_portal_is_seven_words(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "pwnhip.h"\n'
                   'int main(void) {\n'
                   '\tint (*up)(pwn_ctx *, const void *, const void *, void *) = pwn_upload_level_device;\n'
                   '\tint (*st)(pwn_ctx *, unsigned long long *) = pwn_level_device_state;\n'
                   '\tint (*get)(pwn_ctx *, uint8_t *, pwn_portal *) = pwn_get_level_device;\n'
                   '\t_Static_assert(sizeof(pwn_portal) == 28 && offsetof(pwn_portal, rot12) == 16 && offsetof(pwn_portal, c2) == 24, "record");\n'
                   '\treturn up == NULL || st == NULL || get == NULL;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")])


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    buf = np.zeros(4096 + 64, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    for args in [(None, p, p, None), (None, p, None, None), (None, None, None, None), (None, p + 1, None, None), (None, p, p + 4, None)]:
        assert lib.pwn_upload_level_device(*args) == PWN_EINVAL, args
    out = (C.c_uint64 * 8)(*([7] * 8))
    assert lib.pwn_level_device_state(None, out) == PWN_EINVAL and list(out) == [7] * 8
    assert lib.pwn_get_level_device(None, p, None) == PWN_EINVAL
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
    return [
        (np.zeros((64, 64), np.uint8), None),                  # numpy arrays are not taken
        (torch.zeros((64, 64), dtype=torch.uint8), None),      # a tensor, but not on a GPU
        (123, None), (None, None),                             # raw pointers are not taken, and the grid is needed
        (torch.zeros((64, 64), dtype=torch.int32), None), (torch.zeros((4096,), dtype=torch.uint8), None),
        (torch.zeros((64, 128), dtype=torch.uint8)[:, ::2], None),
        (torch.zeros((64, 64), dtype=torch.uint8), np.zeros((26, 7), np.int32)),
    ]
# (what the wrapper says of shape, dtype, contiguity, the device and the alignment of GPU tensors needs GPU tensors:
# tests/test_gpu_level_device.py test_python_refuses_before_the_library_is_entered)


@pytest.mark.parametrize("case", range(8))
def test_upload_level_device_rejects_bad_arguments_before_the_call(monkeypatch, case):
    r = _bare_renderer(monkeypatch)
    data, pmap = _cases()[case]
    with pytest.raises(ValueError) as e:
        r.upload_level_device(data, pmap)
    assert str(e.value).startswith("upload_level_device: ")


def test_library_holds_the_bake_kernel():
    """the kernel is registered under its mangled name, both new objects are in the Makefile's list, and the kernels' file is built
    with the flags of the other small kernels"""
    _lib()
    blob = open(LIB, "rb").read()
    assert re.search(rb"_Z21pwn_level_bake_kernelPK", blob)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    obj = re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert "level_bake.o" in obj and "pwn_level_device.o" in obj
    rule = re.search(r"^\$\(B\)/level_bake\.o:.*level_bake\.h.*\n\t.*\n\t(.*)$", mk, re.M)
    assert rule and "$(VIEW_SETUP_FLAGS)" in rule.group(1)
