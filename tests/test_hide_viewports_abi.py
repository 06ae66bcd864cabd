"""pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device and pwn_trace_rays_hide_device without a GPU: the three
exports and their bindings, the header's contract text, the C entries' argument checks that need no context, and the names of their
kernels in the built library (a __global__ of its own, trace_hide_vp.hip: tests/test_hide_abi.py pins pwn_trace_kernel's set)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_trace_viewports_hide_device", "pwn_trace_viewport_hits_hide_device", "pwn_trace_rays_hide_device")


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
    names = {n: a for n, _, a in binding.ABI}
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    for e in ENTRIES:
        sibling = e.replace("_hide", "")
        assert hasattr(raw, e), e
        assert e in names, e
        # one pointer more than the call it shadows, in the binding and in the prototype
        assert len(names[e]) == len(names[sibling]) + 1, e
        assert names[e].count(C.c_void_p) == names[sibling].count(C.c_void_p) + 1, e
        protos = {n: re.search(r"^int %s\(([^;]*)\);" % n, hdr, re.M | re.S) for n in (e, sibling)}
        assert protos[e] and protos[sibling], e
        args = {n: [a.strip() for a in m.group(1).split(",")] for n, m in protos.items()}
        assert len(args[e]) == len(args[sibling]) + 1 and "const void *d_hide" in args[e], e
        assert [a for a in args[e] if a != "const void *d_hide"] == args[sibling], e
    for m in ("trace_viewports_device", "trace_viewport_hits_device", "trace_rays_device"):
        p = inspect.signature(getattr(pwnfps_amd.Renderer, m)).parameters
        assert "hide" in p and p["hide"].default is None, m


def test_header_names_the_calls_in_the_one_block():
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    assert hdr.count("One hidden sphere per view or ray") == 1
    sec = hdr[hdr.index("One hidden sphere per view or ray"):hdr.index("#define PWN_HIDE_NONE")]
    flat = re.sub(r"[\s*]+", " ", sec).lower()
    for phrase in ("pwn_trace_viewports_device", "pwn_trace_viewport_hits_device", "pwn_trace_rays_device", "the layout's count",
                   "rectangle i", "d_col / d_depth", "layout-use event", "changes nothing"):
        assert phrase in flat, phrase
    # the prototypes follow the block's, behind the define
    tail = hdr[hdr.index("#define PWN_HIDE_NONE"):]
    for e in ENTRIES:
        assert re.search(r"^int %s\(" % e, tail, re.M), e


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)
    assert lib.pwn_trace_viewports_hide_device(None, p, p, p, p, 0, p, p, p, None) == PWN_EINVAL
    assert lib.pwn_trace_viewport_hits_hide_device(None, p, p, p, 0, p, None, None, None) == PWN_EINVAL
    assert lib.pwn_trace_rays_hide_device(None, 1, p, p, p, 0.0, 0, p, p, None) == PWN_EINVAL


def test_library_holds_the_kernels_under_their_own_name():
    """COUNT x HAS_W x the three forms of the sphere lists, ORDER off, for PWN_KM_RAYS, PWN_KM_VIEWPORTS and PWN_KM_VIEWPORT_HITS with
    PWN_KM_HIDE or'ed in -- thirty-six instantiations of pwn_trace_hide2_kernel and no other; the set-up kernel takes the array"""
    _lib()
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    assert re.search(r"\bPWN_KM_HIDE = 8\b", tab)
    assert re.search(r"\bPWN_KM_RAYS = 2\b", tab) and re.search(r"\bPWN_KM_VIEWPORTS = 4\b", tab) and re.search(r"\bPWN_KM_VIEWPORT_HITS = 6\b", tab)
    blob = open(LIB, "rb").read()
    every = re.findall(rb"_Z22pwn_trace_hide2_kernelILb([01])ELb([01])ELb([01])ELi([0-9])ELi([0-9]+)EEv16pwn_trace_params", blob)
    found = {(c, w, o, l, int(m)) for c, w, o, l, m in every}
    want = {(c, w, b"0", l, m | 8) for c in (b"0", b"1") for w in (b"0", b"1") for l in (b"0", b"1", b"2") for m in (2, 4, 6)}
    assert found == want, sorted(found)
    assert b"_Z25pwn_viewport_setup_kernelPK" in blob
    assert hasattr(C.CDLL(LIB), "pwn_launch_viewport_setup_hide") and hasattr(C.CDLL(LIB), "pwn_launch_viewport_setup")
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    assert "trace_hide_vp.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert re.search(r"^\$\(B\)/trace_hide_vp\.o: HIPFLAGS \+= \$\(TRACE_EXTRA\)$", mk, re.M)


def test_the_record_word():
    """pwn_viewport_rec.hide: word 30 of a 128-byte record, and every path that makes records without an array leaves 0 there"""
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    rec = tab[tab.index("struct pwn_viewport_rec\n"):tab.index("#define PWN_VP_REC_BYTES 128u")]
    assert re.search(r"seg_shift;\s*uint32_t hide;\s*uint32_t pad_;\s*};", rec)
    setup = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "viewport_setup.hip")).read()
    assert "offsetof(pwn_viewport_rec, hide) == 120" in setup
    calls = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "pwn_calls.cpp")).read()
    bake = calls[calls.index("uint32_t pwn_i_viewport_recs_bake("):calls.index('extern "C" int pwn_trace_viewports(')]
    assert "r.hide = 0u;" in bake
