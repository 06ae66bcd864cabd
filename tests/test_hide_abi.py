"""The *_hide_device calls without a GPU: the three exports and their bindings, the header's contract text, the C entries'
argument checks that need no context, and the HIDE kernels' names in the built library."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_trace_views_hide_device", "pwn_trace_view_hits_hide_device", "pwn_trace_hits_hide_device")


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
        assert hasattr(raw, e), e
        assert e in names, e
        assert re.search(r"^int %s\(" % e, hdr, re.M), e
        # one pointer more than the call it shadows
        assert len(names[e]) == len(names[e.replace("_hide", "")]) + 1, e
    assert re.search(r"^#define PWN_HIDE_NONE \(-1\)$", hdr, re.M) and binding.PWN_HIDE_NONE == -1
    for m in ("trace_views_device", "trace_view_hits_device", "trace_hits_device"):
        p = inspect.signature(getattr(pwnfps_amd.Renderer, m)).parameters
        assert "hide" in p and p["hide"].default is None, m


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    sec = hdr[hdr.index("One hidden sphere per view or ray"):hdr.index("#define PWN_HIDE_NONE")]
    flat = re.sub(r"[\s*]+", " ", sec).lower()
    assert "only ever compared" in flat
    assert "no bit pattern of it reaches an address or a loop bound" in flat
    for phrase in ("full table", "every segment", "sphere_tests", "pwn_hide_none", "int_max", "launches nothing"):
        assert phrase in flat, phrase


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)
    assert lib.pwn_trace_views_hide_device(None, 1, p, p, p, 0, p, p, p, None) == PWN_EINVAL
    assert lib.pwn_trace_view_hits_hide_device(None, 1, p, p, 0, p, None, None, None) == PWN_EINVAL
    assert lib.pwn_trace_hits_hide_device(None, 1, p, p, 0, p, None) == PWN_EINVAL


def test_library_holds_the_hide_kernels():
    """COUNT x HAS_W x the three forms of the sphere lists, ORDER off, for the three modes that have a HIDE instantiation (tables.h:
    PWN_KM_VIEWS, PWN_KM_HITS, PWN_KM_VIEW_HITS with PWN_KM_HIDE or'ed in) -- thirty-six kernels, and no other mode with that bit"""
    _lib()
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    assert re.search(r"\bPWN_KM_HIDE = 8\b", tab)
    assert re.search(r"\bPWN_KM_VIEWS = 1\b", tab) and re.search(r"\bPWN_KM_HITS = 3\b", tab) and re.search(r"\bPWN_KM_VIEW_HITS = 5\b", tab)
    blob = open(LIB, "rb").read()
    every = re.findall(rb"_Z16pwn_trace_kernelILb([01])ELb([01])ELb([01])ELi([0-9])ELi([0-9]+)EEv16pwn_trace_params", blob)
    found = {(c, w, o, l, int(m)) for c, w, o, l, m in every if int(m) >= 8}
    want = {(c, w, b"0", l, m | 8) for c in (b"0", b"1") for w in (b"0", b"1") for l in (b"0", b"1", b"2") for m in (1, 3, 5)}
    assert found == want, sorted(found)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    assert "trace_hide.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert re.search(r"^\$\(B\)/trace_hide\.o: HIPFLAGS \+= \$\(TRACE_EXTRA\)$", mk, re.M)
