"""pwn_trace_reach and its two device forms without a GPU: the exports and their bindings, PWN_HIT_FREE, the header's contract text, the
C entries' refusals that need no context (tests/test_reach_host.py has every other refusal, with nothing launched, on the stand-in
runtime), and the REACH kernels' names in the built library."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_trace_reach", "pwn_trace_reach_device", "pwn_trace_reach_hide_device")


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
        # one pointer more than the pwn_trace_hits form it shadows
        assert len(names[e]) == len(names[e.replace("_reach", "_hits")]) + 1, e
    assert re.search(r"^#define PWN_HIT_FREE\s+3\b", hdr, re.M) and binding.PWN_HIT_FREE == 3
    p = inspect.signature(pwnfps_amd.Renderer.trace_reach).parameters
    assert list(p)[1:] == ["rays", "reach"]
    p = inspect.signature(pwnfps_amd.Renderer.trace_reach_device).parameters
    assert list(p)[1:6] == ["rays", "reach", "hits", "hide", "has_w"] and p["hide"].default is None and p["has_w"].default is False


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    sec = hdr[hdr.index("Rays that stop after a given distance"):hdr.index("#define PWN_HIT_FREE")]
    flat = re.sub(r"[\s*]+", " ", sec).lower()
    assert "trace.h:186" in flat and "trace.h:250" in flat
    assert "no bit pattern of it reaches an address or a loop bound" in flat
    for phrase in ("a process, not geometry", "whichever comes first", "bit for bit", "pwn_hit_none", "portals = p_k", "dist = reach",
                   "without a ramp's skew", "never fused", "never the reach step", "+inf", "nan is never exceeded", "negative reach",
                   "reach = 0", "pwn_hide_none", "up to and including the reach step", "one trace launch", "84 b a ray",
                   "must not overlap d_hits", "launches nothing", "profiles/reach/bench.txt"):
        assert phrase in flat, phrase


def test_c_entries_refuse_without_a_context():
    lib = _lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)
    assert lib.pwn_trace_reach(None, 1, p, p, p) == PWN_EINVAL
    assert lib.pwn_trace_reach_device(None, 1, p, p, 0, p, None) == PWN_EINVAL
    assert lib.pwn_trace_reach_hide_device(None, 1, p, p, p, 0, p, None) == PWN_EINVAL
    assert lib.pwn_trace_reach(None, 0, None, None, None) == PWN_EINVAL


def test_library_holds_the_reach_kernels():
    """PWN_KM_HITS | PWN_KM_REACH with and without PWN_KM_HIDE x the three forms of the sphere lists -- six kernels, each COUNT x HAS_W,
    ORDER off, under trace_reach.hip's own name; pwn_trace_kernel's set carries the bit nowhere"""
    _lib()
    tab = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "tables.h")).read()
    assert re.search(r"\bPWN_KM_REACH = 16\b", tab) and re.search(r"\bPWN_KM_HIDE = 8\b", tab) and re.search(r"\bPWN_KM_HITS = 3\b", tab)
    blob = open(LIB, "rb").read()
    every = re.findall(rb"_Z22pwn_trace_reach_kernelILb([01])ELb([01])ELb([01])ELi([0-9])ELi([0-9]+)EEv16pwn_trace_params", blob)
    found = {(c, w, o, l, int(m)) for c, w, o, l, m in every}
    want = {(c, w, b"0", l, m) for c in (b"0", b"1") for w in (b"0", b"1") for l in (b"0", b"1", b"2") for m in (3 | 16, 3 | 8 | 16)}
    assert found == want, sorted(found)
    others = re.findall(rb"_Z(?:16pwn_trace_kernel|22pwn_trace_hide2_kernel)ILb[01]ELb[01]ELb[01]ELi[0-9]ELi([0-9]+)EEv16pwn_trace_params", blob)
    assert others and all(int(m) < 16 for m in others)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    obj = re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert "trace_reach.o" in obj and "pwn_reach.o" in obj
    assert re.search(r"^\$\(B\)/trace_reach\.o: HIPFLAGS \+= \$\(TRACE_EXTRA\)$", mk, re.M)
