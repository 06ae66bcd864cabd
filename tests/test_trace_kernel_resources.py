"""The units kernel holds the segment's text once per bounce depth (trace_segment.inc), which doubles its code and tempts the
compiler to keep values alive across the copies.  Every instantiation that is not a counting one must still fit the budget of five
waves per SIMD without scratch memory: at most 96 VGPRs, 0 bytes of scratch, occupancy 5 or more.  trace_kernel.hip is cross-compiled
once with the Makefile's own command line (no GPU needed) and -Rpass-analysis=kernel-resource-usage; the compiler's remarks are read."""
import os
import re
import shlex
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")


def _compile_line(obj):
    """what `make` would run to build csrc/build/<obj>"""
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, os.path.join(CSRC, "build", obj)], text=True)
    lines = [ln for ln in out.splitlines() if " -c " in ln and ln.rstrip().endswith(obj[:-2] + ".hip")]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


@pytest.fixture(scope="module")
def usage():
    """{mangled kernel name: {"vgprs", "scratch", "occupancy"}} of trace_kernel.hip as the Makefile builds it"""
    cmd = _compile_line("trace_kernel.o")
    assert "-DPWN_MIN_WAVES=5" in cmd and "-disable-lsr" in cmd, cmd
    i = cmd.index("-o")
    cmd = cmd[:i] + cmd[i + 2:]
    res = subprocess.run(cmd[:-1] + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, cmd[-1]],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    kernels, cur = {}, None
    for ln in res.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return kernels


def _is_counting(name):
    # pwn_trace_kernel<COUNT, HAS_W, ORDER, LISTS, MODE>: the first template argument, Lb1E = true
    m = re.match(r"_Z\d+pwn_trace_kernelILb([01])E", name)
    assert m, name
    return m.group(1) == "1"


def test_every_instantiation_is_reported(usage):
    names = [n for n in usage if "pwn_trace_kernel" in n]
    # 8 frame kernels with an order + 7 modes x 3 list forms x 2 x 2 without one (trace_kernel.hip pwn_launch_trace)
    assert len(names) == 8 + 7 * 3 * 4, len(names)
    assert sum(not _is_counting(n) for n in names) == len(names) // 2
    for n in names:
        assert set(usage[n]) == {"vgprs", "scratch", "occupancy"}, (n, usage[n])


def test_no_scratch_and_five_waves_without_counters(usage):
    bad = {n: u for n, u in usage.items() if "pwn_trace_kernel" in n and not _is_counting(n)
           and (u["vgprs"] > 96 or u["scratch"] != 0 or u["occupancy"] < 5)}
    assert not bad, bad
