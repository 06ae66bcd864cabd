"""trace_reach.hip cross-compiles for gfx950 with the Makefile's own command line (no GPU needed): the code object holds the six REACH
kernels -- PWN_KM_HITS | PWN_KM_REACH with and without PWN_KM_HIDE, the three list forms -- each in its four COUNT x HAS_W variants and
nothing else, the twelve that do not count use no scratch memory, and the twelve that count stay under the worst counting trace kernel.  (The counting variants are the diagnosis build: at the 96-VGPR
budget every counting trace kernel spills, profiles/reach/isa_resources.txt.)"""
import os
import re
import shlex
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
# The counting variants (PWN_OPT_COUNTERS, the diagnosis build) spill like every counting trace kernel at the 96-VGPR budget.  Their bound
# is the most that a counting trace kernel of the project spilled before there were REACH kernels: 684 B a lane, the 4-lane PWN_KM_FRAME
# kernel on lists in device memory (profiles/hide/isa_resources.txt, profiles/reach/isa_resources.txt).  A REACH kernel is a PWN_KM_HITS
# kernel -- set-up, one walk, a record, none of the frame kernel's shading, bounces and composite stack -- with ten more values kept
# across the step, so it has no reason to need more scratch than the frame kernel does; growth beyond that is caught here.
COUNTING_SCRATCH_MAX = 684


def _compile_line(obj):
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, os.path.join(CSRC, "build", obj)], text=True)
    lines = [ln for ln in out.splitlines() if " -c " in ln and ln.rstrip().endswith(obj[:-2] + ".hip")]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def test_reach_unit_has_the_trace_kernels_flags():
    cmd = _compile_line("trace_reach.o")
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd and "-fgpu-flush-denormals-to-zero" in cmd
    assert [a for a in cmd if a.startswith(("-f", "-m", "-D", "-O")) or a == "-disable-lsr"] == \
           [a for a in _compile_line("trace_hide.o") if a.startswith(("-f", "-m", "-D", "-O")) or a == "-disable-lsr"]
    assert "-disable-lsr" in cmd


def test_reach_kernels_isa(tmp_path):
    cmd = _compile_line("trace_reach.o")
    i = cmd.index("-o")
    asm = str(tmp_path / "trace_reach.s")
    cmd = cmd[:i] + cmd[i + 2:]
    cmd.remove("-c")
    subprocess.check_call(cmd[:-1] + ["--cuda-device-only", "-S", "-o", asm, cmd[-1]])
    text = open(asm).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    want = {"_Z22pwn_trace_reach_kernelILb%dELb%dELb0ELi%dELi%dEEv16pwn_trace_params" % (c, w, l, m)
            for c in (0, 1) for w in (0, 1) for l in (0, 1, 2) for m in (19, 27)}
    assert set(syms) == want and len(syms) == 24, sorted(set(syms) ^ want)
    for sym in syms:
        d0 = text.index(".amdhsa_kernel " + sym)
        desc = text[d0:text.index(".end_amdhsa_kernel", d0)]
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        assert re.search(r"\.amdhsa_float_denorm_mode_32\s+0\b", desc), sym
        assert vgprs <= 96, (sym, vgprs)
        if "ILb0E" in sym[:32]:
            assert scratch == 0, (sym, scratch)
        else:
            assert scratch <= COUNTING_SCRATCH_MAX, (sym, scratch)
