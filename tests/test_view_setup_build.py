"""The camera set-up kernel of pwn_trace_views_device restates the host's frame_setup, which runs with denormals kept: its file
alone is built without the denormal flush.  Cross-compiled with the Makefile's own command line (no GPU needed): the kernel's
descriptor asks for fp32 denormal mode 3, and its arithmetic is 20 separate multiplies and adds, none fused or packed."""
import os
import re
import shlex
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")


def _compile_line(obj):
    """what `make` would run to build csrc/build/<obj>"""
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, os.path.join(CSRC, "build", obj)], text=True)
    lines = [ln for ln in out.splitlines() if " -c " in ln and ln.rstrip().endswith(obj[:-2] + ".hip")]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def test_only_the_setup_kernel_keeps_denormals():
    vs = _compile_line("view_setup.o")
    assert "-fno-gpu-flush-denormals-to-zero" in vs and "-fgpu-flush-denormals-to-zero" not in vs
    assert "-ffp-contract=off" in vs
    for obj in ("trace_kernel.o", "trace_refill.o", "post_kernels.o"):
        cmd = _compile_line(obj)
        assert "-fgpu-flush-denormals-to-zero" in cmd and "-fno-gpu-flush-denormals-to-zero" not in cmd, obj
        assert [a for a in cmd if a.startswith("-f")] == [a.replace("-fno-gpu-flush", "-fgpu-flush") for a in vs if a.startswith("-f")], obj


def test_setup_kernel_isa(tmp_path):
    cmd = _compile_line("view_setup.o")
    i = cmd.index("-o")
    asm = str(tmp_path / "view_setup.s")
    cmd = cmd[:i] + cmd[i + 2:]
    cmd.remove("-c")
    subprocess.check_call(cmd[:-1] + ["--cuda-device-only", "-S", "-o", asm, cmd[-1]])
    text = open(asm).read()
    # (the file has one kernel: its code up to its descriptor, then the descriptor)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)) == 1
    sym = re.search(r"^\s*\.amdhsa_kernel\s+(\S*pwn_view_setup_kernel\S*)", text, flags=re.M).group(1)
    body = text[text.index(sym + ":"):text.index(".amdhsa_kernel")]
    desc = text[text.index(".amdhsa_kernel"):text.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_float_denorm_mode_32\s+3\b", desc), desc
    ops = re.findall(r"^\s+(v_[a-z0-9_]+)", body, flags=re.M)
    assert sum(op in ("v_mul_f32_e32", "v_mul_f32_e64", "v_add_f32_e32", "v_add_f32_e64") for op in ops) == 20, ops
    # (no fused or packed floating-point operation; integer multiply-adds of the address arithmetic are no concern)
    assert not [op for op in ops if re.match(r"v_(fma|fmac|mac|mad|pk_\w+?)_(legacy_)?(f16|f32|f64|mix)", op) or op.startswith(("v_fma_mix", "v_mad_mix"))], ops
