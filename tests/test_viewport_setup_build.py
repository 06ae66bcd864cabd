"""The set-up kernel of pwn_trace_viewports_device restates the host's frame_setup for a view of its own size, which runs with
denormals kept: its file is built as view_setup.hip is, without the denormal flush and without contraction.  Cross-compiled with
the Makefile's own command line (no GPU needed): the kernel's descriptor asks for fp32 denormal mode 3, and its arithmetic is 20
separate multiplies and adds, none fused or packed."""
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


def test_the_viewport_setup_file_is_built_as_view_setup_is():
    vp = _compile_line("viewport_setup.o")
    assert "-fno-gpu-flush-denormals-to-zero" in vp and "-fgpu-flush-denormals-to-zero" not in vp
    assert "-ffp-contract=off" in vp
    vs = _compile_line("view_setup.o")
    assert [a for a in vp if a.startswith(("-f", "-O", "-D", "--offload"))] == [a for a in vs if a.startswith(("-f", "-O", "-D", "--offload"))]
    # (and it is part of the library)
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC], text=True)
    link = [ln for ln in out.splitlines() if " -shared " in ln]
    assert len(link) == 1 and "build/viewport_setup.o" in link[0] and "build/pwn_viewports_device.o" in link[0]


def test_viewport_setup_kernel_isa(tmp_path):
    cmd = _compile_line("viewport_setup.o")
    i = cmd.index("-o")
    asm = str(tmp_path / "viewport_setup.s")
    cmd = cmd[:i] + cmd[i + 2:]
    cmd.remove("-c")
    subprocess.check_call(cmd[:-1] + ["--cuda-device-only", "-S", "-o", asm, cmd[-1]])
    text = open(asm).read()
    # (the file has one kernel: its code up to its descriptor, then the descriptor)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)) == 1
    sym = re.search(r"^\s*\.amdhsa_kernel\s+(\S*pwn_viewport_setup_kernel\S*)", text, flags=re.M).group(1)
    body = text[text.index(sym + ":"):text.index(".amdhsa_kernel")]
    desc = text[text.index(".amdhsa_kernel"):text.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_float_denorm_mode_32\s+3\b", desc), desc
    ops = re.findall(r"^\s+(v_[a-z0-9_]+)", body, flags=re.M)
    assert sum(op in ("v_mul_f32_e32", "v_mul_f32_e64", "v_add_f32_e32", "v_add_f32_e64") for op in ops) == 20, ops
    # (no fused or packed floating-point operation; integer multiply-adds of the address arithmetic are no concern)
    assert not [op for op in ops if re.match(r"v_(fma|fmac|mac|mad|pk_\w+?)_(legacy_)?(f16|f32|f64|mix)", op) or op.startswith(("v_fma_mix", "v_mad_mix"))], ops
    # (the records leave in whole 16-byte vector stores, eight a thread)
    stores = re.findall(r"^\s+(global_store_\w+|flat_store_\w+)", body, flags=re.M)
    assert stores and all(s.endswith("dwordx4") for s in stores) and len(stores) == 8, stores
