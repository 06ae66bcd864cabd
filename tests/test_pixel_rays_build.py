"""The ray kernel of pwn_pixel_rays_device restates the second half of the host's pwn_pixel_rays, which runs under FTZ|DAZ and rounds
every product and sum by itself: its file is built by the Makefile's general rule, with the denormal flush and without contraction
(the half that keeps denormals is view_setup.hip's, tests/test_view_setup_build.py).  Cross-compiled with the Makefile's own command
line (no GPU needed): the kernel's descriptor asks for fp32 denormal mode 0, and its arithmetic is separate multiplies and adds,
none fused or packed."""
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


def test_ray_kernel_is_built_with_the_flush_and_without_contraction():
    cmd = _compile_line("pixel_rays.o")
    assert "-fgpu-flush-denormals-to-zero" in cmd and "-fno-gpu-flush-denormals-to-zero" not in cmd
    assert "-ffp-contract=off" in cmd
    assert "-disable-lsr" not in cmd          # (the trace kernel's own extra)
    # the flags of the other flushed files, to the letter
    assert [a for a in cmd if a.startswith("-f")] == [a for a in _compile_line("post_kernels.o") if a.startswith("-f")]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pixel_rays.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0)
    assert not re.search(r"^\$\(B\)/pixel_rays\.o:", mk, re.M), "pixel_rays.o has a rule of its own"


def test_ray_kernel_isa(tmp_path):
    cmd = _compile_line("pixel_rays.o")
    i = cmd.index("-o")
    asm = str(tmp_path / "pixel_rays.s")
    cmd = cmd[:i] + cmd[i + 2:]
    cmd.remove("-c")
    subprocess.check_call(cmd[:-1] + ["--cuda-device-only", "-S", "-o", asm, cmd[-1]])
    text = open(asm).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(syms) == 1 and "pwn_pixel_rays_kernel" in syms[0], syms
    for sym in syms:
        start = text.index(sym + ":")
        body = text[start:text.index("s_endpgm", start)]
        d0 = text.index(".amdhsa_kernel " + sym)
        desc = text[d0:text.index(".end_amdhsa_kernel", d0)]
        assert re.search(r"\.amdhsa_float_denorm_mode_32\s+0\b", desc), desc
        ops = re.findall(r"^\s+([vs]_[a-z0-9_]+)", body, flags=re.M)
        fp = [op for op in ops if re.match(r"v_(mul|add)_f32", op)]
        # four lanes of (cx0 * rdx + rayb) + y * rdy, and the four adds of the chain's loop
        assert sum(op.startswith("v_mul_f32") for op in fp) == 8 and sum(op.startswith("v_add_f32") for op in fp) >= 12, fp
        # (no fused or packed floating-point operation; integer multiply-adds of the address arithmetic are no concern)
        assert not [op for op in ops if re.match(r"v_(fma|fmac|mac|mad|pk_\w+?)_(legacy_)?(f16|f32|f64|mix)", op) or op.startswith(("v_fma_mix", "v_mad_mix"))], ops
        # the record of a wave whose rays share a camera comes by scalar loads; the record goes out in 16-byte stores
        assert any(op.startswith("s_load_dwordx") for op in ops), ops
        assert sum(op == "global_store_dwordx4" for op in re.findall(r"^\s+(global_store_[a-z0-9_]+)", body, flags=re.M)) == 2
        # no integer division per lane: the ray's camera and the pixel's row come by multiply-high
        assert any(op.startswith("v_mul_hi_u32") for op in ops), ops
        assert not [op for op in ops if op.startswith(("v_rcp_", "v_div_"))], ops
