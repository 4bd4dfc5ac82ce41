"""The gfx950 ISA of the fp8-weight grouped GEMMs (csrc/ffn_gemm_f8.hip): every form the launcher can pick is in the code object,
up-casts with the hardware conversion in registers, multiplies on the bf16 matrix instruction, spills nothing, and the forms that
stream weights into registers (hybrid, register ring) do it with non-temporal 16-byte loads.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "moe-infinity_amd", "csrc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "ffn_gemm_f8.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(CSRC, "ffn_gemm_f8.hip")], check=True, capture_output=True, timeout=1200)
    return open(out).read()


def _kernels(text, family):
    """mangled name -> (instruction lines, kernel descriptor text) for every f8w_t instantiation of `family`"""
    lines = text.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN6moeinf\d+%sINS_5f8w_t\S*):" % family, l)
        if m:
            end = next(j for j in range(i, len(lines)) if "s_endpgm" in lines[j])
            code = [x.strip() for x in lines[i:end] if x.strip() and not x.strip().startswith((";", "."))]
            desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, re.S).group(1)
            out[m.group(1)] = (code, desc)
    return out


# (family, forms): hybrid — 2 stages x KK 2/4 x full-line staging on/off; LDS-staged — 2 stages x 4/8 waves x 64/128-row blocks x
# staging; register ring — gated 128/192/256 tokens per pass with and without the split tail, plain 128/192/256
FORMS = {"ffn_gemm_hyb_kernel": 8, "ffn_gemm_lds_kernel": 16, "ffn_gemm_ring2_kernel": 9}


@pytest.mark.parametrize("family", sorted(FORMS))
def test_every_fp8_form_is_built_and_upcasts_in_registers(asm, family):
    ks = _kernels(asm, family)
    assert len(ks) == FORMS[family], sorted(ks)
    for name, (code, desc) in ks.items():
        assert any(l.startswith("v_cvt_scalef32_pk_bf16_fp8") for l in code), f"{name}: no hardware fp8 -> bf16 conversion"
        assert any(l.startswith("v_mfma_f32_16x16x32_bf16") for l in code), f"{name}: no bf16 MFMA"
        assert not any("scratch_" in l for l in code), f"{name}: scratch (register spills)"
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), f"{name}: a private segment"
        assert not any(re.match(r"ds_read_(u8|u16|i8|i16)", l) for l in code), f"{name}: an LDS look-up table"
        if family == "ffn_gemm_lds_kernel":  # both operands through the LDS DMA
            assert any(l.startswith("global_load_lds_dwordx4") for l in code), name
        else:  # weights straight into registers, non-temporal
            assert any(l.startswith("global_load_dwordx4") and re.search(r"\bnt\b", l) for l in code), f"{name}: no non-temporal weight loads"


def test_both_stage_kinds_and_the_split_tail_are_there(asm):
    ring = _kernels(asm, "ffn_gemm_ring2_kernel")
    # ffn_gemm_ring2_kernel<f8w_t, NMAT, NTB, D, TAIL>
    got = {tuple(int(v) for v in re.search(r"f8w_tELi(\d+)ELi(\d+)ELi\d+ELb(\d)", n).groups()) for n in ring}
    assert got == {(2, ntb, t) for ntb in (8, 12, 16) for t in (0, 1)} | {(1, ntb, 0) for ntb in (8, 12, 16)}
