"""The MXFP4-weight grouped GEMMs (csrc/ffn_gemm_mx4.hip) without a GPU: what ffn_form answers for an MXFP4 stage of an engine that has
switched them on (moeinf_ffn_form's flags bit 3), that nothing of it leaks into the other dtypes or the default, the two new calls of
the C interface, the config switch, and the gfx950 ISA of every form the launcher can pick."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "moe-infinity_amd", "csrc")
SLOT_MXFP4 = 16
ROWS, HYB, LDS = 0, 1, 2
GEMM_ON = 8  # moeinf_ffn_form's flags bit 3
_KNOBS = [k for k in os.environ if k.startswith(("MOEINF_FFN_", "MOEINF_GEMM_", "MOEINF_RING"))]
# Mixtral-8x7B's two stages: (epilogue, K, R)
STAGES = ((4, 4096, 14336), (0, 14336, 4096))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from moe_infinity_amd import load_library

    return load_library()


@pytest.fixture()
def no_knobs(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k)


def _form(lib, dt, epi, K, R, rows, flags, active=8, K_sh=0):
    out = (C.c_int32 * 14)()
    assert lib.moeinf_ffn_form(dt, epi, K, K_sh, R, active, rows, 256, flags, out) == 0
    return list(out)


# ---- selection ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 16])
def test_up_to_sixteen_rows_the_switch_changes_nothing(lib, no_knobs, rows):
    for epi, K, R in STAGES:
        f = _form(lib, SLOT_MXFP4, epi, K, R, rows, GEMM_ON)
        assert f[0] == ROWS and f == _form(lib, SLOT_MXFP4, epi, K, R, rows, 0), (rows, f)


@pytest.mark.parametrize("rows", [17, 128])
def test_seventeen_to_128_rows_take_the_hybrid(lib, no_knobs, rows):
    for epi, K, R in STAGES:
        f = _form(lib, SLOT_MXFP4, epi, K, R, rows, GEMM_ON)
        # (kernel, waves, unroll, nt, rw, kk, xl, rgb, passes, ring2 x 5): gated one row group per wave, plain two; one code tile =
        # four activation k-tiles per stage; full-line staging
        assert f == [HYB, 4, 0, 0, 1 if epi == 4 else 2, 4, 1, 0, 0, 0, 0, 0, 0, 0], (rows, epi, f)


@pytest.mark.parametrize("rows", [129, 200, 341, 4096])
def test_above_128_rows_the_lds_form_and_never_ring2_or_big(lib, no_knobs, rows):
    for epi, K, R in STAGES:
        f = _form(lib, SLOT_MXFP4, epi, K, R, rows, GEMM_ON)
        # 8 waves above 128 rows; 64-row blocks (gated: always; plain: 256 row blocks x 8 experts < 512 workgroups of 128 rows)
        assert f == [LDS, 8, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0], (rows, epi, f)


def test_with_65_active_experts_the_hybrid_stops_at_64_rows(lib, no_knobs):
    # DeepSeek-V2-Lite stage 1: K 2048, R 2816, the shared expert (K_sh 2048) in the launch
    f = _form(lib, SLOT_MXFP4, 4, 2048, 2816, 64, GEMM_ON, active=65, K_sh=2048)
    assert f[:7] == [HYB, 4, 0, 0, 1, 4, 1], f
    f = _form(lib, SLOT_MXFP4, 4, 2048, 2816, 65, GEMM_ON, active=65, K_sh=2048)
    assert f[:8] == [LDS, 4, 0, 0, 0, 0, 1, 4], f


def test_the_row_kernel_is_kept_where_the_gemms_do_not_apply(lib, no_knobs):
    for epi, K, R in STAGES:
        # the stage fuses the combine
        f = _form(lib, SLOT_MXFP4, epi, K, R, 400, GEMM_ON | 4)
        assert f[0] == ROWS and f == _form(lib, SLOT_MXFP4, epi, K, R, 400, 4), f
    # a shared expert whose reduction is not whole 128-byte lines
    f = _form(lib, SLOT_MXFP4, 4, 2048, 2816, 400, GEMM_ON, active=65, K_sh=2048 + 32)
    assert f[0] == ROWS and f[3] == 4, f


def test_no_kernel_is_kept(lib, no_knobs):
    assert _form(lib, SLOT_MXFP4, 4, 4096 + 64, 14336, 200, GEMM_ON)[0] == -1
    assert _form(lib, SLOT_MXFP4, 3, 4096, 14336, 200, GEMM_ON)[0] == -1


def test_knobs_of_the_other_forms_do_not_reach_past_what_is_built(lib, monkeypatch, no_knobs):
    monkeypatch.setenv("MOEINF_GEMM_XL", "0")
    monkeypatch.setenv("MOEINF_GEMM_HYB_KK", "2")
    monkeypatch.setenv("MOEINF_FFN_GEMM_RGB2", "8")
    assert _form(lib, SLOT_MXFP4, 4, 4096, 14336, 100, GEMM_ON)[:7] == [HYB, 4, 0, 0, 1, 4, 1]
    assert _form(lib, SLOT_MXFP4, 4, 4096, 14336, 200, GEMM_ON)[:8] == [LDS, 8, 0, 0, 0, 0, 1, 4]
    monkeypatch.setenv("MOEINF_FFN_GEMM", "0")
    assert _form(lib, SLOT_MXFP4, 4, 4096, 14336, 200, GEMM_ON)[0] == ROWS
    monkeypatch.delenv("MOEINF_FFN_GEMM")
    monkeypatch.setenv("MOEINF_FFN_NT", "4")  # forced GEMMs: still the row kernel up to 16 rows
    assert _form(lib, SLOT_MXFP4, 4, 4096, 14336, 16, GEMM_ON)[0] == ROWS


@pytest.mark.parametrize("dt", [0, 3])
def test_the_bit_is_read_for_mxfp4_only(lib, no_knobs, dt):
    """(passes without the feature too: pins that nothing leaks into bf16 and fp8 slots)"""
    for epi, K, R in STAGES:
        for rows in (1, 16, 17, 128, 129, 200, 341, 4096):
            assert _form(lib, dt, epi, K, R, rows, GEMM_ON) == _form(lib, dt, epi, K, R, rows, 0), (dt, epi, rows)


# ---- the C interface and the config ------------------------------------------------------------------------
def test_header_library_and_prototypes_agree(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moeinf.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+moeinf_set_mxfp4_gemm\s*\(\s*moeinf_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+moeinf_last_ffn_forms\s*\(\s*const\s+moeinf_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\[2\]\s*\)\s*;", hdr)
    from moe_infinity_amd import _lib

    for name in ("moeinf_set_mxfp4_gemm", "moeinf_last_ffn_forms"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    out = (C.c_int32 * 2)()
    assert lib.moeinf_set_mxfp4_gemm(None, 1) == 1  # MOEINF_ERR_INVALID
    assert lib.moeinf_last_ffn_forms(None, out) == 1


def test_config_takes_the_switch_with_mxfp4_slots_only():
    from moe_infinity_amd import config as Cf

    base = dict(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2, router_kind=Cf.ROUTER_MIXTRAL)
    with pytest.raises(ValueError):
        Cf.EngineConfig(mxfp4_gemm=True, **base)
    with pytest.raises(ValueError):
        Cf.EngineConfig(mxfp4_gemm=True, fp8_slots=True, dtype=Cf.DTYPE_F8E4M3, **base)
    assert Cf.EngineConfig(mxfp4_slots=True, **base).mxfp4_gemm is False
    assert Cf.EngineConfig(mxfp4_slots=True, mxfp4_gemm=True, **base).mxfp4_gemm is True


# ---- ISA ----------------------------------------------------------------------------------------------------
def _compile(tmp, src):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp / (src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)],
                   check=True, capture_output=True, timeout=1200)
    return open(out).read()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("isa"), "ffn_gemm_mx4.hip")


@pytest.fixture(scope="module")
def asm_bf16(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("isa_bf16"), "ffn_gemm.hip")


def _kernels(text, family, tag):
    """template arguments -> (instruction lines, kernel descriptor text) for every instantiation of `family` whose first template
    argument is `tag` (NS_6mx4w_tE: mx4w_t, t: uint16_t = bf16)"""
    lines = text.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN6moeinf\d+%sI%sLi(\d+)ELi(\d+)ELi(\d+)ELb(\d)EEEvNS_8FfnStageE):" % (family, tag), l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))  # (the whole function: it has several s_endpgm)
            code = [x.strip() for x in lines[i:end] if x.strip() and not x.strip().startswith((";", "."))]
            desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, re.S).group(1)
            out[tuple(int(v) for v in m.groups()[1:])] = (code, desc)
    return out


# what launch_ffn_gemm_mx4 can pick, as (NMAT, RW | RGB, KK | NWV, XL): the hybrid for the gated (one row group per wave) and the
# plain stage (two), KK 4; the LDS-staged kernel gated with 4 row groups per workgroup, plain with 4 or 8, each with 4 or 8 waves; all
# with full-line staging — eight kernels
FORMS = {"ffn_gemm_hyb_kernel": {(2, 1, 4, 1), (1, 2, 4, 1)},
         "ffn_gemm_lds_kernel": {(2, 4, 4, 1), (2, 4, 8, 1), (1, 4, 4, 1), (1, 4, 8, 1), (1, 8, 4, 1), (1, 8, 8, 1)}}


def _lds_bytes(desc):
    return int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))


@pytest.mark.parametrize("family", sorted(FORMS))
def test_every_mxfp4_gemm_form_is_built_upcasts_in_registers_and_fits_the_bf16_forms_lds(asm, asm_bf16, family):
    ks = _kernels(asm, family, "NS_6mx4w_tE")
    assert set(ks) == FORMS[family] and len(ks) == len(FORMS[family]), sorted(ks)
    bf16 = _kernels(asm_bf16, family, "t")
    for args, (code, desc) in ks.items():
        name = f"{family}{args}"
        assert any(l.startswith("v_cvt_scalef32_pk_bf16_fp4") for l in code), f"{name}: no hardware fp4 -> bf16 conversion"
        assert any(l.startswith("v_mfma_f32_16x16x32_bf16") for l in code), f"{name}: no bf16 MFMA"
        assert not any("scratch_" in l for l in code), f"{name}: scratch (register spills)"
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), f"{name}: a private segment"
        assert not any(re.match(r"ds_read_(u8|u16|i8|i16)", l) for l in code), f"{name}: byte or short reads of LDS"
        assert not any(re.match(r"global_load_(u|s)(byte|short)", l) for l in code), f"{name}: byte or short loads"
        assert any(re.match(r"global_load_dword\s", l) for l in code), f"{name}: no 4-byte loads"
        if family == "ffn_gemm_hyb_kernel":
            # codes straight into registers, non-temporal (the scale dwords: the 4-byte loads above)
            assert any(l.startswith("global_load_dwordx4") and re.search(r"\bnt\b", l) for l in code), f"{name}: no non-temporal weight loads"
        else:
            # codes and activations through the 16-byte LDS DMA, the scale dwords through the 4-byte one
            assert any(l.startswith("global_load_lds_dwordx4") for l in code), name
            assert any(re.match(r"global_load_lds_dword\s", l) for l in code), f"{name}: no 4-byte scale loads"
        assert args in bf16, f"{name}: no bf16 form of the same template arguments to compare with"
        assert _lds_bytes(desc) <= _lds_bytes(bf16[args][1]), f"{name}: more static LDS than the bf16 form ({_lds_bytes(bf16[args][1])})"
