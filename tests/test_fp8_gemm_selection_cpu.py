"""Which grouped GEMM an FFN stage of an fp8-slot engine takes (csrc/kernels.h f8_gemm_form, exported as moeinf_ffn_f8_gemm_form;
DESIGN.md section 4.3): the bf16 thresholds without the 256 x 256 kernel, which has no fp8 form.  Pinned with the row estimate the
engine itself passes on the sync-free path.  No GPU needed."""
import ctypes as C

import pytest

from moe_infinity_amd import load_library

ROWS, HYB, LDS, RING2 = 0, 1, 2, 3
MIX = dict(H=4096, F=14336, E=8, K=2)
DSL = dict(H=2048, F=1408, Fs=2816, E=64, K=6)


def form(nmat, K, R, active, max_rows, K_sh=0, cus=256):
    out = (C.c_int32 * 6)()
    assert load_library().moeinf_ffn_f8_gemm_form(nmat, K, K_sh, R, active, max_rows, cus, out) == 0
    return tuple(out)  # (kernel, waves | token groups, split tail, row blocks per expert, first split unit, workgroups)


def est(T, m):
    e = load_library().moeinf_rows_estimate(T, m["K"], m["E"])
    assert e == min(T, (T * m["K"] * 3) // (2 * m["E"]) + 1)
    return e


def mixtral(T):
    """(gate/up stage, down stage) of a Mixtral-8x7B layer at T tokens on the sync-free path"""
    r, act = est(T, MIX), min(MIX["E"], T * MIX["K"])
    return form(2, MIX["H"], MIX["F"], act, r), form(1, MIX["F"], MIX["H"], act, r)


def deepseek(T):
    """DeepSeek-V2-Lite: the hidden shared expert rides in the launch (one more active slot, its own K and R)"""
    r, act = est(T, DSL), min(DSL["E"], T * DSL["K"]) + 1
    return (form(2, DSL["H"], max(DSL["F"], DSL["Fs"]), act, r, K_sh=DSL["H"]),
            form(1, DSL["F"], DSL["H"], act, r, K_sh=DSL["Fs"]))


def test_the_export_is_declared_and_checks_its_arguments():
    lib = load_library()
    from moe_infinity_amd._lib import PROTOTYPES

    assert "moeinf_ffn_f8_gemm_form" in PROTOTYPES
    out = (C.c_int32 * 6)()
    assert lib.moeinf_ffn_f8_gemm_form(3, 4096, 0, 4096, 8, 100, 256, out) == 1  # MOEINF_ERR_INVALID
    assert lib.moeinf_ffn_f8_gemm_form(1, 4096, 0, 4096, 8, 100, 256, None) == 1


def test_mixtral_48_tokens_hybrid_gate_up_ring_down():
    assert est(48, MIX) == 19
    g, p = mixtral(48)
    assert g[:2] == (HYB, 4)
    assert p == (RING2, 8, 0, 32, 0, 256)


def test_mixtral_512_tokens_ring2_192_tokens_per_pass_with_a_split_tail():
    assert est(512, MIX) == 193
    g, p = mixtral(512)
    assert g == (RING2, 12, 1, 112, 768, 1024)  # 896 units = 3.5 rounds of 256 CUs: the last 128 go out as half workgroups
    assert p == (RING2, 12, 0, 32, 0, 256)


def test_mixtral_long_prefills():
    assert est(896, MIX) == 337
    g, p = mixtral(896)
    assert g[:2] == (RING2, 16) and p[:2] == (RING2, 16)
    assert est(1024, MIX) == 385
    g, p = mixtral(1024)  # past ring2's 340 rows; no fp8 form of the 256 x 256 kernel: the LDS kernel, 256 tokens per pass
    assert g == (LDS, 8, 0, 0, 0, 0) and p == (LDS, 8, 0, 0, 0, 0)
    g, p = mixtral(4096)
    assert g[:2] == (LDS, 8) and p[:2] == (LDS, 8)


def test_deepseek_v2_lite():
    assert est(512, DSL) == 73
    g, p = deepseek(512)  # 73 rows, 65 active slots (> 16: the hybrid kernel stops at 64), K = 2048 < 4096: no ring
    assert g[:2] == (LDS, 4) and p[:2] == (LDS, 4)
    assert est(160, DSL) == 23
    g, p = deepseek(160)
    assert g[:2] == (HYB, 4) and p[:2] == (HYB, 4)
    g, p = deepseek(2048)
    assert g[:2] == (LDS, 8) and p[:2] == (LDS, 8)


def test_up_to_16_rows_the_row_kernel():
    for T in (1, 4, 8):
        assert mixtral(T) == ((ROWS,) + (0,) * 5,) * 2
    assert form(2, 4096, 14336, 8, 16)[0] == ROWS
    assert form(2, 4096, 14336, 8, 17)[0] == HYB
    assert form(1, 14336, 4096, 8, 17)[0] == RING2


def test_a_shared_expert_in_the_launch_keeps_ring2_out():
    """ring2's fp8 form takes routed experts only (the shared expert's weights are bf16): a long reduction with a shared expert
    takes the hybrid / LDS kernels, whose workgroups for the shared expert run the bf16 body"""
    assert form(2, 5120, 12288, 161, 200)[0] == RING2
    assert form(2, 5120, 12288, 161, 200, K_sh=5120)[:2] == (LDS, 8)
    assert form(1, 12288, 5120, 161, 40, K_sh=3072)[:2] == (HYB, 4)


def test_environment_knobs_are_honoured(monkeypatch):
    monkeypatch.setenv("MOEINF_GEMM_RING2", "2")  # plain stage only
    g, p = mixtral(512)
    assert g[:2] == (LDS, 8) and p[:2] == (RING2, 12)
    monkeypatch.setenv("MOEINF_GEMM_RING2", "3")
    monkeypatch.setenv("MOEINF_RING_MIN_K", "8192")  # gate/up's K = 4096 no longer counts as long
    g, p = mixtral(512)
    assert g[:2] == (LDS, 8) and p[:2] == (RING2, 12)
    monkeypatch.delenv("MOEINF_RING_MIN_K")
    monkeypatch.setenv("MOEINF_GEMM_HYB_ROWS", "256")  # the hybrid kernel up to 256 rows: gate/up at 512 tokens stays hybrid
    g, p = mixtral(512)
    assert g[:2] == (HYB, 4) and p[:2] == (RING2, 12)
    monkeypatch.delenv("MOEINF_GEMM_HYB_ROWS")
    monkeypatch.setenv("MOEINF_RING2_TAIL", "0")
    assert mixtral(512)[0] == (RING2, 12, 0, 112, 0, 896)
    monkeypatch.delenv("MOEINF_RING2_TAIL")
    monkeypatch.setenv("MOEINF_RING2_MAX_ROWS", "256")
    assert mixtral(896)[0][:2] == (LDS, 8)
    monkeypatch.delenv("MOEINF_RING2_MAX_ROWS")
    monkeypatch.setenv("MOEINF_GEMM_WIDE", "0")
    assert mixtral(1024)[0][:2] == (LDS, 4)
    monkeypatch.delenv("MOEINF_GEMM_WIDE")
    monkeypatch.setenv("MOEINF_FFN_GEMM", "0")  # as for bf16: the row kernel's four-token-tile form
    assert mixtral(512)[0][0] == ROWS
    monkeypatch.setenv("MOEINF_FFN_GEMM", "3")  # always the hybrid kernel
    assert mixtral(1024) == ((HYB, 4, 0, 0, 0, 0),) * 2
