"""Which kernel, and which form of it, an FFN stage takes for bf16, fp16 and fp32 — one function decides (csrc/kernels.h ffn_form;
DESIGN.md section 4.3), exported as moeinf_ffn_form.  Until it existed this choice lived in the launchers' control flow and no
test could reach it without a GPU.  tests/golden/ffn_forms.json holds 808 stages — Mixtral-8x7B, DeepSeek-V2-Lite (shared expert
in the launch), NLLB-MoE-54B and Switch-base-8 (fp32) at the engine's own row estimate, the row thresholds, the declines and the
knob overrides — with the form the launchers ran before ffn_form, recorded from their launches (kernel instantiation, grid and
block) on the CPU.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

from moe_infinity_amd import load_library

BF16, F32, F16 = 0, 1, 2
NONE, BIAS, RELU, BIAS_RELU, SILU, GELU = range(6)
ROWS, HYB, LDS, RING2, GEMM, BIG = range(6)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ffn_forms.json")


def form(dtype, epi, K, R, active, max_rows, K_sh=0, flags=0, cus=256):
    """(kernel, waves, unroll, token groups, row groups per wave, k-tiles per stage, xl, row groups per workgroup, big passes,
    ring2: token groups, split tail, row blocks, first split unit, workgroups)"""
    out = (C.c_int32 * 14)()
    assert load_library().moeinf_ffn_form(dtype, epi, K, K_sh, R, active, max_rows, cus, flags, out) == 0
    return tuple(out)


def est(T, k, e):
    r = load_library().moeinf_rows_estimate(T, k, e)
    assert r == min(T, (T * k * 3) // (2 * e) + 1)
    return r


def _cases():
    with open(GOLDEN) as f:
        data = json.load(f)
    by_env = {}
    for case, want in data:
        by_env.setdefault(case[0], []).append((case[1:], tuple(want)))
    return sorted(by_env.items())


@pytest.mark.parametrize("env,cases", _cases(), ids=lambda v: (v or "default") if isinstance(v, str) else "")
def test_the_recorded_forms(monkeypatch, env, cases):
    for k in [k for k in os.environ if k.startswith("MOEINF_")]:
        monkeypatch.delenv(k)
    if env:
        k, v = env.split("=")
        monkeypatch.setenv(k, v)
    for (label, dt, epi, K, K_sh, R, active, rows, flags), want in cases:
        assert form(dt, epi, K, R, active, rows, K_sh=K_sh, flags=flags) == want, (env, label, dt, epi, K, K_sh, R, active, rows, flags)


def test_the_export_is_declared_and_checks_its_arguments():
    from moe_infinity_amd._lib import PROTOTYPES

    assert "moeinf_ffn_form" in PROTOTYPES
    out = (C.c_int32 * 14)()
    lib = load_library()
    assert lib.moeinf_ffn_form(BF16, 6, 4096, 0, 4096, 8, 100, 256, 0, out) == 1  # MOEINF_ERR_INVALID: no such epilogue
    assert lib.moeinf_ffn_form(BF16, NONE, 4096, 0, 4096, 8, 100, 256, 0, None) == 1


def test_mixtral_prefill():
    r = est(512, 2, 8)
    assert form(BF16, SILU, 4096, 14336, 8, r) == (RING2, 0, 0, 0, 0, 0, 0, 0, 0, 12, 1, 112, 768, 1024)
    assert form(BF16, SILU, 4096, 14336, 8, est(48, 2, 8))[:7] == (HYB, 4, 0, 0, 1, 4, 1)  # 19 rows: hybrid up to 128 (<= 16 active)
    assert form(BF16, NONE, 14336, 4096, 8, est(4096, 2, 8))[:9] == (BIG, 0, 0, 0, 0, 0, 0, 0, 7)  # 1537 rows: seven passes
    assert form(F16, SILU, 4096, 14336, 8, 64)[0] == HYB  # fp16: the ring takes the gated stage from 65 rows, before the hybrid's 128
    assert form(F16, SILU, 4096, 14336, 8, 65)[9] == 8
    assert form(BF16, SILU, 4096, 14336, 8, 16)[:4] == (ROWS, 4, 4, 1)  # decode: the row kernel, one token tile


def test_deepseek_and_nllb():
    a = min(64, 512 * 6) + 1
    assert form(BF16, SILU, 2048, 2816, a, est(512, 6, 64), K_sh=2048)[:8] == (LDS, 4, 0, 0, 0, 0, 1, 4)
    assert form(BF16, BIAS, 8192, 2048, 128, est(2048, 2, 128))[0] == RING2  # 49 rows, K = 8192
    assert form(BF16, BIAS_RELU, 2048, 8192, 128, est(2048, 2, 128))[:7] == (HYB, 4, 0, 0, 2, 4, 1)


def test_switch_fp32_has_neither_ring_nor_big_kernel():
    assert est(512, 1, 8) == 97 and est(4096, 1, 8) == 769
    assert form(F32, RELU, 768, 3072, 8, 97)[:7] == (HYB, 4, 0, 0, 2, 4, 1)
    assert form(F32, NONE, 3072, 768, 8, 769)[:8] == (LDS, 8, 0, 0, 0, 0, 1, 4)


def test_declines():
    assert form(BF16, GELU, 4096, 14336, 8, 400)[:4] == (ROWS, 4, 0, 4)           # gelu gate: the row kernel at every size
    assert form(BF16, SILU, 4096 + 16, 14336, 8, 193)[:4] == (GEMM, 4, 0, 4)       # K off the k-tile: the register GEMM
    assert form(BF16, NONE, 14336, 4096, 8, 400, flags=1)[0] == LDS                # ld_out % 8: no 256 x 256 kernel
    assert form(BF16, SILU, 4096, 14336, 8, 193, flags=2)[0] == LDS                # rows_bound * ld_in past 32 bits: no ring
    assert form(BF16, NONE, 14336, 4096, 8, 400, flags=4)[:4] == (ROWS, 8, 4, 1)  # the fused combine: the row kernel


def test_fp8_stages_the_kernels_do_not_take():
    F8 = 3
    assert form(F8, GELU, 4096, 14336, 8, 100)[0] == -1
    assert form(F8, BIAS, 8192, 2048, 8, 100)[0] == -1
    assert form(F8, SILU, 4096 + 32, 14336, 8, 100)[0] == -1
    assert form(F8, SILU, 4096, 14336, 8, 400)[:2] == (LDS, 8)  # no fp8 256 x 256 kernel
