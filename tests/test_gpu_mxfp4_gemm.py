"""The MXFP4-weight grouped GEMMs (csrc/ffn_gemm_mx4.hip; EngineConfig.mxfp4_gemm, moeinf_set_mxfp4_gemm): prefill-sized stages of an
MXFP4-slot engine run the hybrid and the LDS-staged kernel on code tiles up-cast in registers.  Each case first asks the selection
export (moeinf_ffn_form with flags bit 3) which form the engine's row estimate picks, checks the layer against the oracle on the
dequantised weights, y = FFN(x; dequant(W).to(bf16)), routing exact, on the decision path (first forward, misses) and the sync-free
path (second), and then asks the engine which kernels the forward took (moeinf_last_ffn_forms) — so a switch that does nothing fails.
The weights hold every (code, scale byte) pair.  Needs an MI355X: -m gpu."""
import ctypes as C

import pytest
import torch

from helpers import R, acts, assert_block_close, assert_model_close, oracle_expert_rows, register_all
from moe_infinity_amd import load_library
from test_gpu_mxfp4_slots import _engine, _mx_weights, _routing_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOT_MXFP4 = 16
ROWS, HYB, LDS = 0, 1, 2


def _form(epi, K, Rr, active, rows, K_sh=0):
    out = (C.c_int32 * 14)()
    assert load_library().moeinf_ffn_form(SLOT_MXFP4, epi, K, K_sh, Rr, active, rows, 256, 8, out) == 0
    return (out[0], out[1])  # (kernel, waves)


def _forms(h, f, e, k, t, n_shared=0):
    """(stage 1, stage 2) as (kernel, waves) for the sync-free path's row estimate"""
    rows = load_library().moeinf_rows_estimate(t, k, e)
    fs = f * n_shared
    active = min(e, t * k) + (1 if n_shared else 0)
    return rows, _form(4, h, max(f, fs), active, rows, K_sh=h if n_shared else 0), _form(0, f, h, active, rows, K_sh=fs)


def _oracle(family, x, gate, deq, k, shared):
    if family == "mixtral":
        return R.block_mixtral(x[None], gate, deq, top_k=k)
    return R.block_deepseek(x[None], gate, deq, k, shared=shared)


def _run(family, h, f, e, k, t, seed, n_shared=0, x=None, gate=None, weights=None, want=None):
    gate0, packed, deq, shared = weights or _mx_weights(family, h, f, e, seed, n_shared)
    gate = gate0 if gate is None else gate
    x = acts(t, h, torch.bfloat16, seed + 2) if x is None else x
    eng = _engine(family, h, f, e, k, n_shared=n_shared, max_tokens=t, mxfp4_gemm=True)
    register_all(eng, packed, shared)
    ref = _oracle(family, x, gate, deq, k, shared)
    rows = oracle_expert_rows(ref, e)
    for rnd in range(2):  # misses (the decision path), then hits (the sync-free path)
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
        _routing_exact(eng, ref, sets=family == "deepseek")
        assert_block_close(out, ref, torch.bfloat16, f"round {rnd}: MXFP4 GEMM vs the oracle on dequantised weights")
        # the bar test_gpu_fp8_gemm.py set for a GEMM that sums k in another order than the row kernel
        assert_model_close(eng.expert_outputs(rows.shape[0]), rows, torch.bfloat16, f"round {rnd}: expert FFN rows", ulps=2.0)
        st = eng.stats()
        assert (st["expert_misses"] > 0) if rnd == 0 else (st["expert_hits"] > 0)
    if want is not None:
        assert eng.last_ffn_forms() == want, ("the kernels the sync-free forward took", eng.last_ffn_forms(), want)
    counts = [int(ref.expert_out[i].shape[0]) if i in ref.expert_out else 0 for i in range(e)]
    eng.close()
    return counts


@pytest.mark.parametrize("family,h,f,e,k,n_shared,t,est,want1,want2", [
    # K = 384 in stage 2: 3 code tiles per row group, scale dwords that straddle row groups; a partial token group (19 rows)
    ("mixtral", 512, 384, 8, 2, 0, 48, 19, (HYB, 4), (HYB, 4)),
    # the 8-wave form, a code tile across two stages, an odd tile count
    ("mixtral", 512, 384, 8, 2, 0, 512, 193, (LDS, 8), (LDS, 8)),
    # an expert with more rows than one pass of the 8-wave form holds
    ("mixtral", 512, 256, 8, 2, 0, 1024, 385, (LDS, 8), (LDS, 8)),
    # DeepSeek-V2-Lite's widths: 11 tiles = 11 hybrid stages (odd) in stage 2, the bf16 shared expert in the launch
    ("deepseek", 2048, 1408, 8, 4, 1, 40, 31, (HYB, 4), (HYB, 4)),
    # the 4-wave form, 65 active: the shared expert's workgroups take the bf16 body
    ("deepseek", 1024, 384, 64, 6, 2, 512, 73, (LDS, 4), (LDS, 4)),
    # the hybrid with the shared expert
    ("deepseek", 1024, 384, 64, 6, 2, 160, 23, (HYB, 4), (HYB, 4))],
    ids=["hyb_t48", "lds8_t512", "lds8_two_passes_t1024", "dsv2_widths_hyb_t40", "ds_lds4_shared_t512", "ds_hyb_shared_t160"])
def test_mxfp4_gemm_forms_equal_the_oracle(family, h, f, e, k, n_shared, t, est, want1, want2):
    rows, f1, f2 = _forms(h, f, e, k, t, n_shared)
    assert rows == est and f1 == want1 and f2 == want2, (rows, f1, f2)
    counts = _run(family, h, f, e, k, t, 11100 + t + h, n_shared, want=(want1[0], want2[0]))
    if t == 1024:
        assert max(counts) > 256, ("an expert with more rows than one pass of the 8-wave form holds", counts)


def test_every_token_on_two_experts_takes_extra_passes_and_leaves_experts_empty():
    """the row estimate (193) picks the 8-wave LDS form; experts 0 and 1 get all 512 rows (two passes), the other six none"""
    h, f, e, k, t = 512, 384, 8, 2, 512
    rows, f1, f2 = _forms(h, f, e, k, t)
    assert f1 == (LDS, 8) and f2 == (LDS, 8)
    weights = _mx_weights("mixtral", h, f, e, 11300)
    gate = torch.zeros_like(weights[0])
    gate[0, 0], gate[1, 0] = 2.0, 1.0  # logits 8, 4, then 0 for every other expert
    x = acts(t, h, torch.bfloat16, 11301)
    x[:, 0] = 4.0
    counts = _run("mixtral", h, f, e, k, t, 11300, x=x, gate=gate, weights=weights, want=(LDS, LDS))
    assert counts[:2] == [t, t] and counts[2:] == [0] * 6, counts


def test_the_switch_goes_on_and_off_on_one_engine():
    h, f, e, k, t = 512, 384, 8, 2, 48
    gate, packed, deq, _ = _mx_weights("mixtral", h, f, e, 11400)
    x = acts(t, h, torch.bfloat16, 11401)
    ref = _oracle("mixtral", x, gate, deq, k, None)
    n_rows = oracle_expert_rows(ref, e).shape[0]
    eng = _engine("mixtral", h, f, e, k, max_tokens=t)
    register_all(eng, packed)
    got = []
    for on, want in ((None, (ROWS, ROWS)), (True, (HYB, HYB)), (False, (ROWS, ROWS))):
        if on is not None:
            eng.set_mxfp4_gemm(on)
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
        assert eng.last_ffn_forms() == want, (on, eng.last_ffn_forms())
        _routing_exact(eng, ref)
        assert_block_close(out, ref, torch.bfloat16, f"switch {on}")
        got.append(eng.expert_outputs(n_rows))
    assert_model_close(got[1], got[0], torch.bfloat16, "GEMM forms vs row kernel, expert FFN rows", ulps=2.0)
    assert_model_close(got[1], got[2], torch.bfloat16, "GEMM forms vs row kernel again, expert FFN rows", ulps=2.0)
    # one token with the switch on: still the decode launchers
    eng.set_mxfp4_gemm(True)
    x1 = acts(1, h, torch.bfloat16, 11402)
    out = eng.forward(0, x1.to(DEV), gate.to(DEV))
    assert eng.last_ffn_forms() == (-2, -2), eng.last_ffn_forms()
    assert_block_close(out, _oracle("mixtral", x1, gate, deq, k, None), torch.bfloat16, "decode with the switch on")
    eng.close()


def test_an_engine_without_mxfp4_slots_refuses_the_switch():
    eng = _engine("mixtral", 256, 512, 8, 2, mxfp4=False, max_tokens=4)
    with pytest.raises(Exception, match="mxfp4"):
        eng.set_mxfp4_gemm(True)
    eng.close()
