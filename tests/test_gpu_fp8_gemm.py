"""The fp8-weight grouped GEMMs (csrc/ffn_gemm_f8.hip): prefill-sized stages of an fp8-slot engine run the hybrid, LDS-staged and
register-ring kernels on e4m3fn tiles up-cast in registers.  Each case first asks the selection export (moeinf_ffn_f8_gemm_form)
which form the engine's row estimate picks, then checks the layer against the oracle on the up-cast weights, y = FFN(x;
W.to(bf16)), routing exact, on the decision path (first forward, misses) and the sync-free path (second).  The weights hold every
finite e4m3fn code.  Needs an MI355X: -m gpu."""
import ctypes as C

import pytest
import torch

from helpers import (R, acts, assert_as_accurate_as_the_oracle, assert_block_close, assert_model_close, oracle_expert_rows,
                     register_all)
from moe_infinity_amd import load_library
from test_gpu_fp8_slots import _engine, _every_code, _routing_exact, _up

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn
ROWS, HYB, LDS, RING2 = 0, 1, 2, 3


def _form(nmat, K, Rr, active, rows, K_sh=0):
    out = (C.c_int32 * 6)()
    assert load_library().moeinf_ffn_f8_gemm_form(nmat, K, K_sh, Rr, active, rows, 256, out) == 0
    return tuple(out)


def _forms(family, h, f, e, k, t, n_shared=0):
    """(stage 1, stage 2) forms for the sync-free path's row estimate"""
    rows = load_library().moeinf_rows_estimate(t, k, e)
    fs = f * n_shared
    active = min(e, t * k) + (1 if n_shared else 0)
    return (_form(2, h, max(f, fs), active, rows, K_sh=h if n_shared else 0),
            _form(1, f, h, active, rows, K_sh=fs))


def _weights(family, h, f, e, seed, n_shared=0):
    """N(0, 0.02^2) e4m3fn experts generated on the GPU, every finite code stamped in; the shared expert fp8 too (the engine keeps
    it bf16).  Returns the gate and CPU fp8 tensors."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    shapes = [(f, h), (h, f), (f, h)] if family == "mixtral" else [(f, h), (f, h), (h, f)]
    ex8 = [[_every_code(torch.empty(s, device=DEV).normal_(0.0, 0.02, generator=g).to(F8), 3 * i + j).cpu() for j, s in enumerate(shapes)]
           for i in range(e)]
    sh8 = None
    if n_shared:
        fs = f * n_shared
        sh8 = [torch.empty(s, device=DEV).normal_(0.0, 0.02, generator=g).to(F8).cpu() for s in [(fs, h), (fs, h), (h, fs)]]
    gate = (torch.randn(e, h, generator=torch.Generator().manual_seed(seed + 1)) * 0.02).to(torch.bfloat16)
    return gate, ex8, sh8


def _run(family, h, f, e, k, t, seed, n_shared=0, x=None, gate=None, fp8_slots=True, weights=None):
    gate0, ex8, sh8 = weights or _weights(family, h, f, e, seed, n_shared)
    gate = gate0 if gate is None else gate
    x = acts(t, h, torch.bfloat16, seed + 2) if x is None else x
    eng = _engine(family, h, f, e, k, fp8_slots=fp8_slots, n_shared=n_shared, max_tokens=t)
    register_all(eng, ex8, sh8)
    up = [_up(ts) for ts in ex8]
    if family == "mixtral":
        ref = R.block_mixtral(x[None], gate, up, top_k=k)
    else:
        ref = R.block_deepseek(x[None], gate, up, k, shared=_up(sh8))
    rows = oracle_expert_rows(ref, e)
    outs = []
    for rnd in range(2):  # misses (the decision path), then hits (the sync-free path)
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
        _routing_exact(eng, ref, sets=family == "deepseek")
        assert_block_close(out, ref, torch.bfloat16, f"round {rnd}: fp8 GEMM vs the oracle on up-cast weights")
        got = eng.expert_outputs(rows.shape[0])
        if rnd == 1:  # the fp32-exact arm (as test_gpu_fp8_slots.py's full-size layers): as close to fp32 as the oracle is
            assert_as_accurate_as_the_oracle(out, ref, family, x[None], up, torch.bfloat16, "fp8 GEMM layer", shared=_up(sh8), rows=got)
        # the fp8 forms sum k in another order than the bf16 kernels; with every e4m3fn code in the weights (+-448 included) a
        # last-bit flip carried through the gated epilogue's three rounding points reached 1.6 ulp in one of 7.3 M elements
        assert_model_close(got, rows, torch.bfloat16, f"round {rnd}: expert FFN rows", ulps=2.0)
        st = eng.stats()
        assert (st["expert_misses"] > 0) if rnd == 0 else (st["expert_hits"] > 0)
        outs.append((out.cpu(), got))
    counts = [int(ref.expert_out[i].shape[0]) if i in ref.expert_out else 0 for i in range(e)]
    eng.close()
    return outs, counts


@pytest.mark.parametrize("family,h,f,e,k,t,n_shared,want1,want2", [
    ("mixtral", 4096, 4096, 8, 2, 48, 0, (HYB, 4), (RING2, 8)),
    ("mixtral", 4096, 5120, 8, 2, 512, 0, (RING2, 12, 1), (RING2, 12, 0)),
    ("mixtral", 4096, 4096, 8, 2, 896, 0, (RING2, 16), (RING2, 16)),
    ("mixtral", 1024, 2048, 8, 2, 1024, 0, (LDS, 8), (LDS, 8)),
    ("deepseek", 1024, 512, 64, 6, 512, 2, (LDS, 4), (LDS, 4)),
    ("deepseek", 1024, 512, 64, 6, 160, 2, (HYB, 4), (HYB, 4))],
    ids=["hyb_gated_ring2_plain_t48", "ring2_ntb12_split_tail_t512", "ring2_ntb16_t896", "lds8_two_passes_t1024",
         "deepseek_lds_shared_expert_t512", "deepseek_hyb_shared_expert_t160"])
def test_fp8_gemm_forms_equal_the_oracle(family, h, f, e, k, t, n_shared, want1, want2):
    f1, f2 = _forms(family, h, f, e, k, t, n_shared)
    assert f1[:len(want1)] == want1 and f2[:len(want2)] == want2, (f1, f2)
    _outs, counts = _run(family, h, f, e, k, t, 7100 + t + h, n_shared)
    if t == 1024:
        assert max(counts) > 256, ("an expert with more rows than one pass of the 8-wave form holds", counts)


def test_every_token_on_two_experts_takes_extra_passes_and_leaves_experts_empty():
    """the row estimate (193) picks ring2's 192-token form; experts 0 and 1 get all 512 rows (three passes), the other six none"""
    h, f, e, k, t = 4096, 4096, 8, 2, 512
    f1, f2 = _forms("mixtral", h, f, e, k, t)
    assert f1[:2] == (RING2, 12) and f2[:2] == (RING2, 12)
    weights = _weights("mixtral", h, f, e, 7300)
    gate = torch.zeros_like(weights[0])
    gate[0, 0], gate[1, 0] = 2.0, 1.0  # logits 8, 4, then 0 for every other expert
    x = acts(t, h, torch.bfloat16, 7301)
    x[:, 0] = 4.0
    _outs, counts = _run("mixtral", h, f, e, k, t, 7300, x=x, gate=gate, weights=weights)
    assert counts[:2] == [t, t] and counts[2:] == [0] * 6, counts


def test_fp8_slots_equal_bf16_slots_on_the_same_fp8_weights_at_512_tokens():
    h, f, e, k, t = 4096, 5120, 8, 2, 512
    weights = _weights("mixtral", h, f, e, 7400)
    x = acts(t, h, torch.bfloat16, 7401)
    a, _ = _run("mixtral", h, f, e, k, t, 7400, x=x, fp8_slots=False, weights=weights)
    b, _ = _run("mixtral", h, f, e, k, t, 7400, x=x, fp8_slots=True, weights=weights)
    # both engines met the block bar against the oracle in _run; their expert rows agree within the multi-token bar
    for (_oa, ra), (_ob, rb) in zip(a, b):
        assert_model_close(rb, ra, torch.bfloat16, "fp8 slots vs bf16 slots, expert FFN rows", ulps=2.0)
