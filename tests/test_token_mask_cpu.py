"""Token masks without a device: the new C-ABI symbol, its argument refusals, the NLLB block's reduction of HF padding
masks (against transformers' own NllbMoeTop2Router.route_tokens) and the padded golden fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import R, load_golden, make_weights, tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from moe_infinity_amd import load_library

    return load_library()


def test_masked_forward_is_declared_prototyped_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moeinf.h")).read(), flags=re.S)
    m = re.search(r"int\s+moeinf_moe_forward_masked\s*\(([^)]*)\)", hdr)
    assert m, "moeinf_moe_forward_masked is not declared"
    assert "const uint8_t* token_mask_dev" in re.sub(r"\s+", " ", m.group(1))
    from moe_infinity_amd._lib import PROTOTYPES

    assert PROTOTYPES["moeinf_moe_forward_masked"][1][:9] == PROTOTYPES["moeinf_moe_forward"][1]
    assert len(PROTOTYPES["moeinf_moe_forward_masked"][1]) == 10
    assert hasattr(lib, "moeinf_moe_forward_masked")
    assert lib.moeinf_abi_version() == 4


def test_masked_forward_refuses_a_null_engine(lib):
    mask = (C.c_uint8 * 4)(1, 0, 1, 1)
    rc = lib.moeinf_moe_forward_masked(None, 0, None, 4, 1, None, None, None, 0, C.cast(mask, C.c_void_p))
    assert rc == 1
    assert b"engine is NULL" in lib.moeinf_last_error()
    assert lib.moeinf_moe_forward_masked(None, 0, None, 4, 1, None, None, None, 0, None) == 1


def _hf_router(e=8, ignore=False):
    from transformers import NllbMoeConfig
    from transformers.models.nllb_moe.modeling_nllb_moe import NllbMoeTop2Router

    cfg = NllbMoeConfig(d_model=32, num_experts=e, expert_capacity=1024, router_dtype="float32", second_expert_policy="all",
                        batch_prioritized_routing=False, moe_eval_capacity_token_fraction=1.0, router_ignore_padding_tokens=ignore)
    return NllbMoeTop2Router(cfg).eval(), cfg


def _hf_routed(router, t, padding_mask):
    """tokens route_tokens gives a pair (its top-1 / top-2 masks survive the padding reduction)"""
    logits = torch.randn(t, router.num_experts, generator=torch.Generator().manual_seed(t))
    top1, probs = router.route_tokens(logits, torch.float32, padding_mask)
    return top1.sum(-1) != 0


def _additive(keep_keys, q_len, causal=False):
    b, skv = keep_keys.shape
    m = torch.zeros((b, 1, q_len, skv))
    m.masked_fill_(~keep_keys[:, None, None, :], torch.finfo(torch.float32).min)
    if causal:
        q = torch.arange(q_len)[:, None] + (skv - q_len)
        m.masked_fill_((torch.arange(skv)[None, :] > q)[None, None], torch.finfo(torch.float32).min)
    return m


def test_nllb_padding_reduction_matches_hf_route_tokens():
    from moe_infinity_amd.blocks import nllb_non_padding

    router, _ = _hf_router()
    lengths = torch.tensor([7, 3, 5, 1])
    keep = torch.arange(7)[None, :] < lengths[:, None]
    t = keep.numel()
    # 2-D [B, S] key-padding mask (1 = pad): route_tokens broadcasts it per token once flattened
    pad2d = (~keep).long()
    np_ = nllb_non_padding(pad2d, t)
    assert torch.equal(np_, keep.reshape(-1))
    assert torch.equal(np_, _hf_routed(router, t, pad2d.reshape(-1)))
    # encoder: HF's additive 4-D mask [B, 1, S, S]
    enc = _additive(keep, 7)
    assert torch.equal(nllb_non_padding(enc, t), _hf_routed(router, t, enc))
    assert torch.equal(nllb_non_padding(enc, t), keep.reshape(-1))
    # decoder prefill: causal + padding, [B, 1, S, S]; route_tokens reads the last query row of every sequence
    dec = _additive(keep, 7, causal=True)
    assert torch.equal(nllb_non_padding(dec, t), _hf_routed(router, t, dec))
    # decoder step: [B, 1, 1, S_kv], nb_tokens = B: the last B entries of the flattened last-query rows (HF's quirk)
    keep_kv = torch.ones((4, 9), dtype=torch.bool)
    keep_kv[3, 6:] = False
    step = _additive(keep_kv, 1)
    got = nllb_non_padding(step, 4)
    assert torch.equal(got, _hf_routed(router, 4, step))
    assert got.tolist() == [True, False, False, False]
    with pytest.raises(ValueError):
        nllb_non_padding(pad2d, t - 1)


class _FakeEngine:
    """records the mask the block hands the engine; reports routing the way moeinf_copy_routing_dev does"""

    def __init__(self, idx, w):
        self.idx, self.w, self.mask = idx, w, "unset"

    def forward(self, layer, x, gate_w, batch_rows=1, token_mask=None):
        self.mask = token_mask
        return x.clone()

    def routing_tensors(self, logits=True, topk=False):
        return None, self.idx, self.w


@pytest.mark.parametrize("ignore", [False, True])
def test_nllb_block_hands_the_reduced_mask_to_the_engine(ignore):
    from moe_infinity_amd.blocks import SyncNllbMoeSparseMLP

    _, cfg = _hf_router(ignore=ignore)
    blk = SyncNllbMoeSparseMLP(cfg, 64)
    keep = torch.tensor([[True, True, False], [True, False, False]])
    pm = _additive(keep, 3)
    idx = torch.tensor([[3, 5], [1, 4], [-1, -1], [2, 7], [-1, -1], [-1, -1]], dtype=torch.int32)
    w = torch.tensor([[0.75, 0.25], [0.5, 0.5], [0, 0], [0.5, 0.5], [0, 0], [0, 0]])
    if ignore:  # the engine reports every token routed
        idx = torch.tensor([[3, 5], [1, 0], [4, 6], [2, 7], [0, 1], [6, 2]], dtype=torch.int32)
        w = torch.full((6, 2), 0.5)
    blk.engine = _FakeEngine(idx, w)
    blk.layer_id = 0
    x = torch.randn(2, 3, 32)
    out, (probs, top1) = blk(x, pm)
    if ignore:
        assert blk.engine.mask is None
        assert top1.tolist() == [3, 1, 4, 2, 0, 6]
        return
    assert blk.engine.mask.tolist() == keep.reshape(-1).tolist()
    assert top1.tolist() == [3, 1, 0, 2, 0, 0]
    assert probs[2].abs().sum() == 0 and probs[4].abs().sum() == 0 and probs[5].abs().sum() == 0
    assert probs[0, 3] == 0.75 and probs[0, 5] == 0.25 and probs[3, 2] == 0.5 and probs[3, 7] == 0.5


@pytest.mark.parametrize("name", ["nllb_padded_enc_bf16.npz", "nllb_padded_enc_norm_before_bf16.npz", "nllb_padded_dec_bf16.npz"])
def test_padded_golden_equals_the_restated_contract(name):
    """The reference block with a padding mask = the oracle block on the real tokens, pad rows = x (HF's padding semantics):
    the restatement the GPU tests use, checked against the reference's own output."""
    from moe_infinity_amd.blocks import nllb_non_padding
    from oracle import parity as P

    z = load_golden(name)
    b, s, h, f, e, seed, norm_before = [int(v) for v in z["meta"]]
    keep = nllb_non_padding(torch.from_numpy(z["padding_mask"]), b * s)
    probs = z["router_probs"].reshape(b * s, e)
    assert np.array_equal((probs != 0).any(-1), keep.numpy()), "pad rows route nowhere, real rows route"
    assert (z["top1"].reshape(-1)[~keep.numpy()] == 0).all()
    gate, experts, _ = make_weights("nllb", h, f, e, seed, torch.bfloat16, gate_std=0.5)
    x = tt(z["x"], torch.bfloat16).reshape(b * s, h)
    real = keep.nonzero()[:, 0]
    sub = R.block_nllb(x[real][None], gate, experts, normalize_router_prob_before_dropping=bool(norm_before))
    out = torch.from_numpy(z["out"]).reshape(b * s, h)
    assert torch.equal(out[~keep], x[~keep].float()), "pad rows are the input (next_states == 0 passthrough)"
    rep = P.block_report(out[real].to(torch.bfloat16), sub, torch.bfloat16, x=x[real])
    assert rep["ok"], rep
    assert np.array_equal(sub.router_mask.reshape(-1, e).numpy(), probs[keep.numpy()] != 0)
