"""Token masks (moeinf_moe_forward_masked / MoEEngine.forward(token_mask=...) / the NLLB block's padding_mask) on the GPU.

The masked forward is compared with an in-test restatement of the contract: the oracle block run on the real tokens only,
the masked rows filled by the family's no-pair rule (Mixtral / Grok: 0, DeepSeek: the shared expert alone, Switch:
router_prob * x, NLLB: x).  Needs an MI355X: -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import R, acts, assert_block_close, engine_for, load_golden, make_weights, register_all, tt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn

# family -> (h, f, e, k, n_shared, engine kw, oracle kw, gate std)
FAM = {
    "mixtral": (256, 512, 8, 2, 0, {}, {}, 0.02),
    "grok": (256, 512, 8, 2, 0, {}, {}, 0.02),
    "deepseek": (256, 192, 16, 4, 2, {}, {}, 0.02),
    "deepseek_v3": (256, 192, 16, 4, 1, {"n_group": 4, "topk_group": 2, "norm_topk_prob": True, "routed_scaling_factor": 2.5},
                    {"n_group": 4, "topk_group": 2, "norm_topk_prob": True, "routed_scaling_factor": 2.5}, 0.02),
    "switch": (192, 384, 8, 1, 0, {}, {}, 0.5),
    "nllb": (256, 512, 16, 2, 0, {}, {}, 0.5),
}
SWITCH_CAP = 3  # binds at T >= 4: the capacity of the real tokens decides which of them are dropped


def _engine(family, t, dtype=torch.bfloat16, **extra):
    from moe_infinity_amd import config as Cf

    h, f, e, k, n_sh, kw, _, _ = FAM[family]
    kw = dict(kw)
    base = {"grok": "mixtral", "deepseek_v3": "deepseek"}.get(family, family)
    if family == "grok":
        kw["router_kind"] = Cf.ROUTER_SOFTMAX_TOPK
    if family == "deepseek_v3":
        kw["router_kind"] = Cf.ROUTER_DEEPSEEK_V3
    if family == "switch":
        kw["expert_capacity"] = SWITCH_CAP
    kw.update(extra)
    return engine_for(base, h, f, e, k, dtype, n_shared=n_sh, max_tokens=max(t, 8), **kw)


def _weights(family, seed, dtype=torch.bfloat16):
    h, f, e, k, n_sh, _, _, std = FAM[family]
    base = {"grok": "mixtral", "deepseek_v3": "deepseek"}.get(family, family)
    return make_weights(base, h, f, e, seed, dtype, n_shared=n_sh, gate_std=std)


def _oracle(family, x3d, gate, experts, shared, e_bias=None):
    h, f, e, k, n_sh, _, okw, _ = FAM[family]
    if family == "mixtral":
        return R.block_mixtral(x3d, gate, experts, top_k=k)
    if family == "grok":
        return R.block_grok(x3d, gate, experts, top_k=k)
    if family == "deepseek":
        return R.block_deepseek(x3d, gate, experts, k, shared=shared)
    if family == "deepseek_v3":
        return R.block_deepseek(x3d, gate, experts, k, shared=shared, e_bias=e_bias, **okw)
    if family == "switch":
        return R.block_switch(x3d, gate, experts, expert_capacity=SWITCH_CAP)
    return R.block_nllb(x3d, gate, experts)


def restate(family, x2d, keep, gate, experts, shared=None, e_bias=None):
    """The contract, restated: the oracle block on the real tokens only (one batch row, in token order), masked rows = the
    family's no-pair rule.  Returns a full-size BlockResult for helpers.assert_block_close."""
    T, H = x2d.shape
    E = gate.shape[0]
    real = keep.nonzero()[:, 0]
    sub = _oracle(family, x2d[real][None], gate, experts, shared, e_bias) if real.numel() else None
    out = torch.zeros((T, H), dtype=x2d.dtype)
    r = R.BlockResult(out=out, router_mask=torch.zeros((T, E), dtype=torch.bool))
    if family in ("deepseek", "deepseek_v3"):
        sh = R.expert_ffn(x2d, shared, R.DEEPSEEK_DENSE_ACT_DENSE)
        out[:] = sh
        r.extra["shared_out"] = sh
    elif family == "switch":
        _, probs, _ = R.route_switch(x2d[None], gate, SWITCH_CAP)
        probs = probs.reshape(T, 1)
        out[:] = probs * x2d
        r.extra["router_probs"] = probs
    elif family == "nllb":
        out[:] = x2d
        r.extra["pre_passthrough"] = torch.zeros((T, H), dtype=x2d.dtype)
        r.extra["x"] = x2d
    if sub is not None:
        out[real] = sub.out.reshape(-1, H)
        r.router_mask[real] = sub.router_mask.reshape(-1, E)
        r.expert_out = sub.expert_out
        if sub.weights_mask is not None:
            r.weights_mask = torch.zeros((T, E), dtype=sub.weights_mask.dtype)
            r.weights_mask[real] = sub.weights_mask.reshape(-1, E)
        if sub.topk_idx is not None and family != "switch":
            r.topk_idx = torch.full((T, sub.topk_idx.shape[1]), -1, dtype=torch.long)
            r.topk_idx[real] = sub.topk_idx.reshape(real.numel(), -1).long()
        if family == "nllb":
            r.extra["pre_passthrough"][real] = sub.extra["pre_passthrough"].reshape(-1, H)
    return r


def _mask(t, pattern):
    if pattern == "real":
        return torch.ones(t, dtype=torch.bool)
    if pattern == "masked":
        return torch.zeros(t, dtype=torch.bool)
    keep = torch.ones(t, dtype=torch.bool)
    keep[: t // 4] = False  # left padding
    keep[t // 4 + 1::5] = False  # and some inside
    return keep


def _check(eng, out, ref, keep, family, dtype, what):
    r = eng.routing()
    got = np.zeros(ref.router_mask.shape, dtype=bool)
    for t, row in enumerate(r["topk_idx"]):
        for i in row:
            if i >= 0:
                got[t, i] = True
    assert np.array_equal(got, ref.router_mask.numpy()), f"{what}: routing of the real tokens must be bit-exact, masked pairs dropped"
    assert not got[~keep.numpy()].any(), f"{what}: a masked token has a pair"
    assert (r["topk_w"][~keep.numpy()] == 0).all(), f"{what}: a masked pair has a weight"
    if family in ("mixtral", "grok") and ref.topk_idx is not None:
        assert np.array_equal(r["topk_idx"], ref.topk_idx.numpy().astype(np.int32)), f"{what}: routing indices"
    e = ref.router_mask.shape[1]
    assert np.array_equal(r["counts"][:e], ref.router_mask.sum(0).numpy().astype(np.int32)), f"{what}: expert rows count real pairs only"
    assert_block_close(out, ref, dtype, what)


CASES = [("mixtral", 1, "masked"), ("mixtral", 1, "real"), ("mixtral", 4, "ragged"), ("mixtral", 32, "ragged"), ("mixtral", 200, "ragged"),
         ("mixtral", 2048, "ragged"),
         ("grok", 1, "masked"), ("grok", 4, "ragged"), ("grok", 200, "ragged"),
         ("deepseek", 1, "masked"), ("deepseek", 1, "real"), ("deepseek", 4, "ragged"), ("deepseek", 32, "ragged"), ("deepseek", 200, "ragged"),
         ("deepseek_v3", 1, "masked"), ("deepseek_v3", 4, "ragged"), ("deepseek_v3", 200, "ragged"),
         ("switch", 1, "masked"), ("switch", 1, "real"), ("switch", 4, "ragged"), ("switch", 32, "ragged"), ("switch", 200, "ragged"),
         ("nllb", 1, "masked"), ("nllb", 1, "real"), ("nllb", 4, "ragged"), ("nllb", 32, "ragged"), ("nllb", 200, "ragged"),
         ("mixtral", 8, "masked"), ("deepseek", 8, "masked"), ("switch", 8, "masked"), ("nllb", 8, "masked")]


@pytest.mark.parametrize("family,t,pattern", CASES, ids=[f"{f}_t{t}_{p}" for f, t, p in CASES])
def test_masked_forward_equals_the_restated_contract(family, t, pattern):
    seed = 7100 + t + 17 * list(FAM).index(family)
    gate, experts, shared = _weights(family, seed)
    h = FAM[family][0]
    eng = _engine(family, t)
    register_all(eng, experts, shared)
    e_bias = None
    if family == "deepseek_v3":
        e_bias = torch.linspace(-0.05, 0.05, FAM[family][2])
        bias = e_bias.to(DEV, torch.float32).contiguous()
        eng.set_gate_bias(0, bias)
    x = acts(t, h, torch.bfloat16, seed + 1)
    keep = _mask(t, pattern)
    fwd0 = eng.stats()["forwards"]
    out = eng.forward(0, x.to(DEV), gate.to(DEV), token_mask=keep.to(DEV))
    torch.cuda.synchronize()
    ref = restate(family, x, keep, gate, experts, shared, e_bias)
    _check(eng, out, ref, keep, family, torch.bfloat16, f"{family} T={t} {pattern}")
    st = eng.stats()
    assert st["forwards"] == fwd0 + 1
    if not keep.any():
        assert st["expert_misses"] == 0 and int(eng.routing()["counts"][: FAM[family][2]].sum()) == 0
    # the same engine, no mask: today's forward, unchanged
    out2 = eng.forward(0, x.to(DEV), gate.to(DEV))
    torch.cuda.synchronize()
    _check(eng, out2, restate(family, x, torch.ones(t, dtype=torch.bool), gate, experts, shared, e_bias), torch.ones(t, dtype=torch.bool),
           family, torch.bfloat16, f"{family} T={t} unmasked after masked")
    eng.close()


@pytest.mark.parametrize("t", [1, 4, 200])
def test_masked_forward_with_fp8_slots(t):
    from moe_infinity_amd import config as Cf

    gate, experts, _ = make_weights("mixtral", 256, 512, 8, 7300 + t, torch.bfloat16)
    ex8 = [[w.to(F8) for w in ts] for ts in experts]
    up = [[w.to(torch.bfloat16) for w in ts] for ts in ex8]
    from moe_infinity_amd import MoEEngine

    eng = MoEEngine(Cf.EngineConfig(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2,
                                    router_kind=Cf.ROUTER_MIXTRAL, dtype=Cf.DTYPE_F8E4M3, gate_dtype=Cf.DTYPE_BF16, device_memory_ratio=0.5,
                                    max_tokens=max(t, 8), fp8_slots=True))
    assert eng.slot_dtype == Cf.DTYPE_F8E4M3
    register_all(eng, ex8)
    x = acts(t, 256, torch.bfloat16, 7301 + t)
    for pattern in ("masked", "ragged") if t == 1 else ("ragged",):
        keep = _mask(t, pattern)
        out = eng.forward(0, x.to(DEV), gate.to(DEV), token_mask=keep.to(DEV))
        torch.cuda.synchronize()
        _check(eng, out, restate("mixtral", x, keep, gate, up), keep, "mixtral", torch.bfloat16, f"fp8 slots T={t} {pattern}")
    eng.close()


def test_mask_accepts_bs_bool_and_uint8_and_refuses_bad_masks():
    gate, experts, _ = _weights("mixtral", 7400)
    eng = _engine("mixtral", 24)
    register_all(eng, experts)
    x = acts(24, 256, torch.bfloat16, 7401)
    keep = _mask(24, "ragged")
    ref = restate("mixtral", x, keep, gate, experts)
    for m in (keep.reshape(2, 12), keep.to(torch.uint8)):
        out = eng.forward(0, x.reshape(2, 12, 256).to(DEV), gate.to(DEV), token_mask=m.to(DEV))
        torch.cuda.synchronize()
        _check(eng, out, ref, keep, "mixtral", torch.bfloat16, f"mask {m.dtype} {tuple(m.shape)}")
    for bad in (keep, keep.to(DEV).float(), keep[:10].to(DEV)):
        with pytest.raises(ValueError, match="token_mask"):
            eng.forward(0, x.to(DEV), gate.to(DEV), token_mask=bad)
    eng.close()


def test_masked_token_never_causes_a_miss():
    """An expert only masked tokens route to stays non-resident and expert_misses does not count it; without the mask the
    same batch fetches it."""
    h, f, e, k = 256, 512, 8, 2
    gate, experts, _ = make_weights("mixtral", h, f, e, 7500, torch.bfloat16)
    eng = engine_for("mixtral", h, f, e, k, torch.bfloat16, max_tokens=8)
    register_all(eng, experts)
    slot = eng.stats()["slot_bytes"]
    eng.set_cache_budget(3 * slot)
    x_real = acts(1, h, torch.bfloat16, 7501)
    real_set = set(int(i) for i in R.block_mixtral(x_real[None], gate, experts, top_k=k).topk_idx[0])
    resident = {i for i in range(e) if eng.is_resident(0, i)}
    cand = [i for i in range(e) if i not in real_set and i not in resident]
    assert len(cand) >= 2, (real_set, resident)
    a, b = cand[:2]
    x_pad = ((gate[a].float() + gate[b].float()) * 100.0).to(torch.bfloat16)[None].repeat(3, 1)
    x = torch.cat([x_pad, x_real], 0)  # left-padded prompt
    assert set(int(i) for i in R.block_mixtral(x_pad[:1][None], gate, experts, top_k=k).topk_idx[0]) == {a, b}
    keep = torch.tensor([False, False, False, True])
    eng.reset_stats()
    out = eng.forward(0, x.to(DEV), gate.to(DEV), token_mask=keep.to(DEV))
    eng.sync()
    st = eng.stats()
    assert not eng.is_resident(0, a) and not eng.is_resident(0, b), "a masked token fetched an expert"
    assert st["expert_misses"] == len(real_set - resident), st
    _check(eng, out, restate("mixtral", x, keep, gate, experts), keep, "mixtral", torch.bfloat16, "residency, masked")
    eng.forward(0, x.to(DEV), gate.to(DEV))
    eng.sync()
    assert eng.stats()["expert_misses"] > st["expert_misses"], "without the mask the pads' experts are fetched"
    eng.close()


def test_mask_under_expert_parallelism_is_refused_before_anything_is_enqueued():
    from moe_infinity_amd import MoEEngine, MoeInfError
    from moe_infinity_amd import config as Cf

    h, f, e, k = 256, 512, 8, 2
    gate, experts, _ = make_weights("mixtral", h, f, e, 7600, torch.bfloat16)
    eng = MoEEngine(Cf.EngineConfig(num_layers=1, num_experts=e, expert_type=Cf.EXPERT_MIXTRAL, hidden=h, inter=f, top_k=k,
                                    router_kind=Cf.ROUTER_MIXTRAL, device_memory_ratio=0.25, ep_rank=0, ep_size=2, max_tokens=8))
    for i in range(0, e, 2):
        eng.register_expert(0, i, experts[i])
    x = acts(4, h, torch.bfloat16, 7601).to(DEV)
    keep = torch.ones(4, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    g = gate.to(DEV)
    f0 = eng.stats()["forwards"]
    rc = eng.lib.moeinf_moe_forward_masked(eng._h, 0, C.c_void_p(x.data_ptr()), 4, 1, C.c_void_p(g.data_ptr()), C.c_void_p(out.data_ptr()),
                                           None, 1, C.c_void_p(keep.data_ptr()))  # (ROUTE_ONLY: what an EP rank would run)
    assert rc == 5, rc
    assert "expert parallelism" in eng.lib.moeinf_last_error().decode()
    with pytest.raises(MoeInfError, match="expert parallelism"):
        eng.forward(0, x, g, token_mask=keep)
    assert eng.stats()["forwards"] == f0, "nothing may be enqueued"
    eng.close()


@pytest.mark.parametrize("name", ["nllb_padded_enc_bf16.npz", "nllb_padded_enc_norm_before_bf16.npz", "nllb_padded_dec_bf16.npz"])
def test_nllb_block_with_padding_mask_equals_the_reference(name):
    """SyncNllbMoeSparseMLP.forward(hidden_states, padding_mask) (the call HF's NLLB-MoE encoder / decoder layers make) against
    the reference block's own output on the same padded batch (tools/gen_golden_padded.py)."""
    from transformers import NllbMoeConfig

    from moe_infinity_amd.blocks import SyncNllbMoeSparseMLP

    z = load_golden(name)
    b, s, h, f, e, seed, norm_before = [int(v) for v in z["meta"]]
    gate, experts, _ = make_weights("nllb", h, f, e, seed, torch.bfloat16, gate_std=0.5)
    cfg = NllbMoeConfig(d_model=h, num_experts=e, normalize_router_prob_before_dropping=bool(norm_before), router_ignore_padding_tokens=False)
    blk = SyncNllbMoeSparseMLP(cfg, f)
    with torch.no_grad():
        blk.router.classifier.weight.copy_(gate)
    blk.router.classifier.to(DEV, torch.bfloat16)
    eng = engine_for("nllb", h, f, e, 2, torch.bfloat16, max_tokens=b * s, norm_topk_prob=bool(norm_before))
    register_all(eng, experts)
    blk.attach_engine(eng, 0)
    x = tt(z["x"], torch.bfloat16)
    pm = torch.from_numpy(z["padding_mask"]).to(DEV)
    out, (router_probs, top1) = blk(x.to(DEV), pm)
    torch.cuda.synchronize()
    keep = torch.from_numpy(z["router_probs"].reshape(b * s, e) != 0).any(-1)
    ref = restate("nllb", x.reshape(-1, h), keep, gate, experts)
    ref.out = ref.out.reshape(b, s, h)
    assert_block_close(out, ref, torch.bfloat16, "padded NLLB block vs the restated contract")
    assert_block_close(out, ref, torch.bfloat16, "padded NLLB block vs the reference block", golden=tt(z["out"], torch.float32))
    assert np.array_equal(top1.cpu().numpy().reshape(-1), z["top1"].reshape(-1)), "top-1 index (pad rows: 0)"
    want = torch.from_numpy(z["router_probs"]).reshape(b * s, e)
    got = router_probs.float().cpu().reshape(b * s, e)
    assert torch.equal(got != 0, want != 0), "router_probs: routed pairs, pad rows all zero"
    assert torch.allclose(got, want, rtol=0, atol=2 ** -7), "router_probs values"
    eng.close()
