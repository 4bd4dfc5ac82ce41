"""fp8 slots (moeinf_create_ex, slot_dtype = MOEINF_DTYPE_F8E4M3; EngineConfig.fp8_slots): fp8 experts stay e4m3fn in their HBM
slots and the FFN kernels up-cast them in registers (v_cvt_scalef32_pk_bf16_fp8).  The arithmetic is the bf16 engine's, so every
result must equal the oracle run on the up-cast weights, y = FFN(x; W.to(bf16)), under the usual bars, routing bit-exact — with
weights that hold every finite e4m3fn code, so a wrong conversion shows as a parity miss.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest
import torch

from helpers import (R, acts, assert_as_accurate_as_the_oracle, assert_block_close, assert_model_close, make_weights, oracle_expert_rows,
                     register_all)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn


def _every_code(w8, salt):
    """fp8 copy of w8 with the 254 finite e4m3fn codes (subnormals, +-0, +-448) written at spread positions, at most one per row
    where the matrix has the rows for it"""
    codes = torch.arange(256, dtype=torch.int32)
    codes = codes[(codes & 0x7F) != 0x7F].to(torch.uint8)
    q = w8.clone()
    u = q.view(torch.uint8)
    rows, cols = u.shape
    for i, c in enumerate(codes.tolist()):
        u[(i * 7 + salt) % rows, (i * 13 + 5 * salt) % cols] = c
    return q


def _fp8_weights(family, h, f, e, seed, n_shared=0):
    gate, experts, shared = make_weights(family, h, f, e, seed, torch.bfloat16, n_shared=n_shared)
    ex8 = [[_every_code(w.to(F8), 3 * i + j) for j, w in enumerate(ts)] for i, ts in enumerate(experts)]
    sh8 = [w.to(F8) for w in shared] if shared else None
    return gate, ex8, sh8


def _up(ts):
    return [w.to(torch.bfloat16) for w in ts] if ts else None


def _engine(family, h, f, e, k, fp8_slots=True, n_shared=0, max_tokens=64, **kw):
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    et = {"mixtral": Cf.EXPERT_MIXTRAL, "deepseek": Cf.EXPERT_DEEPSEEK}[family]
    rk = {"mixtral": Cf.ROUTER_MIXTRAL, "deepseek": Cf.ROUTER_DEEPSEEK}[family]
    base = dict(num_layers=1, num_experts=e, expert_type=et, hidden=h, inter=f, top_k=k, router_kind=rk, dtype=Cf.DTYPE_F8E4M3,
                gate_dtype=Cf.DTYPE_BF16, shared_inter=f * n_shared, device_memory_ratio=0.5, max_tokens=max_tokens, fp8_slots=fp8_slots)
    base.update(kw)
    return MoEEngine(Cf.EngineConfig(**base))


def _routing_exact(eng, ref, sets=False):
    idx = eng.routing()["topk_idx"]
    if sets:
        assert [sorted(int(v) for v in r) for r in idx] == [sorted(int(v) for v in r) for r in ref.topk_idx.numpy()], "routing sets must be bit-exact"
    else:
        assert np.array_equal(idx, ref.topk_idx.numpy().astype(np.int32)), "routing indices must be bit-exact"


@pytest.mark.parametrize("family,h,f,e,k,n_shared,t,router", [
    ("mixtral", 256, 512, 8, 2, 0, 1, "mixtral"), ("mixtral", 256, 512, 8, 2, 0, 4, "mixtral"), ("mixtral", 256, 512, 8, 2, 0, 40, "mixtral"),
    ("mixtral", 256, 512, 8, 2, 0, 200, "mixtral"), ("deepseek", 256, 192, 16, 4, 2, 1, "deepseek"), ("deepseek", 256, 192, 16, 4, 2, 5, "deepseek"),
    ("deepseek", 256, 192, 16, 4, 2, 1, "deepseek_v3"), ("mixtral", 256, 512, 8, 2, 0, 1, "grok")],
    ids=["mixtral_t1_selfroute_pair", "mixtral_t4_multi", "mixtral_t40_many_rows", "mixtral_t200_many_rows", "deepseek_t1_front1_decode1",
         "deepseek_t5", "deepseek_v3_router_t1", "grok_router_t1"])
def test_fp8_slots_equal_the_oracle_on_upcast_weights(family, h, f, e, k, n_shared, t, router):
    from moe_infinity_amd import config as Cf

    gate, ex8, sh8 = _fp8_weights(family, h, f, e, 9100 + t, n_shared)
    kw, gate_kw = {}, {}
    if router == "deepseek_v3":
        kw = dict(router_kind=Cf.ROUTER_DEEPSEEK_V3, n_group=4, topk_group=2, norm_topk_prob=True, routed_scaling_factor=2.5)
        gate_kw = dict(e_bias=torch.linspace(-0.05, 0.05, e), n_group=4, topk_group=2, norm_topk_prob=True, routed_scaling_factor=2.5)
    elif router == "grok":
        kw = dict(router_kind=Cf.ROUTER_SOFTMAX_TOPK)
    eng = _engine(family, h, f, e, k, n_shared=n_shared, max_tokens=t, **kw)
    assert eng.slot_dtype == Cf.DTYPE_F8E4M3
    if router == "deepseek_v3":
        bias = gate_kw["e_bias"].to(DEV, torch.float32).contiguous()
        eng.set_gate_bias(0, bias)
    register_all(eng, ex8, sh8)
    x = acts(t, h, torch.bfloat16, 9200 + t)
    up = [_up(ts) for ts in ex8]
    if family == "mixtral":
        ref = (R.block_grok if router == "grok" else R.block_mixtral)(x[None], gate, up, top_k=k)
    else:
        ref = R.block_deepseek(x[None], gate, up, k, shared=_up(sh8), **gate_kw)
    for rnd in range(2):  # misses (the decision path), then hits (the sync-free path)
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
        _routing_exact(eng, ref, sets=family == "deepseek")
        assert_block_close(out, ref, torch.bfloat16, f"round {rnd}: fp8 slots vs the oracle on up-cast weights")
        st = eng.stats()
        assert (st["expert_misses"] > 0) if rnd == 0 else (st["expert_hits"] > 0)
    rows = oracle_expert_rows(ref, e)
    assert_model_close(eng.expert_outputs(rows.shape[0]), rows, torch.bfloat16, "expert FFN outputs")
    eng.close()


@pytest.mark.parametrize("t", [1, 40], ids=["decode_b1", "t40"])
def test_fp8_slots_against_the_bf16_slot_fp8_engine_and_capacity(t):
    """The same fp8 experts through today's fp8 engine (bf16 slots, up-cast by the pull kernel) and through fp8 slots, with the
    same byte budget: the same results within the bf16 bars, about twice the slots at half the bytes, the same link bytes."""
    from moe_infinity_amd import config as Cf

    h, f, e, k, L = 256, 512, 8, 2, 4
    gate, ex8, _ = _fp8_weights("mixtral", h, f, e, 9300)
    x = acts(t, h, torch.bfloat16, 9301)
    res = {}
    budget = None
    for fp8_slots in (False, True):
        eng = _engine("mixtral", h, f, e, k, fp8_slots=fp8_slots, max_tokens=t, num_layers=L,
                      device_memory_bytes=budget or 6 * 3 * f * h * 2)  # six bf16 slots
        budget = eng.cfg.device_memory_bytes
        for layer in range(L):
            register_all(eng, ex8, layer=layer)
        outs = [eng.forward(layer, x.to(DEV), gate.to(DEV)).cpu() for layer in range(L)]
        ref = R.block_mixtral(x[None], gate, [_up(ts) for ts in ex8], top_k=k)
        rows = eng.expert_outputs(oracle_expert_rows(ref, e).shape[0])
        res[fp8_slots] = dict(outs=outs, rows=rows, st=eng.stats(), slot_dtype=eng.slot_dtype, lay=eng.expert_layout(0))
        eng.close()
    a, b = res[False], res[True]
    assert a["slot_dtype"] == Cf.DTYPE_BF16 and b["slot_dtype"] == Cf.DTYPE_F8E4M3
    for oa, ob in zip(a["outs"], b["outs"]):
        assert_model_close(ob, oa, torch.bfloat16, "fp8 slots vs bf16 slots, block output")
    assert_model_close(b["rows"], a["rows"], torch.bfloat16, "fp8 slots vs bf16 slots, expert FFN rows")
    sa, sb = a["st"], b["st"]
    assert sb["slots_total"] >= 1.9 * sa["slots_total"], (sa["slots_total"], sb["slots_total"])
    assert sb["slot_bytes"] <= 0.52 * sa["slot_bytes"], (sa["slot_bytes"], sb["slot_bytes"])
    assert a["lay"] == b["lay"], "the HOST blob layout is the same in both modes"
    assert sb["expert_misses"] == sa["expert_misses"] > 0 and sb["h2d_bytes"] == sa["h2d_bytes"], "the same fp8 host blobs on the link"
    per_miss = sb["h2d_bytes"] / sb["expert_misses"]
    assert sum(b["lay"][1]) <= per_miss <= b["lay"][2], ("one fp8 host blob per miss", per_miss, b["lay"])


def test_fp8_slots_offload_under_pressure_and_cache_budget_changes():
    h, f, e, k, t = 256, 512, 8, 2, 3
    gate, ex8, _ = _fp8_weights("mixtral", h, f, e, 9400)
    up = [_up(ts) for ts in ex8]
    probe = _engine("mixtral", h, f, e, k, max_tokens=t)
    slot = probe.stats()["slot_bytes"]
    probe.close()
    eng = _engine("mixtral", h, f, e, k, max_tokens=t, device_memory_bytes=3 * slot)
    assert eng.stats()["slots_total"] == 3
    register_all(eng, ex8)
    for step in range(20):
        if step == 10:
            eng.set_cache_budget(2 * slot)
        if step == 14:
            eng.set_cache_budget(8 * slot)
        x = acts(t, h, torch.bfloat16, 9500 + step)
        g = gate if step % 2 == 0 else gate.flip(0)  # changing routing
        out = eng.forward(0, x.to(DEV), g.to(DEV))
        ref = R.block_mixtral(x[None], g, up, top_k=k)
        _routing_exact(eng, ref)
        assert_block_close(out, ref, torch.bfloat16, f"step {step}")
    st = eng.stats()
    assert st["evictions"] > 0 and st["expert_misses"] > 3
    eng.close()


def test_fp8_slots_dispatch_mask():
    """the drop-in path (moeinf_dispatch_mask): the caller's router_mask, expert-sorted rows out"""
    h, f, e, k, t = 256, 512, 8, 2, 6
    gate, ex8, _ = _fp8_weights("mixtral", h, f, e, 9600)
    eng = _engine("mixtral", h, f, e, k, max_tokens=t)
    register_all(eng, ex8)
    x = acts(t, h, torch.bfloat16, 9601)
    ref = R.block_mixtral(x[None], gate, [_up(ts) for ts in ex8], top_k=k)
    y, counts, _hit = eng.dispatch_mask(0, x.to(DEV), ref.router_mask.to(DEV))
    rows = oracle_expert_rows(ref, e)
    assert int(counts.sum()) == rows.shape[0]
    assert_model_close(y[: rows.shape[0]].cpu(), rows, torch.bfloat16, "dispatch_mask rows, fp8 slots")
    eng.close()


@pytest.mark.parametrize("what", ["bf16_dtype", "nllb", "ep_size_2", "hidden_not_multiple_of_64"])
def test_fp8_slots_refusals(what):
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf
    from moe_infinity_amd._lib import MoeInfError

    base = dict(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2, router_kind=Cf.ROUTER_MIXTRAL,
                dtype=Cf.DTYPE_F8E4M3, gate_dtype=Cf.DTYPE_BF16, device_memory_ratio=0.5, max_tokens=8, fp8_slots=True)
    base.update({"bf16_dtype": dict(dtype=Cf.DTYPE_BF16),
                 "nllb": dict(expert_type=Cf.EXPERT_NLLB, router_kind=Cf.ROUTER_NLLB),
                 "ep_size_2": dict(ep_size=2),
                 "hidden_not_multiple_of_64": dict(hidden=224)}[what])
    with pytest.raises(MoeInfError, match="fp8 slots"):
        MoEEngine(Cf.EngineConfig(**base))


def _fill_fp8_layer(eng, shapes, seed, std=0.02):
    """N(0, std^2) weights rounded to e4m3fn, generated on the GPU into the engine's pinned arena; bf16 up-casts for the oracle"""
    off, siz, tot = eng.expert_layout(0)
    g = torch.Generator(device=DEV)
    experts = []
    for ex in range(eng.cfg.num_experts):
        eng.register_expert(0, ex, None)
        g.manual_seed(seed + ex)
        raw = eng.expert_host_view(0, ex)
        ts = []
        for o, s, sh in zip(off, siz, shapes):
            w8 = torch.empty(sh, device=DEV).normal_(0.0, std, generator=g).to(F8)
            raw[o:o + s].copy_(w8.view(torch.uint8).reshape(-1))
            ts.append(w8.to(torch.bfloat16).cpu())
        experts.append(ts)
    shared = None
    if eng.cfg.shared_inter:
        h, fs = eng.cfg.hidden, eng.cfg.shared_inter
        g.manual_seed(seed + 9999)
        sh8 = [torch.empty(sh, device=DEV).normal_(0.0, std, generator=g).to(F8).cpu() for sh in [(fs, h), (fs, h), (h, fs)]]
        eng.register_shared(0, sh8)
        shared = _up(sh8)
    torch.cuda.synchronize()
    return experts, shared


@pytest.mark.parametrize("family,t", [("mixtral", 1), ("mixtral", 512), ("deepseek", 1), ("deepseek", 512)],
                         ids=["mixtral_8x7b_b1", "mixtral_8x7b_t512", "deepseek_v2_lite_b1", "deepseek_v2_lite_t512"])
def test_fp8_slots_full_size_layer(family, t):
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    cfg = (Cf.mixtral_8x7b if family == "mixtral" else Cf.deepseek_v2_lite)(dtype=Cf.DTYPE_F8E4M3, gate_dtype=Cf.DTYPE_BF16, max_tokens=t,
                                                                             fp8_slots=True)
    cfg.num_layers = 1
    eng = MoEEngine(cfg)
    h, f = cfg.hidden, cfg.inter
    shapes = [(f, h), (h, f), (f, h)] if family == "mixtral" else [(f, h), (f, h), (h, f)]
    experts, shared = _fill_fp8_layer(eng, shapes, 5000 if family == "mixtral" else 6000)
    gate = (torch.randn(cfg.num_experts, h, generator=torch.Generator().manual_seed(77)) * 0.02).to(torch.bfloat16)
    x = acts(t, h, torch.bfloat16, 78)
    for _ in range(2):  # misses, then the sync-free path
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
    if family == "mixtral":
        ref = R.block_mixtral(x[None], gate, experts, top_k=cfg.top_k)
    else:
        ref = R.block_deepseek(x[None], gate, experts, cfg.top_k, shared=shared)
    _routing_exact(eng, ref, sets=family == "deepseek")
    rows = oracle_expert_rows(ref, cfg.num_experts)
    got_rows = eng.expert_outputs(rows.shape[0])
    # the fp32-exact arm first (as test_gpu_fullsize.py): over the same rows the GPU is as close to the fp32 computation as the oracle
    # is, so what the row bar sees are last-bit flips carried through the gated epilogue's three rounding points (the fp8 form sums
    # k in another order than the bf16 kernels: 13 M DeepSeek rows at 512 tokens show single elements at 1.3 ulp), not lost precision
    acc = assert_as_accurate_as_the_oracle(out, ref, family, x[None], experts, torch.bfloat16, f"{family} layer, {t} tokens, fp8 slots",
                                           shared=shared, rows=got_rows)
    assert_model_close(got_rows, rows, torch.bfloat16, f"expert FFN outputs (fp32-exact arm over these rows: ratio {acc['rows']['ratio']:.4f})",
                       ulps=1.0 if t == 1 else 1.5)
    assert_block_close(out, ref, torch.bfloat16, f"{family} layer, {t} tokens, fp8 slots")
    eng.close()
