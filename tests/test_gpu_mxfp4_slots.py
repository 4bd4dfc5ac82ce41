"""MXFP4 slots (moeinf_create_ex, slot_dtype = MOEINF_SLOT_MXFP4; EngineConfig.mxfp4_slots): the routed experts are OCP MXFP4 — e2m1
codes, one e8m0 scale per 32 k — in the host tier, on the link and in their HBM slots, and the FFN kernels up-cast them in registers
(v_cvt_scalef32_pk_bf16_fp4).  e2m1 x 2^n is exact in bf16, so every result must equal the oracle run on the dequantised weights,
y = FFN(x; dequant(W).to(bf16)), under the usual bf16 bars, routing bit-exact — with weights that hold every code under a spread of
scale bytes, so a wrong conversion, nibble order or scale position shows as a parity miss.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest
import torch

from helpers import R, acts, assert_block_close, assert_model_close, make_weights, oracle_expert_rows, register_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = list(range(115, 130))  # 2^-12 .. 2^2: around the scales N(0, 0.02^2)-like weights quantise to


def _every_code_and_scale(codes, scales, salt):
    """copies with, for every (code, scale byte) pair, at least one whole block — all 32 elements the code, the block's scale the
    byte — written at spread positions (a different row and block for every pair where the matrix has the room)"""
    codes, scales = codes.clone(), scales.clone()
    rows, nblk = scales.shape
    i = 0
    for sb in SCALES:
        for c in range(16):
            r, b = (i * 7 + salt) % rows, (i * 5 + 3 * salt) % nblk
            codes[r, 16 * b:16 * b + 16] = c | (c << 4)
            codes[r, 16 * b + (i % 16)] = c | (((c + 5) & 15) << 4)  # ... and a byte whose two nibbles differ (their order matters)
            scales[r, b] = sb
            i += 1
    return codes, scales


def _mx_weights(family, h, f, e, seed, n_shared=0):
    """(gate, per expert [(codes, scales), ...], per expert dequantised bf16 tensors, bf16 shared expert or None)"""
    from moe_infinity_amd.quant import mxfp4_dequantize, mxfp4_quantize

    gate, experts, shared = make_weights(family, h, f, e, seed, torch.bfloat16, n_shared=n_shared)
    packed, deq = [], []
    for i, ts in enumerate(experts):
        ps = [_every_code_and_scale(*mxfp4_quantize(w.float()), salt=3 * i + j) for j, w in enumerate(ts)]
        ds = []
        for c, s in ps:
            d32 = mxfp4_dequantize(c, s, torch.float32)
            d = mxfp4_dequantize(c, s)  # bf16
            assert bool(torch.isfinite(d32).all()) and torch.equal(d.float(), d32), "the dequantised weights are bf16-exact and finite"
            ds.append(d)
        packed.append(ps)
        deq.append(ds)
    # (every pair is there: checked once, on the first matrix)
    c0, s0 = packed[0][0]
    lo = (c0 & 15).reshape(c0.shape[0], -1, 16)
    seen = {(int(c), int(s)) for c, s in zip(lo[:, :, 1].reshape(-1).tolist(), s0.reshape(-1).tolist())}
    assert all((c, sb) in seen for c in range(16) for sb in SCALES)
    return gate, packed, deq, shared


def _engine(family, h, f, e, k, mxfp4=True, n_shared=0, max_tokens=64, **kw):
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    et = {"mixtral": Cf.EXPERT_MIXTRAL, "deepseek": Cf.EXPERT_DEEPSEEK}[family]
    rk = {"mixtral": Cf.ROUTER_MIXTRAL, "deepseek": Cf.ROUTER_DEEPSEEK}[family]
    base = dict(num_layers=1, num_experts=e, expert_type=et, hidden=h, inter=f, top_k=k, router_kind=rk, dtype=Cf.DTYPE_BF16,
                gate_dtype=Cf.DTYPE_BF16, shared_inter=f * n_shared, device_memory_ratio=0.5, max_tokens=max_tokens, mxfp4_slots=mxfp4)
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
    ("mixtral", 256, 512, 8, 2, 0, 200, "mixtral"), ("deepseek", 256, 256, 16, 4, 2, 1, "deepseek"), ("deepseek", 256, 256, 16, 4, 2, 5, "deepseek"),
    ("deepseek", 256, 256, 16, 4, 2, 1, "deepseek_v3"), ("mixtral", 256, 512, 8, 2, 0, 1, "grok"),
    # reductions of real sizes and odd tile counts.  h = 384: 3 k-tiles per row group (scale dwords that start inside a dword, shifts
    # 1..3).  h = 4096, f = 1152: two code units per source row in the tier mover, eight / ten scale units per tensor with a short
    # last one (f's 9 tiles: 28 row groups per unit, 256 row groups), several batches per wave and work for every wave in the k-loop.
    # DeepSeek-V2-Lite's widths: 11 tiles in stage 2.
    ("mixtral", 384, 512, 8, 2, 0, 1, "mixtral"), ("mixtral", 384, 512, 8, 2, 0, 40, "mixtral"),
    ("mixtral", 4096, 1152, 4, 2, 0, 1, "mixtral"), ("mixtral", 4096, 1152, 4, 2, 0, 3, "mixtral"), ("mixtral", 4096, 1152, 4, 2, 0, 40, "mixtral"),
    ("deepseek", 2048, 1408, 8, 4, 1, 1, "deepseek"), ("deepseek", 2048, 1408, 8, 4, 1, 40, "deepseek")],
    ids=["mixtral_t1_selfroute_pair", "mixtral_t4_multi", "mixtral_t40_many_rows", "mixtral_t200_many_rows", "deepseek_t1_front1_decode1",
         "deepseek_t5", "deepseek_v3_router_t1", "grok_router_t1", "h384_three_tiles_t1", "h384_three_tiles_t40", "h4096_f1152_t1",
         "h4096_f1152_t3_multi", "h4096_f1152_t40", "deepseek_v2_lite_widths_t1", "deepseek_v2_lite_widths_t40"])
def test_mxfp4_slots_equal_the_oracle_on_dequantised_weights(family, h, f, e, k, n_shared, t, router):
    from moe_infinity_amd import config as Cf

    gate, packed, deq, shared = _mx_weights(family, h, f, e, 9700 + t, n_shared)
    kw, gate_kw = {}, {}
    if router == "deepseek_v3":
        kw = dict(router_kind=Cf.ROUTER_DEEPSEEK_V3, n_group=4, topk_group=2, norm_topk_prob=True, routed_scaling_factor=2.5)
        gate_kw = dict(e_bias=torch.linspace(-0.05, 0.05, e), n_group=4, topk_group=2, norm_topk_prob=True, routed_scaling_factor=2.5)
    elif router == "grok":
        kw = dict(router_kind=Cf.ROUTER_SOFTMAX_TOPK)
    eng = _engine(family, h, f, e, k, n_shared=n_shared, max_tokens=t, **kw)
    assert eng.slot_dtype == Cf.SLOT_MXFP4
    if router == "deepseek_v3":
        eng.set_gate_bias(0, gate_kw["e_bias"].to(DEV, torch.float32).contiguous())
    register_all(eng, packed, shared)
    x = acts(t, h, torch.bfloat16, 9800 + t)
    if family == "mixtral":
        ref = (R.block_grok if router == "grok" else R.block_mixtral)(x[None], gate, deq, top_k=k)
    else:
        ref = R.block_deepseek(x[None], gate, deq, k, shared=shared, **gate_kw)
    for rnd in range(2):  # misses (the decision path), then hits (the sync-free path)
        out = eng.forward(0, x.to(DEV), gate.to(DEV))
        _routing_exact(eng, ref, sets=family == "deepseek")
        assert_block_close(out, ref, torch.bfloat16, f"round {rnd}: MXFP4 slots vs the oracle on dequantised weights")
        st = eng.stats()
        assert (st["expert_misses"] > 0) if rnd == 0 else (st["expert_hits"] > 0)
    rows = oracle_expert_rows(ref, e)
    assert_model_close(eng.expert_outputs(rows.shape[0]), rows, torch.bfloat16, "expert FFN outputs")
    eng.close()


def test_mxfp4_slots_dispatch_mask():
    """the drop-in path (moeinf_dispatch_mask): the caller's router_mask, expert-sorted rows out"""
    h, f, e, k, t = 256, 512, 8, 2, 6
    gate, packed, deq, _ = _mx_weights("mixtral", h, f, e, 9900)
    eng = _engine("mixtral", h, f, e, k, max_tokens=t)
    register_all(eng, packed)
    x = acts(t, h, torch.bfloat16, 9901)
    ref = R.block_mixtral(x[None], gate, deq, top_k=k)
    y, counts, _hit = eng.dispatch_mask(0, x.to(DEV), ref.router_mask.to(DEV))
    rows = oracle_expert_rows(ref, e)
    assert int(counts.sum()) == rows.shape[0]
    assert_model_close(y[: rows.shape[0]].cpu(), rows, torch.bfloat16, "dispatch_mask rows, MXFP4 slots")
    eng.close()


@pytest.mark.parametrize("t", [1, 40], ids=["decode_b1", "t40"])
def test_mxfp4_slots_against_a_bf16_engine_on_the_dequantised_weights_and_capacity(t):
    """The same experts as MXFP4 slots and, dequantised, in a bf16 engine with the same byte budget: the same results within the bf16
    bars, slot bytes as the layout gives them (68 KiB against 256 KiB per matrix here), one MXFP4 host blob on the link per miss."""
    from moe_infinity_amd import config as Cf

    h, f, e, k, L = 256, 512, 8, 2, 4
    gate, packed, deq, _ = _mx_weights("mixtral", h, f, e, 10000)
    x = acts(t, h, torch.bfloat16, 10001)
    res = {}
    # eight bf16 slots = 30.1 MXFP4 slots of the 32 experts registered (whole slots: with six, 22.6 floors to 22 = 3.67 x)
    budget = 8 * 3 * f * h * 2
    for mx in (False, True):
        eng = _engine("mixtral", h, f, e, k, mxfp4=mx, max_tokens=t, num_layers=L, device_memory_bytes=budget)
        for layer in range(L):
            register_all(eng, packed if mx else deq, layer=layer)
        outs = [eng.forward(layer, x.to(DEV), gate.to(DEV)).cpu() for layer in range(L)]
        ref = R.block_mixtral(x[None], gate, deq, top_k=k)
        rows = eng.expert_outputs(oracle_expert_rows(ref, e).shape[0])
        res[mx] = dict(outs=outs, rows=rows, st=eng.stats(), slot_dtype=eng.slot_dtype, lay=eng.expert_layout(0))
        eng.close()
    a, b = res[False], res[True]
    assert a["slot_dtype"] == Cf.DTYPE_BF16 and b["slot_dtype"] == Cf.SLOT_MXFP4
    for oa, ob in zip(a["outs"], b["outs"]):
        assert_model_close(ob, oa, torch.bfloat16, "MXFP4 slots vs bf16 slots, block output")
    assert_model_close(b["rows"], a["rows"], torch.bfloat16, "MXFP4 slots vs bf16 slots, expert FFN rows")
    sa, sb = a["st"], b["st"]
    # per matrix [R, K]: R/16 x K/128 code tiles of 1 KiB, then one scale dword per lane and four tiles; each padded to 4 KiB
    def mat(r, kk):
        tiles = (r // 16) * (kk // 128)
        return -(-(tiles * 1024 + -(-tiles // 4) * 256) // 4096) * 4096
    assert sb["slot_bytes"] == mat(f, h) + mat(h, f) + mat(f, h) == 3 * 68 * 1024
    assert sb["slot_bytes"] <= 0.27 * sa["slot_bytes"], (sa["slot_bytes"], sb["slot_bytes"])
    assert sb["slots_total"] >= 3.7 * sa["slots_total"], (sa["slots_total"], sb["slots_total"])
    off, siz, tot = b["lay"]
    assert siz == [f * h // 2 + f * h // 32] * 3 and len(off) == 3, "one tensor per matrix: codes, then scales"
    assert sb["expert_misses"] > 0
    per_miss = sb["h2d_bytes"] / sb["expert_misses"]
    assert sum(siz) <= per_miss <= tot, ("one MXFP4 host blob per miss", per_miss, b["lay"])


def test_mxfp4_slots_under_pressure_cache_budget_changes_and_a_masked_forward():
    h, f, e, k, t = 256, 512, 8, 2, 3
    gate, packed, deq, _ = _mx_weights("mixtral", h, f, e, 10100)
    probe = _engine("mixtral", h, f, e, k, max_tokens=t)
    slot = probe.stats()["slot_bytes"]
    probe.close()
    eng = _engine("mixtral", h, f, e, k, max_tokens=t, device_memory_bytes=3 * slot)
    assert eng.stats()["slots_total"] == 3
    register_all(eng, packed)
    for step in range(20):
        if step == 10:
            eng.set_cache_budget(2 * slot)
        if step == 14:
            eng.set_cache_budget(8 * slot)
        x = acts(t, h, torch.bfloat16, 10200 + step)
        g = gate if step % 2 == 0 else gate.flip(0)  # changing routing
        out = eng.forward(0, x.to(DEV), g.to(DEV))
        ref = R.block_mixtral(x[None], g, deq, top_k=k)
        _routing_exact(eng, ref)
        assert_block_close(out, ref, torch.bfloat16, f"step {step}")
    st = eng.stats()
    assert st["evictions"] > 0 and st["expert_misses"] > 3
    # one masked forward (the generic launches): the middle token is padding
    x = acts(t, h, torch.bfloat16, 10300)
    mask = torch.tensor([True, False, True])
    out = eng.forward(0, x.to(DEV), gate.to(DEV), token_mask=mask.to(DEV))
    ref = R.block_mixtral(x[mask][None], gate, deq, top_k=k)  # the oracle block on the real tokens; a masked Mixtral row is 0
    assert_block_close(out.cpu()[mask], ref, torch.bfloat16, "masked forward, MXFP4 slots")
    assert bool((out.cpu()[~mask] == 0).all())
    eng.close()


def test_mxfp4_slots_through_an_offload_directory_equal_the_resident_run(tmp_path):
    """host_memory_bytes below the expert bytes: the MXFP4 blobs come back from the offload store; bit for bit the resident run"""
    from moe_infinity_amd.offload_store import OffloadStore

    h, f, e, k, t = 256, 512, 8, 2, 3
    gate, packed, deq, _ = _mx_weights("mixtral", h, f, e, 10400)
    xs = [acts(t, h, torch.bfloat16, 10500 + i) for i in range(6)]
    outs = {}
    for mode in ("resident", "store"):
        if mode == "resident":
            eng = _engine("mixtral", h, f, e, k, max_tokens=t)
            register_all(eng, packed)
        else:
            probe = _engine("mixtral", h, f, e, k, max_tokens=t)
            off, siz, tot = probe.expert_layout(0)
            slot = probe.stats()["slot_bytes"]
            store = OffloadStore(str(tmp_path))
            ids, tid = {}, 10
            for ex in range(e):  # one tensor per matrix: its codes followed by its scales, as the host blob holds them
                blob = probe.pack_expert(packed[ex])
                ids[ex] = []
                for o, s in zip(off, siz):
                    store.offload(blob[o:o + s].clone(), tid)
                    ids[ex].append(tid)
                    tid += 1
            probe.close()
            store.close()
            store = OffloadStore(str(tmp_path))
            eng = _engine("mixtral", h, f, e, k, max_tokens=t, device_memory_bytes=3 * slot, host_memory_bytes=3 * tot)
            for ex in range(e):
                store.register_expert(eng, 0, ex, ids[ex])
        outs[mode] = [eng.forward(0, x.to(DEV), (gate if i % 2 == 0 else gate.flip(0)).to(DEV)).cpu() for i, x in enumerate(xs)]
        eng.close()
    for a, b in zip(outs["resident"], outs["store"]):
        assert torch.equal(a, b), "an expert that came back from the offload directory computes the same bits"
