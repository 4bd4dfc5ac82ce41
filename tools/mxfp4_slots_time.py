#!/usr/bin/env python3
"""MXFP4 slots (EngineConfig.mxfp4_slots; mxfp4-gemm: with EngineConfig.mxfp4_gemm, the MXFP4 grouped GEMMs switched on) against bf16
slots and fp8 slots, A/B/C/D/A/B/C/D, every run in a process of its own.  Legs:

    decode-mixtral     Mixtral-8x7B, 32 layers resident, batch 1: ms/token
    decode-deepseek    DeepSeek-V2-Lite, 26 layers resident, batch 1: ms/token
    miss-mixtral       Mixtral-8x7B, 16 layers, device_memory_bytes = 50 % of the layers' bf16 expert bytes, changing routing:
                       hit rate once warm, ms/token, link GB/s and the time misses x blob bytes / link rate would take
    tight-mixtral      the same with a budget of 10 % of the bf16 expert bytes (no format fits)
    prefill-mixtral    Mixtral-8x7B, 8 layers resident, 64 / 512 tokens (--tokens): ms per layer
    prefill-deepseek   DeepSeek-V2-Lite, 8 layers resident, 64 / 512 tokens (--tokens): ms per layer

    python tools/mxfp4_slots_time.py [--tokens N,...] [--slots bf16,fp8,mxfp4,mxfp4-gemm] [--rounds N] [--trees DIR,...] [leg ...]
        (default: every leg, every slot kind; one JSON line per run, then a summary.  --trees: the same runs against the library of
        each of these checkouts in turn — e.g. the parent commit and this one; a tree without MXFP4 slots runs bf16 and fp8 only, one
        without the MXFP4 grouped GEMMs not mxfp4-gemm)
    python tools/mxfp4_slots_time.py --child <leg> <bf16|fp8|mxfp4|mxfp4-gemm> [--steps N] [--tokens N] [--tree DIR]   (one run; used by the
        above and under rocprofv3)
The expert bytes are random: fp8 blobs N(0, 0.02^2) rounded to e4m3fn, MXFP4 blobs random codes with scale bytes 115..129 (any
codes and in-contract scales cost the same), bf16 blobs N(0, 0.02^2)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["decode-mixtral", "decode-deepseek", "miss-mixtral", "tight-mixtral", "prefill-mixtral", "prefill-deepseek"]
KINDS = ["bf16", "fp8", "mxfp4", "mxfp4-gemm"]


def child(leg, kind, steps, tokens=512, tree=ROOT):
    sys.path.insert(0, tree)
    import torch
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    wl = "mixtral" if "mixtral" in leg else "deepseek"
    T = tokens if leg.startswith("prefill") else 1
    mk = Cf.mixtral_8x7b if wl == "mixtral" else Cf.deepseek_v2_lite
    kw = dict(gate_dtype=Cf.DTYPE_BF16, max_tokens=T, device_memory_ratio=0.8)
    if kind == "fp8":
        cfg = mk(dtype=Cf.DTYPE_F8E4M3, fp8_slots=True, **kw)
    elif kind == "mxfp4":
        cfg = mk(dtype=Cf.DTYPE_BF16, mxfp4_slots=True, **kw)
    elif kind == "mxfp4-gemm":
        cfg = mk(dtype=Cf.DTYPE_BF16, mxfp4_slots=True, mxfp4_gemm=True, **kw)
    else:
        cfg = mk(dtype=Cf.DTYPE_BF16, **kw)
    pressure = leg in ("miss-mixtral", "tight-mixtral")
    if pressure:
        cfg.num_layers = 16
        slot16 = 3 * cfg.hidden * cfg.inter * 2  # bf16 slot bytes (4 KiB multiples for these shapes)
        cfg.device_memory_bytes = cfg.num_layers * cfg.num_experts * slot16 // (2 if leg == "miss-mixtral" else 10)
    elif leg.startswith("prefill"):
        cfg.num_layers = 8
    L, E, dev = cfg.num_layers, cfg.num_experts, torch.device("cuda:0")
    eng = MoEEngine(cfg)
    off, siz, tot = eng.expert_layout(0)
    g = torch.Generator(device=dev)
    for l in range(L):
        for e in range(E):
            eng.register_expert(l, e, None)
            g.manual_seed(1000 * l + e)
            view = eng.expert_host_view(l, e)
            if kind == "fp8":
                view.copy_(torch.empty(tot, device=dev).normal_(0.0, 0.02, generator=g).to(torch.float8_e4m3fn).view(torch.uint8))
            elif kind.startswith("mxfp4"):
                # every byte a pair of random codes; then the scale bytes of every tensor (its last 1/17) into the contract's range
                view.copy_(torch.randint(0, 256, (tot,), device=dev, generator=g, dtype=torch.uint8))
                for o, s in zip(off, siz):
                    ns = s // 17
                    view[o + s - ns:o + s].copy_(torch.randint(115, 130, (ns,), device=dev, generator=g, dtype=torch.uint8))
            else:
                view.view(torch.bfloat16).copy_(torch.empty(tot // 2, device=dev).normal_(0.0, 0.02, generator=g).to(torch.bfloat16))
        if cfg.shared_inter:
            _, sizs, _ = eng.expert_layout(1)
            es = 1 if kind == "fp8" else 2
            sh = [torch.empty(s // es, dtype=torch.float32).normal_(0.0, 0.02) for s in sizs]
            eng.register_shared(l, [t.to(torch.float8_e4m3fn) if kind == "fp8" else t.to(torch.bfloat16) for t in sh])
        eng.prefetch(l, list(range(E)))  # (pressure legs: every expert once, so the cache starts warm — what it holds is the policy's choice)
    eng.sync_copies()
    torch.cuda.synchronize()
    gates = [(torch.randn(E, cfg.hidden, device=dev) * 0.02).to(torch.bfloat16) for _ in range(L)]
    xs = [(torch.randn(T, cfg.hidden, device=dev)).to(torch.bfloat16) for _ in range(8)]
    out = torch.empty(T, cfg.hidden, dtype=torch.bfloat16, device=dev)
    res = dict(leg=leg, slots=kind, blob_bytes=tot)
    if pressure:
        def token(i):
            for l in range(L):
                eng.forward(l, xs[(i + l) % 8], gates[(i * 7 + l) % L], out=out)
        for i in range(L):  # warm: the cache settles under the changing routing
            token(i)
        torch.cuda.synchronize()
        s0 = eng.stats()
        t0 = time.perf_counter()
        for i in range(steps):
            token(L + i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        s1 = eng.stats()
        hits, miss = s1["expert_hits"] - s0["expert_hits"], s1["expert_misses"] - s0["expert_misses"]
        h2d = s1["h2d_bytes"] - s0["h2d_bytes"]
        res.update(ms_per_token=round(dt * 1e3, 3), hit_rate=round(hits / max(1, hits + miss), 4), misses_per_token=round(miss / steps, 2),
                   link_gbs=round(h2d / steps / dt / 1e9, 2), slots_total=s1["slots_total"], slot_bytes=s1["slot_bytes"])
    else:
        iters = steps * L
        for i in range(2 * L):
            eng.forward(i % L, xs[i % 8], gates[i % L], out=out)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            for i in range(iters):
                eng.forward(i % L, xs[i % 8], gates[i % L], out=out)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / iters)
        st = eng.stats()
        if leg.startswith("decode"):
            res.update(ms_per_token=round(best * L * 1e3, 4), layers=L)
        else:
            res.update(ms_per_layer=round(best * 1e3, 4), tokens=T)
            if hasattr(eng, "last_ffn_forms"):  # the kernels the last forward's two stages took (moeinf_ffn_form's ids)
                res.update(ffn_forms=list(eng.last_ffn_forms()))
        res.update(slots_total=st["slots_total"], slot_bytes=st["slot_bytes"], misses_measured=st["expert_misses"])
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main(legs, tokens=(64, 512), trees=(ROOT,), kinds=KINDS, rounds=2):
    steps = {"decode-mixtral": 40, "decode-deepseek": 60, "miss-mixtral": 10, "tight-mixtral": 6, "prefill-mixtral": 3, "prefill-deepseek": 5}
    runs = [(leg, t) for leg in legs for t in (tokens if leg.startswith("prefill") else (1,))]
    rows = []
    for rnd in range(rounds):  # A/B/C/A/B/C
        for leg, t in runs:
            for tree in trees:
                has_mx = os.path.exists(os.path.join(tree, "moe-infinity_amd", "quant.py"))
                for kind in kinds:
                    if kind.startswith("mxfp4") and not has_mx:
                        continue
                    if kind == "mxfp4-gemm" and not os.path.exists(os.path.join(tree, "moe-infinity_amd", "csrc", "ffn_gemm_mx4.hip")):
                        continue
                    st = max(1, steps[leg] * 512 // t) if leg.startswith("prefill") else steps[leg]
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, kind, "--steps", str(st), "--tokens", str(t),
                                        "--tree", tree], capture_output=True, text=True, timeout=900)
                    r = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                    if p.returncode != 0 or not r:
                        print(f"{leg} slots={kind} tree={tree}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                        sys.exit(1)  # a failed GPU run ends the measurement
                    d = json.loads(r[0][7:])
                    d.update(round=rnd, tree=os.path.basename(os.path.abspath(tree)))
                    rows.append(d)
                    print(json.dumps(d), flush=True)
    for leg, t in runs:
        for tree in trees:
            name = os.path.basename(os.path.abspath(tree))
            for kind in kinds:
                rs = [r for r in rows if r["leg"] == leg and r["slots"] == kind and r["tree"] == name and (r.get("tokens", 1) == t or not leg.startswith("prefill"))]
                if not rs:
                    continue
                key = "ms_per_token" if "ms_per_token" in rs[0] else "ms_per_layer"
                extra = f" hit_rate {[r['hit_rate'] for r in rs]} link GB/s {[r['link_gbs'] for r in rs]}" if "hit_rate" in rs[0] else ""
                tt = f" T={t}" if leg.startswith("prefill") else ""
                print(f"SUMMARY {leg:18s}{tt:7s} {name:10s} {kind:10s} slots {key} {[r[key] for r in rs]}{extra}", flush=True)
        # what the misses alone would take at the link rate the bf16 run of the same leg reached
        for tree in trees:
            name = os.path.basename(os.path.abspath(tree))
            base = [r for r in rows if r["leg"] == leg and r["slots"] == "bf16" and r["tree"] == name and "link_gbs" in r and r["misses_per_token"] > 0]
            if base:
                rate = max(r["link_gbs"] for r in base)
                for r in rows:
                    if r["leg"] == leg and r["tree"] == name and "link_gbs" in r:
                        floor = r["misses_per_token"] * r["blob_bytes"] / (rate * 1e9) * 1e3
                        print(f"LINK    {leg:18s} {name:10s} {r['slots']:5s} round {r['round']}: {r['ms_per_token']} ms/token, misses x blob / "
                              f"{rate} GB/s (bf16's rate in this session) = {floor:.3f} ms", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    steps_, tokens_, tree_, trees_ = opt("--steps", "20"), opt("--tokens", "64,512"), opt("--tree", ROOT), opt("--trees", ROOT)
    kinds_, rounds_ = opt("--slots", ",".join(KINDS)), int(opt("--rounds", "2"))
    if args and args[0] == "--child":
        child(args[1], args[2], int(steps_), int(tokens_.split(",")[0]), os.path.abspath(tree_))
    else:
        main(args or LEGS, [int(t) for t in tokens_.split(",")], [os.path.abspath(t) for t in trees_.split(",")], kinds_.split(","), rounds_)
