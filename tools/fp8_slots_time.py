#!/usr/bin/env python3
"""fp8 slots (EngineConfig.fp8_slots) against today's fp8 engine (bf16 slots, the pull kernel up-casts), A/B/A/B, every run in a
process of its own.  Legs:

    decode-mixtral     Mixtral-8x7B, 32 layers resident, batch 1: ms/token
    decode-deepseek    DeepSeek-V2-Lite, 26 layers resident, batch 1: ms/token
    miss-mixtral       Mixtral-8x7B, 16 layers, device_memory_bytes = 50 % of the layers' bf16 expert bytes, changing routing:
                       hit rate once warm and ms/token
    prefill-mixtral    Mixtral-8x7B, 8 layers resident, 512 tokens (--tokens): ms per layer
    prefill-deepseek   DeepSeek-V2-Lite, 8 layers resident, 512 tokens (--tokens): ms per layer

    python tools/fp8_slots_time.py [--tokens N,...] [--trees DIR,...] [leg ...]
        (default: every leg; one JSON line per run, then a summary.  --tokens: the prefill legs at each length; --trees: the
        same runs against the library of each of these checkouts in turn, A/B/A/B — e.g. the parent commit and this one)
    python tools/fp8_slots_time.py --child <leg> <0|1> [--steps N] [--tokens N] [--tree DIR]   (one run; used by the above and by rocprofv3)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["decode-mixtral", "decode-deepseek", "miss-mixtral", "prefill-mixtral", "prefill-deepseek"]


def child(leg, fp8_slots, steps, tokens=512, tree=ROOT):
    sys.path.insert(0, tree)
    import torch
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    wl = "mixtral" if "mixtral" in leg else "deepseek"
    T = tokens if leg.startswith("prefill") else 1
    mk = Cf.mixtral_8x7b if wl == "mixtral" else Cf.deepseek_v2_lite
    cfg = mk(dtype=Cf.DTYPE_F8E4M3, gate_dtype=Cf.DTYPE_BF16, max_tokens=T, fp8_slots=bool(fp8_slots), device_memory_ratio=0.8)
    if leg == "miss-mixtral":
        cfg.num_layers = 16
        slot16 = 3 * cfg.hidden * cfg.inter * 2  # bf16 slot bytes (4 KiB multiples for these shapes)
        cfg.device_memory_bytes = cfg.num_layers * cfg.num_experts * slot16 // 2
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
            w = torch.empty(tot, device=dev).normal_(0.0, 0.02, generator=g).to(torch.float8_e4m3fn)
            eng.expert_host_view(l, e).copy_(w.view(torch.uint8))
            del w
        if cfg.shared_inter:
            _, sizs, _ = eng.expert_layout(1)
            eng.register_shared(l, [torch.empty(s, dtype=torch.float32).normal_(0.0, 0.02).to(torch.float8_e4m3fn) for s in sizs])
        eng.prefetch(l, list(range(E)))  # (miss leg: every expert once, so the cache starts warm — what it holds is the policy's choice)
    eng.sync_copies()
    torch.cuda.synchronize()
    gates = [(torch.randn(E, cfg.hidden, device=dev) * 0.02).to(torch.bfloat16) for _ in range(L)]
    xs = [(torch.randn(T, cfg.hidden, device=dev)).to(torch.bfloat16) for _ in range(8)]
    out = torch.empty(T, cfg.hidden, dtype=torch.bfloat16, device=dev)
    res = dict(leg=leg, fp8_slots=int(fp8_slots))
    if leg == "miss-mixtral":
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
        res.update(ms_per_token=round(dt * 1e3, 3), hit_rate=round(hits / max(1, hits + miss), 4), slots_total=s1["slots_total"],
                   slot_bytes=s1["slot_bytes"])
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
        res.update(slots_total=st["slots_total"], slot_bytes=st["slot_bytes"], misses_measured=st["expert_misses"])
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main(legs, tokens=(512,), trees=(ROOT,)):
    steps = {"decode-mixtral": 40, "decode-deepseek": 60, "miss-mixtral": 10, "prefill-mixtral": 3, "prefill-deepseek": 5}
    runs = [(leg, t) for leg in legs for t in (tokens if leg.startswith("prefill") else (1,))]
    rows = []
    for rnd in range(2):  # A/B/A/B
        for leg, t in runs:
            for tree in trees:
                for f8 in (0, 1):
                    st = max(1, steps[leg] * 512 // t) if leg.startswith("prefill") else steps[leg]
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(f8), "--steps", str(st), "--tokens", str(t),
                                        "--tree", tree], capture_output=True, text=True, timeout=900)
                    r = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                    if p.returncode != 0 or not r:
                        print(f"{leg} fp8_slots={f8} tree={tree}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                        sys.exit(1)  # a failed GPU run ends the measurement
                    d = json.loads(r[0][7:])
                    d.update(round=rnd, tree=os.path.basename(os.path.abspath(tree)))
                    rows.append(d)
                    print(json.dumps(d), flush=True)
    for leg, t in runs:
        for tree in trees:
            for f8 in (0, 1):
                name = os.path.basename(os.path.abspath(tree))
                rs = [r for r in rows if r["leg"] == leg and r["fp8_slots"] == f8 and r["tree"] == name and (r.get("tokens", 1) == t or leg.startswith(("decode", "miss")))]
                key = "ms_per_token" if "ms_per_token" in rs[0] else "ms_per_layer"
                extra = f" hit_rate {[r['hit_rate'] for r in rs]}" if "hit_rate" in rs[0] else ""
                tt = f" T={t}" if leg.startswith("prefill") else ""
                print(f"SUMMARY {leg:18s}{tt:7s} {name:10s} {'fp8 slots ' if f8 else 'bf16 slots'} {key} {[r[key] for r in rs]}{extra}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    steps_, tokens_, tree_, trees_ = opt("--steps", "20"), opt("--tokens", "512"), opt("--tree", ROOT), opt("--trees", ROOT)
    if args and args[0] == "--child":
        child(args[1], int(args[2]), int(steps_), int(tokens_), os.path.abspath(tree_))
    else:
        main(args or LEGS, [int(t) for t in tokens_.split(",")], [os.path.abspath(t) for t in trees_.split(",")])
