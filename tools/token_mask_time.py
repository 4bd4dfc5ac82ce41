#!/usr/bin/env python3
"""Token masks (MoEEngine.forward(token_mask=...)) at model size: what padded tokens cost with and without the mask.

    nllb      NLLB-MoE-54B shapes (H 2048, F 8192, 128 experts, top-2), one resident layer, an encoder batch of B = 32 sequences
              with lengths 16..128 padded to 128 (T = 4096): expert rows and ms per layer, masked vs unmasked
    mixtral   Mixtral-8x7B, 4 layers, device_memory_bytes = 50 % of the layers' expert bytes, left-padded prompts (B = 4,
              lengths 2..S padded to S, S = 16 and 256, new activations every prefill): expert misses and ms per prefill
              (4 layers), masked vs unmasked, alternating prefill by prefill on one engine

    python tools/token_mask_time.py [nllb] [mixtral]      (one JSON line per measurement, each leg in a process of its own)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fill(eng, L, std=0.02):
    import torch

    dev = torch.device("cuda:0")
    off, siz, tot = eng.expert_layout(0)
    es = 2
    g = torch.Generator(device=dev)
    for l in range(L):
        for e in range(eng.cfg.num_experts):
            eng.register_expert(l, e, None)
            g.manual_seed(1000 * l + e)
            w = torch.empty(tot // es, dtype=torch.bfloat16, device=dev).normal_(0.0, std, generator=g)
            eng.expert_host_view(l, e).view(torch.bfloat16).copy_(w)
            del w
    torch.cuda.synchronize()


def _lengths(b, lo, hi, seed):
    import torch

    return torch.randint(lo, hi + 1, (b,), generator=torch.Generator().manual_seed(seed))


def leg_nllb():
    import torch
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    B, S = 32, 128
    T = B * S
    cfg = Cf.nllb_moe_54b(max_tokens=T, device_memory_ratio=0.8)
    cfg.num_layers = 1
    eng = MoEEngine(cfg)
    _fill(eng, 1)
    eng.prefetch(0, list(range(cfg.num_experts)))
    eng.sync_copies()
    dev = torch.device("cuda:0")
    lens = _lengths(B, 16, S, 5)
    keep = (torch.arange(S)[None, :] < lens[:, None]).reshape(-1).to(dev)
    gate = (torch.randn(cfg.num_experts, cfg.hidden, device=dev) * 0.5 / cfg.hidden ** 0.5).to(torch.bfloat16)
    x = torch.randn(T, cfg.hidden, device=dev).to(torch.bfloat16)
    out = torch.empty_like(x)
    rows = {}
    for name, m in (("unmasked", None), ("masked", keep)):
        eng.forward(0, x, gate, out=out, token_mask=m)
        torch.cuda.synchronize()
        rows[name] = int(eng.routing()["counts"][: cfg.num_experts].sum())
    times = {"unmasked": [], "masked": []}
    iters = 20
    for rnd in range(4):  # A/B/A/B
        for name, m in (("unmasked", None), ("masked", keep)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                eng.forward(0, x, gate, out=out, token_mask=m)
            torch.cuda.synchronize()
            times[name].append(round((time.perf_counter() - t0) / iters * 1e3, 3))
    st = eng.stats()
    eng.close()
    for name in ("unmasked", "masked"):
        print("RESULT " + json.dumps(dict(leg="nllb", variant=name, tokens=T, real_tokens=int(keep.sum()), expert_rows=rows[name],
                                          ms_per_layer=times[name], expert_misses=st["expert_misses"])), flush=True)


def leg_mixtral(S):
    import torch
    from moe_infinity_amd import MoEEngine
    from moe_infinity_amd import config as Cf

    B = 4
    T = B * S
    cfg = Cf.mixtral_8x7b(max_tokens=T)
    cfg.num_layers = 4
    L, E = cfg.num_layers, cfg.num_experts
    cfg.device_memory_bytes = L * E * 3 * cfg.hidden * cfg.inter * 2 // 2
    eng = MoEEngine(cfg)
    _fill(eng, L)
    for l in range(L):
        eng.prefetch(l, list(range(E)))
    eng.sync_copies()
    dev = torch.device("cuda:0")
    gates = [(torch.randn(E, cfg.hidden, device=dev) * 0.02).to(torch.bfloat16) for _ in range(L)]
    out = torch.empty(T, cfg.hidden, dtype=torch.bfloat16, device=dev)
    res = {"unmasked": dict(ms=[], misses=[], rows=[]), "masked": dict(ms=[], misses=[], rows=[])}
    steps = 12
    for step in range(steps + 2):
        g = torch.Generator(device=dev).manual_seed(step)
        x = torch.randn(T, cfg.hidden, device=dev, generator=g).to(torch.bfloat16)
        lens = _lengths(B, 2, S, 100 + step)
        keep = (torch.arange(S)[None, :] >= (S - lens)[:, None]).reshape(-1).to(dev)  # left padding
        for name, m in ((("unmasked", None), ("masked", keep)) if step % 2 == 0 else (("masked", keep), ("unmasked", None))):
            torch.cuda.synchronize()
            s0 = eng.stats()["expert_misses"]
            rows = 0
            t0 = time.perf_counter()
            for l in range(L):
                eng.forward(l, x, gates[l], out=out, token_mask=m)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            rows = int(eng.routing()["counts"][:E].sum())  # last layer's expert rows
            if step >= 2:  # warm
                res[name]["ms"].append(round(dt, 2))
                res[name]["misses"].append(eng.stats()["expert_misses"] - s0)
                res[name]["rows"].append(rows)
    eng.close()
    for name in ("unmasked", "masked"):
        r = res[name]
        print("RESULT " + json.dumps(dict(leg="mixtral", variant=name, prompt_len=S, batch=B, layers=L, cache="50%",
                                          ms_per_prefill=r["ms"], misses_per_prefill=r["misses"],
                                          mean_ms=round(sum(r["ms"]) / len(r["ms"]), 2),
                                          mean_misses=round(sum(r["misses"]) / len(r["misses"]), 2),
                                          last_layer_rows=r["rows"])), flush=True)


def main(legs):
    for leg in legs:
        for arg in (["16", "256"] if leg == "mixtral" else [""]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, arg], capture_output=True, text=True, timeout=1200)
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    print(line[7:], flush=True)
            if p.returncode != 0:
                print(f"{leg} {arg}: exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
                sys.exit(1)  # a failed GPU run ends the measurement


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        if sys.argv[2] == "nllb":
            leg_nllb()
        else:
            leg_mixtral(int(sys.argv[3]))
    else:
        main(sys.argv[1:] or ["nllb", "mixtral"])
