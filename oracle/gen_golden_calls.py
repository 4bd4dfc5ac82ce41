#!/usr/bin/env python3
"""Generate tests/golden/reference_call_traces.json: what the REFERENCE's own Python code calls across two interface
boundaries, recorded on CPU.  TEST INFRASTRUCTURE ONLY; needs the reference checkout (oracle/gen_golden.py REF), the
fixture it writes is committed so the tests that hold our mirrors to it run anywhere.  Re-run:  python oracle/gen_golden_calls.py

  dispatch_local      DistributedExpertExecutor.dispatch_local (moe_infinity/distributed/expert_executor.py) driving a
                      recording expert_dispatcher, 25 seeded routing masks, each as [T, E] and as [1, T, E], 3 GPUs
  expert_prefetcher   ExpertPrefetcher.prefetch_experts (moe_infinity/memory/expert_prefetcher.py) driving our
                      PrefetchHandle adapter: every adapter call with its arguments and return value
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_call_traces.json")
DEVICE_COUNT = 3  # gpu_id = expert_id % device_count
PREFETCH_L, PREFETCH_E, PREFETCH_LAYER = 3, 4, 1
PREFETCH_MATRIX = [[0, 0, 0, 0], [0.5, 0, 0.25, 0], [0, 0.125, 0, 0.75]]


class Recorder:
    """expert_dispatcher stand-in that records the call sequence"""

    def __init__(self):
        self.calls = []

    def set_inputs(self, hidden, mask):
        self.calls.append(("set_inputs", tuple(hidden.shape), tuple(mask.shape), int(mask.sum())))

    def set_expected_queue(self, n):
        self.calls.append(("set_expected_queue", int(n)))

    def enqueue_expert(self, layer, expert, gpu, remote):
        self.calls.append(("enqueue_expert", int(layer), int(expert), int(gpu), bool(remote)))

    def wait_expert(self):
        self.calls.append(("wait_expert",))
        return [("result", len(self.calls))]


def jsonable(x):
    return json.loads(json.dumps(x))


def mask_of(case):
    m = torch.zeros(case["t"], case["e"], dtype=torch.bool)
    for r, c in case["mask"]:
        m[r, c] = True
    return m


def run_dispatch_case(executor_cls, case):
    """one case through executor_cls.dispatch_local, as [T, E] then as [1, T, E]: (calls, outputs) of each"""
    rec = Recorder()
    ex = executor_cls(None)
    ex.set_expert_dispatcher(rec)
    mask = mask_of(case)
    hidden = torch.zeros(case["t"], 16)
    res = {}
    for form, (h, m) in (("2d", (hidden, mask)), ("3d", (hidden[None], mask[None]))):
        out = ex.dispatch_local(h, m, case["layer"])
        res[form] = {"calls": jsonable(rec.calls), "out": jsonable(out)}
    return res


def dispatch_cases():
    g = torch.Generator().manual_seed(3)
    cases = []
    for trial in range(25):
        t, e = int(torch.randint(1, 40, (1,), generator=g)), int(torch.randint(2, 130, (1,), generator=g))
        mask = torch.rand(t, e, generator=g) < (2.0 / e)
        if trial % 5 == 0:
            mask[:] = False  # nothing routed: empty expert list
        cases.append({"t": t, "e": e, "layer": trial % 7, "mask": mask.nonzero().tolist()})
    return cases


class _AdapterLog:
    """forwards to a PrefetchHandle and records (method, args, return value) of every call"""

    def __init__(self, inner):
        self._inner, self.log = inner, []

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def call(*args):
            r = fn(*args)
            self.log.append([name, jsonable([a.tolist() if hasattr(a, "tolist") else a for a in args]), jsonable(r)])
            return r

        return call


class _Engine:
    class cfg:
        device_id = 0

    def protect(self, pairs):
        pass

    def prefetch(self, layer, experts, scores=None):
        pass


def reference_prefetcher_trace(ref_root):
    from moe_infinity_amd.prefetch_handle import PrefetchHandle

    src = os.path.join(ref_root, "moe_infinity", "memory", "expert_prefetcher.py")
    # the module imports moe_infinity.utils.parse_moe_param; stub the package around the one file we want
    stub, utils = types.ModuleType("moe_infinity"), types.ModuleType("moe_infinity.utils")
    utils.parse_moe_param = lambda config: (PREFETCH_L, PREFETCH_E, 0)
    stub.utils = utils
    saved = {k: sys.modules.get(k) for k in ("moe_infinity", "moe_infinity.utils")}
    sys.modules["moe_infinity"], sys.modules["moe_infinity.utils"] = stub, utils
    try:
        spec = importlib.util.spec_from_file_location("ref_expert_prefetcher", src)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    tmap = {(l, e): 100 + 10 * l + e for l in range(PREFETCH_L) for e in range(PREFETCH_E)}
    handle = _AdapterLog(PrefetchHandle(_Engine(), tmap))
    ref = mod.ExpertPrefetcher(config=None)
    ref.set_archer_engine(handle)
    ref.expert_tensor_map = tmap
    ref.prefetch_experts(PREFETCH_LAYER, np.array(PREFETCH_MATRIX))
    return {"L": PREFETCH_L, "E": PREFETCH_E, "layer": PREFETCH_LAYER, "matrix": PREFETCH_MATRIX,
            "tensor_id": "100 + 10 * layer + expert", "adapter_calls": handle.log}


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    from oracle.gen_golden import REF, import_reference

    torch.cuda.device_count = lambda: DEVICE_COUNT
    theirs = import_reference()["executor"].DistributedExpertExecutor
    cases = dispatch_cases()
    for c in cases:
        c.update(run_dispatch_case(theirs, c))
    d = {"dispatch_local": {"device_count": DEVICE_COUNT, "hidden_columns": 16, "cases": cases},
         "expert_prefetcher": reference_prefetcher_trace(REF)}
    with open(OUT, "w") as f:
        json.dump(d, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
