"""The drop-in boundary on CPU: our mirror of ``DistributedExpertExecutor.dispatch_local`` (12 lines restated from
moe_infinity/distributed/expert_executor.py:32-58 — an interface mirror, not a design of ours) must drive a dispatcher
exactly like the reference's own function does.  What the reference's function called is recorded in
tests/golden/reference_call_traces.json (oracle/gen_golden_calls.py ran it); the GPU tests then use the mirror with the
real dispatcher."""
import json
import os

import pytest
import torch

from oracle.gen_golden_calls import run_dispatch_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_call_traces.json")


def test_dispatch_local_mirror_drives_the_dispatcher_like_the_reference_does(monkeypatch):
    from moe_infinity_amd.expert_executor import DistributedExpertExecutor as Ours

    gold = json.load(open(GOLD))["dispatch_local"]
    monkeypatch.setattr(torch.cuda, "device_count", lambda: gold["device_count"])  # gpu_id = expert_id % device_count
    cases = gold["cases"]
    assert len(cases) == 25 and any(not c["mask"] for c in cases) and max(c["e"] for c in cases) > 64
    for case in cases:
        got = run_dispatch_case(Ours, case)
        # [T, E] masks, then the same mask as [B, S, E] (viewed (-1, E) by both), on one dispatcher
        for form in ("2d", "3d"):
            assert got[form]["calls"] == case[form]["calls"], (case["layer"], case["t"], case["e"], form)
            assert got[form]["out"] == case[form]["out"]


def test_prefetch_op_exports_the_pybind_surface():
    """every method name of py_archer_prefetch.cpp:14-92 exists on the drop-in classes with the reference's arity"""
    import inspect

    from moe_infinity_amd import prefetch_op as P

    want_handle = {"offload": 2, "register": None, "set_tensor_device": 2, "begin": 2, "end": 2, "get_hit_rate": 0, "set_trace": 1,
                   "set_topology": 1, "update_tensor_map": 2, "is_tensor_offloaded": 1, "is_tensor_index_initialized": 0,
                   "is_tensor_on_device": 1, "get_node_default_device": 1, "get_node_device": 1, "prefetch_tensors": 2,
                   "replace_cache_candidates": 1, "enqueue_prefetch": 2, "fetch_tensors": 2, "clean_up_resources": 0}
    for name, arity in want_handle.items():
        fn = getattr(P.prefetch_handle, name)
        if arity is not None:
            assert len([p for p in inspect.signature(fn).parameters.values() if p.name != "self"]) == arity, name
    assert list(inspect.signature(P.prefetch_handle.__init__).parameters)[1:] == ["prefix", "device_memory_ratio"]
    assert list(inspect.signature(P.expert_dispatcher.__init__).parameters)[1:] == ["num_experts", "num_layers", "dtype", "expert_type", "num_threads"]
    want_disp = {"register_expert": 3, "enqueue_expert": 4, "set_inputs": 2, "set_expected_queue": 1, "wait_expert": 0, "clear_expert_cache_counts": 0}
    for name, arity in want_disp.items():
        assert len([p for p in inspect.signature(getattr(P.expert_dispatcher, name)).parameters.values() if p.name != "self"]) == arity, name
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.prefetch_handle("/tmp/x", 0.5)
