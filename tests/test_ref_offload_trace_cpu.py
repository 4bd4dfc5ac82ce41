"""tests/golden/offload_engine_trace.json is what the REFERENCE'S code does: the reference's OffloadEngine._offload_state_dict /
setup_archer_hooks / module hooks, its SyncMixtralSparseMoeBlock and dispatch_local, run by oracle/gen_offload_trace.py against
the recording stand-in of the pybind module (re-run it beside a reference checkout to refresh the fixture).  This file checks the fixture's shape; the
GPU test tests/test_gpu_dropin.py::test_prefetch_op_under_the_reference_offload_engines_own_call_sequence then holds the real
prefetch_op to this sequence."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "offload_engine_trace.json")


def test_fixture_is_well_formed():
    d = json.load(open(GOLD))
    names = [c[0] for c in d["calls"]]
    assert names.count("forward") == 2 and names.count("set_topology") == 1
    L, E = d["shapes"]["L"], d["shapes"]["E"]
    assert names.count("register_expert") == L * E and names.count("offload") == names.count("register") == len(d["name_id_map"])
    assert names.count("begin") == names.count("end") and names.count("wait_expert") == 2 * L
    assert [n for n, _ in d["topology"]] == [x for l in range(L) for x in (f"layers.{l}", f"layers.{l}.block_sparse_moe.experts")] + ["lm_head"]
