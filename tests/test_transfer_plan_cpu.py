"""How the routed experts are held and how one of them travels from its pinned host blob into its HBM slot — two pure functions
decide (csrc/transfer_plan.h weight_format and transfer_plan; DESIGN.md sections 5 and 5.1), exported as moeinf_transfer_plan.
Until they existed the choice lived in the control flow of moeinf_create_ex, create_engine and issue_copy, and only GPU tests
reached it.  tests/golden/transfer_plans.json holds 311 engines — Mixtral-8x7B, DeepSeek-V2-Lite (with its shared expert), NLLB-MoE
and fsgpt (bias vectors), Switch-base-8 and a gated Switch; bf16 / fp16 / fp32, fp8 experts with bf16 slots, fp8 slots and MXFP4 slots
where the family has them; MOEINF_H2D_PULL x MOEINF_H2D_WHOLE_BLOB_MB, MOEINF_H2D_PULL_WGS; one engine per refusal — with what that
control flow answered and the stream commands its issue_copy issued for one expert, recorded on the CPU from its HIP runtime calls.

No case has a bias vector that is not a 16-byte multiple (the shape that makes the pull form fall back to SDMA tensor by tensor):
validate() admits none — hidden and inter are multiples of 8 (two-byte dtypes) or 4 (fp32), so a vector is whole 16-byte pieces."""
import ctypes as C
import json
import os

import pytest

from moe_infinity_amd import load_library

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "transfer_plans.json")
KNOBS = ("MOEINF_H2D_PULL", "MOEINF_H2D_WHOLE_BLOB_MB", "MOEINF_H2D_PULL_WGS")
PULL, SDMA_BLOB, SDMA_TENSORS = 0, 1, 2
UNSUPPORTED = 5
MIXTRAL_8X7B = [0, 0, -1, 4, 0, 1, 4096, 14336, 0]
DEEPSEEK_V2_LITE = [0, 0, -1, 5, 1, 1, 2048, 1408, 2816]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def plan(shape):
    """(rc, None) or (0, the exported plan as a dict)"""
    out = (C.c_int32 * 168)()
    rc = load_library().moeinf_transfer_plan((C.c_int32 * 9)(*shape), 9, out, 168)
    assert out[0] == rc
    if rc:
        return rc, None
    o = list(out)
    u64 = lambda lo, hi: (lo & 0xFFFFFFFF) | (hi << 32)
    p = dict(dt=o[1], host_dt=o[2], slot_dt=o[3], form=o[4], one_event=o[5], src_f8=o[6], pull_wgs=o[7], write_stream=("copy", "retile")[o[8]],
             event_timing=o[9], stage_bytes=u64(o[10], o[11]), h2d_bytes=u64(o[12], o[13]), steps=[])
    for s in range(o[14]):
        b = 16 + 38 * s
        t = [o[b + 2 + 9 * j: b + 11 + 9 * j] for j in range(o[b])]
        p["steps"].append(dict(ready1_after=o[b + 1], tensors=[dict(index=v[0], src=u64(v[1], v[2]), dst=u64(v[3], v[4]), bytes=u64(v[5], v[6]),
                                                                     R=v[7], K=v[8]) for v in t]))
    return 0, p


def commands(p):
    """the stream commands of one transfer: the three executors of engine.cpp (run_pull, run_sdma_blob, run_sdma_tensors) and the
    frame issue_copy puts around them, restated"""
    blob = lambda st: [[t["src"], t["dst"], t["R"], t["K"]] for t in st["tensors"]]
    c = [["copy", "record", "timer"]] if p["event_timing"] else []
    if p["form"] == PULL:
        c.append(["copy", "first_write"])
        for k, st in enumerate(p["steps"]):
            c.append(["copy", "pull", blob(st), 4 if p["slot_dt"] == 16 else p["slot_dt"], p["src_f8"], p["pull_wgs"], 1, int(k == 0)])
            c += [["copy", "record", "ready1"]] * st["ready1_after"]
    elif p["form"] == SDMA_BLOB:
        c += [["copy", "memcpy", "h2d", 0, p["h2d_bytes"]], ["copy", "record", "filled"], ["retile", "wait", "filled"], ["retile", "first_write"],
              ["retile", "retile_blob", blob(p["steps"][0]), p["dt"], 0], ["retile", "record", "freed"]]
    else:
        for k, st in enumerate(p["steps"]):
            (t,) = st["tensors"]
            c += [["copy", "memcpy", "h2d", t["src"], t["bytes"]], ["copy", "record", "filled"], ["retile", "wait", "filled"]]
            c += [["retile", "first_write"]] * (k == 0)
            c.append(["retile", "retile", t["dst"], t["R"], t["K"], p["dt"]] if t["K"] else ["retile", "memcpy", "d2d", t["dst"], t["bytes"]])
            c.append(["retile", "record", "freed"])
            c += [["retile", "record", "ready1"]] * st["ready1_after"]
    c += [["copy", "record", "timer"]] * p["event_timing"]
    c.append([p["write_stream"], "record", "ready"])
    return c


def _set_env(monkeypatch, env):
    for k in KNOBS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def test_every_recorded_transfer_is_the_plan_executed(monkeypatch):
    g = _golden()
    assert g["recorded_from"] == "a3d39d0" and len(g["cases"]) == 311
    for case in g["cases"]:
        _set_env(monkeypatch, case["env"])
        rc, p = plan(case["shape"])
        assert rc == case["rc"], case["name"]
        if rc:
            continue
        assert case["copy_rc"] == 0
        assert commands(p) == case["commands"], case["name"]
        assert (p["slot_dt"], p["stage_bytes"], p["h2d_bytes"], p["one_event"]) == \
            (case["slot_dtype"], case["stage_bytes"], case["h2d_bytes"], case["one_event"]), case["name"]


# one per refusal of weight_format: (what the refusal's text says, then as now) -> the recorded case that meets it
REFUSALS = {
    "refuse-fp8slots-bf16-experts": ("fp8 slots", "need fp8 experts"),
    "refuse-fp8slots-nllb": ("fp8 slots", "Mixtral and DeepSeek experts only"),
    "refuse-fp8slots-switch-router": ("fp8 slots", "router_kind"),
    "refuse-fp8slots-ep2": ("fp8 slots", "expert parallelism"),
    "refuse-fp8slots-hidden-4128": ("fp8 slots", "multiples of 64"),
    "refuse-fp16slots-fp8-experts": ("slot_dtype 2 with dtype 3",),
    "refuse-fp32slots-bf16-experts": ("slot_dtype 1 with dtype 0",),
    "refuse-mxfp4-fp16-engine": ("mxfp4", "bf16 engine"),
    "refuse-mxfp4-fp8-experts": ("mxfp4", "bf16 engine"),
    "refuse-mxfp4-fp16-gate": ("mxfp4", "neither bf16 nor fp32"),
    "refuse-mxfp4-nllb": ("mxfp4", "Mixtral and DeepSeek experts only"),
    "refuse-mxfp4-switch-router": ("mxfp4", "router_kind"),
    "refuse-mxfp4-ep2": ("mxfp4", "expert parallelism"),
    "refuse-mxfp4-inter-14400": ("mxfp4", "multiples of 128"),
    "refuse-mxfp4-hidden-8320": ("mxfp4", "too long for the tier mover"),
    "refuse-mxfp4-pull0": ("mxfp4", "PULL tier mover", "MOEINF_H2D_PULL=0"),
    "refuse-fp8host-hidden-4104": ("fp8 experts", "multiples of 16"),
    "refuse-fp8host-pull0": ("fp8 experts", "PULL tier mover", "MOEINF_H2D_PULL=0"),
    "refuse-fp8slots-pull0": ("fp8 experts", "PULL tier mover", "MOEINF_H2D_PULL=0"),
}


def test_the_fixture_hides_no_branch(monkeypatch):
    cases = _golden()["cases"]
    ok = [c for c in cases if c["rc"] == 0]
    kinds = lambda c: [cmd[1] for cmd in c["commands"]]
    pulls = lambda c: kinds(c).count("pull")
    # all three forms, as the parent issued them
    assert any(pulls(c) for c in ok) and any("retile_blob" in kinds(c) for c in ok) and any("retile" in kinds(c) for c in ok)
    assert {c["one_event"] for c in ok} == {0, 1}
    assert {cmd[4] for c in ok for cmd in c["commands"] if cmd[1] == "pull"} == {0, 1}, "src_f8"
    assert {pulls(c) for c in ok} == {0, 1, 2}, "a one-step and a two-step pull"
    assert {cmd[3] for c in ok for cmd in c["commands"] if cmd[1] == "pull"} == {0, 1, 2, 3, 4}, "bf16, fp32, fp16, fp8 and MXFP4 slots"
    assert {cmd[5] for c in ok for cmd in c["commands"] if cmd[1] == "pull"} == {8, 16, 32}, "workgroups per launch"
    assert any(cmd[1:3] == ["memcpy", "d2d"] for c in ok for cmd in c["commands"]), "a bias vector through the staging ring"
    # ... and what the export says about them
    seen = set()
    for c in ok:
        _set_env(monkeypatch, c["env"])
        p = plan(c["shape"])[1]
        seen.add((p["form"], p["one_event"], p["src_f8"], len(p["steps"]), p["host_dt"], p["slot_dt"]))
    assert {s[0] for s in seen} == {PULL, SDMA_BLOB, SDMA_TENSORS}
    assert {(s[0], s[3]) for s in seen} == {(PULL, 1), (PULL, 2), (SDMA_BLOB, 1), (SDMA_TENSORS, 2), (SDMA_TENSORS, 3), (SDMA_TENSORS, 4)}
    assert {s[4:] for s in seen} == {(0, 0), (1, 1), (2, 2), (3, 0), (3, 3), (16, 16)}, "(host, slot) dtypes"
    # every refusal: recorded with the parent's code and text, and refused by weight_format with the same code and the same words
    refused = {c["name"]: c for c in cases if c["rc"]}
    assert set(refused) == set(REFUSALS)
    lib = load_library()
    for name, words in REFUSALS.items():
        c = refused[name]
        assert c["rc"] == UNSUPPORTED and all(w in c["error"] for w in words), c
        _set_env(monkeypatch, c["env"])
        assert plan(c["shape"])[0] == UNSUPPORTED
        msg = lib.moeinf_last_error().decode()
        assert all(w in msg for w in words), (name, msg)


def test_the_two_flagship_plans_are_what_design_md_states(monkeypatch):
    """DeepSeek-V2-Lite's 16.5 MiB expert is one pull launch and one event; Mixtral-8x7B's 336 MiB expert two
    launches, w1 and w3 first, with `ready1` between them"""
    _set_env(monkeypatch, {})
    _, d = plan(DEEPSEEK_V2_LITE)
    assert (d["form"], d["one_event"], d["src_f8"], d["pull_wgs"], d["write_stream"], d["event_timing"]) == (PULL, 1, 0, 16, "copy", 0)
    assert [[t["index"] for t in s["tensors"]] for s in d["steps"]] == [[0, 1, 2]] and d["steps"][0]["ready1_after"] == 0
    assert d["h2d_bytes"] == d["stage_bytes"] == 3 * 1408 * 2048 * 2
    _, m = plan(MIXTRAL_8X7B)
    assert (m["form"], m["one_event"], m["h2d_bytes"], m["stage_bytes"]) == (PULL, 0, 3 * 4096 * 14336 * 2, 4096 * 14336 * 2)
    assert [([t["index"] for t in s["tensors"]], s["ready1_after"]) for s in m["steps"]] == [([0, 2], 1), ([1], 0)]
    assert [cmd[1:3] for cmd in commands(m)] == [["first_write"], ["pull", [[0, 0, 14336, 4096], [2 * 4096 * 14336 * 2] * 2 + [14336, 4096]]],
                                                ["record", "ready1"], ["pull", [[4096 * 14336 * 2] * 2 + [4096, 14336]]], ["record", "ready"]]


def test_the_export_is_bound_and_checks_its_arguments():
    from moe_infinity_amd._lib import PROTOTYPES

    assert "moeinf_transfer_plan" in PROTOTYPES
    lib = load_library()
    shape = (C.c_int32 * 9)(*MIXTRAL_8X7B)
    out = (C.c_int32 * 168)()
    assert lib.moeinf_transfer_plan(shape, 9, out, 168) == 0
    assert lib.moeinf_transfer_plan(shape, 8, out, 168) == 1  # MOEINF_ERR_INVALID
    assert lib.moeinf_transfer_plan(shape, 9, out, 167) == 1
    assert lib.moeinf_transfer_plan(None, 9, out, 168) == 1
    shape[6] = 0
    assert lib.moeinf_transfer_plan(shape, 9, out, 168) == 1  # no hidden size
