"""Which launches make up a forward, and which form each decode launcher takes — one function decides (csrc/kernels.h layer_form;
DESIGN.md section 4.3), exported as moeinf_layer_form.  Until it existed this choice lived in the control flow of moe_forward,
dispatch_experts and the decode launchers, and no test could reach it without a GPU.  tests/golden/layer_forms.json holds 1013
forwards — Mixtral-8x7B, DeepSeek-V2-Lite (bf16 and fp32 gate), a DeepSeek-V3-style gate, NLLB-MoE-54B and Switch-base-8 at 1 .. 4096
tokens, bf16 / fp16 / fp32 engines, fp8 and MXFP4 slots, both paths, masks, flags, an output override, CU counts the Switch
one-launch layer does not fit, and every knob value where it changes a launch — with what that control flow launched, recorded from its launches (kernel
instantiation, grid, block and dynamic LDS) on the CPU.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

from moe_infinity_amd import load_library

BF16, F32, F16, F8, MX4 = 0, 1, 2, 3, 16
ROUTE_ONLY, NO_COMBINE = 1, 2
# out[4]: the router launches
R_NONE, R_GATE, R_GATE_SHARED1, R_GATE_SHARED1_ROUTE_SHARED2, R_GATE_ROUTE_INDEX, R_GATE_TOPK_INDEX, R_GATE_TOPK_WIDE = range(7)
# out[6] / out[12]: the stages' launchers
ST_NONE, ST_GENERIC, ST_SELFROUTE, ST_SELFROUTE_MULTI, ST_FRONT1, ST_LAYER1_SWITCH, ST_DECODE1 = range(7)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "layer_forms.json")
FIELDS = ("hide_shared", "selfroute", "front1", "layer1_switch", "router", "gate", "stage1", "sr_waves", "sr_tiles", "sr_lds_kb",
          "sr_shared_last", "sr_grid", "stage2", "dec1_pair", "dec1_waves", "dec1_unroll", "dec1_grid_x", "dec1_grid_y", "sh1_waves",
          "sh1_unroll", "sh2_waves", "sh2_unroll", "can_fuse_combine", "fuse_mode", "kt1", "poll_sleep")

#             router kind, expert type, K, E, H, F, Fs, shared, n_group, v3, capacity
FAMILIES = {
    "mixtral": (0, 4, 2, 8, 4096, 14336, 0, 0, 1, 0, 0),
    "deepseek": (1, 5, 6, 64, 2048, 1408, 2816, 1, 1, 0, 0),
    "switch": (2, 0, 1, 8, 768, 3072, 0, 0, 1, 0, 64),
}


def raw(shape):
    out = (C.c_int32 * 26)()
    assert load_library().moeinf_layer_form((C.c_int32 * 21)(*shape), 21, out, 26) == 0
    return tuple(out)


def form(family, T=1, dt=BF16, gate=None, slot=None, flags=0, masked=0, fast=1, ovr_out=0, cus=256, wgs=2):
    rk, et, K, E, H, F, Fs, sh, ng, v3, cap = FAMILIES[family]
    gate = dt if gate is None else gate
    slot = dt if slot is None else slot
    return dict(zip(FIELDS, raw([rk, et, dt, gate, slot, T, K, E, H, F, Fs, sh, ng, v3, cap, flags, masked, fast, ovr_out, cus, wgs])))


def pick(f, *names):
    return tuple(f[n] for n in names)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _cases():
    by_env = {}
    for case, want in _golden()["cases"]:
        by_env.setdefault(case[0], []).append((case[1:], tuple(want)))
    return sorted(by_env.items())


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOEINF_")]:
        monkeypatch.delenv(k)


@pytest.mark.parametrize("env,cases", _cases(), ids=lambda v: (v or "default") if isinstance(v, str) else "")
def test_the_recorded_forms(monkeypatch, env, cases):
    for kv in filter(None, env.split(",")):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    for (label, *shape), want in cases:
        assert raw(shape) == want, (env, label, shape)


def test_the_fixture_hides_no_branch():
    """Under default knobs every enumerator of every enum field of LayerForm, and both values of every boolean field, occurs in a
    recorded case.  (sr_shared_last is the one field default knobs cannot reach: only MOEINF_SR_ORDER=1 sets it; it must occur
    among the knob cases.  fuse_mode is an int that only MOEINF_WIDE_OUT moves.)"""
    data = _golden()
    assert data["recorded_from"].startswith("ce76e31")
    default = [dict(zip(FIELDS, w)) for c, w in data["cases"] if c[0] == ""]
    seen = lambda name, rows=default: {r[name] for r in rows}
    for name in ("hide_shared", "front1", "dec1_pair", "can_fuse_combine", "kt1"):
        assert seen(name) == {0, 1}, name
    assert seen("selfroute") == {0, 1, 2}
    assert seen("layer1_switch") == {0, 1, 2}
    assert seen("router") == set(range(7))
    assert seen("gate") == {0, 1, 4, 16}
    assert seen("stage1") == {ST_NONE, ST_GENERIC, ST_SELFROUTE, ST_SELFROUTE_MULTI, ST_FRONT1, ST_LAYER1_SWITCH}
    assert seen("stage2") == {ST_NONE, ST_GENERIC, ST_DECODE1}
    assert seen("sr_shared_last", [dict(zip(FIELDS, w)) for c, w in data["cases"]]) == {0, 1}
    assert seen("fuse_mode", [dict(zip(FIELDS, w)) for c, w in data["cases"]]) == {1, 2}


def test_every_knob_is_recorded_where_a_launcher_tells_it_apart():
    """Every knob of LayerKnobs occurs among the recorded cases, and every recorded knob case differs from the same forward under
    default knobs (a row that a knob cannot change would claim coverage it does not give)."""
    cases = _golden()["cases"]
    default = {tuple(c[2:]): w for c, w in cases if c[0] == ""}
    names = set()
    for c, w in cases:
        if c[0]:
            names.update(kv.split("=")[0] for kv in c[0].split(","))
            assert tuple(c[2:]) not in default or default[tuple(c[2:])] != w, c
    assert names == {"MOEINF_" + k for k in (
        "HIDE_SHARED", "SELFROUTE", "SELFROUTE_MULTI", "SELFROUTE_MULTI_PAIRS", "LAYER1_SWITCH", "FRONT1", "INDEX_WIDE_PAIRS", "FUSE_COMBINE",
        "WIDE_OUT", "LAYER1_SLEEP", "SR_LDS_KB", "SR_U", "SR_ORDER", "DEC1_PAIR", "DEC1_PAIR_U", "DEC1_U", "DEC1_SWITCH_U", "SH1_U", "SH1_NW",
        "SH2_NW", "SH2_U", "GATE_MFMA_TILES")}
    # the forms only a knob reaches: Switch's ffn2_decode1<T, 16, 4> for every dtype, bf16's sweep forms, the eight-wave pair kernel
    dec1 = {(c[4], w[13], w[14], w[15]) for c, w in cases if w[12] == ST_DECODE1}
    assert {(dt, 0, 16, 4) for dt in (BF16, F16, F32)} <= dec1
    assert {(BF16, 1, 4, 2), (BF16, 1, 8, 4), (BF16, 0, 4, 12), (BF16, 0, 4, 8), (BF16, 1, 4, 8)} <= dec1


def test_the_export_is_declared_and_checks_its_arguments():
    from moe_infinity_amd._lib import PROTOTYPES

    assert "moeinf_layer_form" in PROTOTYPES
    lib = load_library()
    shape, out = (C.c_int32 * 21)(*([0, 4, 0, 0, 0, 1, 2, 8, 4096, 14336] + [0] * 11)), (C.c_int32 * 26)()
    assert lib.moeinf_layer_form(shape, 21, out, 26) == 0
    assert lib.moeinf_layer_form(shape, 20, out, 26) == 1  # MOEINF_ERR_INVALID
    assert lib.moeinf_layer_form(shape, 21, out, 25) == 1
    assert lib.moeinf_layer_form(None, 21, out, 26) == 1
    shape[5] = 0
    assert lib.moeinf_layer_form(shape, 21, out, 26) == 1  # no tokens


def test_mixtral_batch_1():
    f = form("mixtral")  # gate, ffn1_selfroute<bf16, 2, 4, 4> under 30 KB of dynamic LDS (1 + 2 * 896 workgroups), ffn2_decode1_pair<4, 4>
    assert pick(f, "router", "gate", "stage1", "stage2") == (R_GATE, 1, ST_SELFROUTE, ST_DECODE1)
    assert pick(f, "sr_waves", "sr_tiles", "sr_lds_kb", "sr_grid") == (4, 4, 30, 1793)
    assert pick(f, "dec1_pair", "dec1_waves", "dec1_unroll", "dec1_grid_x", "dec1_grid_y") == (1, 4, 4, 256, 1)
    assert pick(f, "front1", "can_fuse_combine", "kt1") == (0, 1, 1)
    # fp8 and MXFP4 slots take the same forms
    assert form("mixtral", slot=F8) == f and form("mixtral", slot=MX4) == f
    # the decision path: the generic launches, the combine fused into stage 2
    assert pick(form("mixtral", fast=0), "router", "stage1", "stage2", "can_fuse_combine") == (R_GATE_ROUTE_INDEX, ST_GENERIC, ST_GENERIC, 1)


def test_deepseek_batch_1():
    f = form("deepseek")  # moe_front1 (gate, both shared stages, stage 1: 64 + 176 + 1 + 6 * 88 + 128 workgroups), then ffn2_decode1<4, 4>
    assert pick(f, "hide_shared", "front1", "router", "gate", "stage1", "stage2") == (1, 1, R_NONE, 0, ST_FRONT1, ST_DECODE1)
    assert pick(f, "sr_waves", "sr_tiles", "sr_lds_kb", "sr_grid") == (4, 8, 0, 897)
    assert pick(f, "dec1_pair", "dec1_waves", "dec1_unroll", "dec1_grid_x", "dec1_grid_y") == (0, 4, 4, 128, 6)
    # an fp32 gate rides along; a grouped (V3-style) gate does not self-route
    assert form("deepseek", gate=F32) == f
    rk, et, K, E, H, F, Fs, sh, _, _, cap = FAMILIES["deepseek"]
    v3 = dict(zip(FIELDS, raw([rk, et, BF16, BF16, BF16, 1, K, E, H, F, Fs, sh, 8, 1, cap, 0, 0, 1, 0, 256, 2])))
    assert pick(v3, "selfroute", "router", "stage1", "stage2") == (0, R_GATE_SHARED1_ROUTE_SHARED2, ST_GENERIC, ST_GENERIC)
    assert pick(v3, "sh1_waves", "sh1_unroll", "sh2_waves", "sh2_unroll") == (8, 8, 8, 4)


def test_small_decode_batches():
    # 2 .. 8 tokens and at most 24 (token, expert) pairs self-route; DeepSeek at 8 tokens = 48 pairs > 24 = no multi form
    assert pick(form("deepseek", T=4), "selfroute", "router", "stage1", "stage2", "kt1") == (2, R_GATE_SHARED1, ST_SELFROUTE_MULTI, ST_GENERIC, 0)
    assert pick(form("deepseek", T=8), "selfroute", "router", "stage1") == (0, R_GATE_SHARED1_ROUTE_SHARED2, ST_GENERIC)
    assert pick(form("mixtral", T=8), "selfroute", "stage1", "sr_grid") == (2, ST_SELFROUTE_MULTI, 1 + 8 * 896)
    assert form("mixtral", T=9)["selfroute"] == 0
    # up to 16 tokens the combine rides in stage 2; the shared expert hides under the router up to 64 pairs (DeepSeek: 10 tokens);
    # up to 64 tokens one launch routes and indexes
    assert pick(form("deepseek", T=10), "hide_shared", "can_fuse_combine") == (1, 1)
    assert pick(form("deepseek", T=16), "hide_shared", "can_fuse_combine", "router") == (0, 1, R_GATE_ROUTE_INDEX)
    assert pick(form("deepseek", T=17), "hide_shared", "can_fuse_combine", "router") == (0, 0, R_GATE_ROUTE_INDEX)
    assert form("mixtral", T=65)["router"] == R_GATE_TOPK_INDEX
    assert pick(form("mixtral", T=4096), "router", "gate") == (R_GATE_TOPK_WIDE, 16)  # 8192 pairs > 2048; 256 x 1 logit tiles >= 128


def test_switch_batch_1():
    f = form("switch", dt=F32)  # one launch: 8 + 1 + 192 + 4 * 48 = 393 workgroups, two per CU
    assert pick(f, "layer1_switch", "router", "stage1", "stage2", "can_fuse_combine") == (1, R_NONE, ST_LAYER1_SWITCH, ST_NONE, 1)
    # 393 workgroups do not fit 2 x 128 CUs: gate, the self-routing stage 1 on sixteen waves, ffn2_decode1<16, 12>
    d = form("switch", dt=F32, cus=128)
    assert pick(d, "layer1_switch", "router", "stage1", "stage2") == (2, R_GATE, ST_SELFROUTE, ST_DECODE1)
    assert pick(d, "sr_waves", "sr_tiles", "sr_lds_kb", "sr_grid") == (16, 4, 0, 193)
    assert pick(d, "dec1_pair", "dec1_waves", "dec1_unroll", "dec1_grid_x", "dec1_grid_y") == (0, 16, 12, 48, 1)
    assert form("switch", dt=F32, wgs=0)["layer1_switch"] == 2  # occupancy unknown
    assert form("switch", dt=F16)["layer1_switch"] == 0          # no fp16 form
    assert pick(f, "poll_sleep") == (2,) and d["poll_sleep"] == 0  # the counters' poll interval belongs to the fused launches


def test_knobs_of_the_switch_decode_forms(monkeypatch):
    monkeypatch.setenv("MOEINF_DEC1_SWITCH_U", "4")
    monkeypatch.setenv("MOEINF_LAYER1_SWITCH", "0")
    monkeypatch.setenv("MOEINF_LAYER1_SLEEP", "0")
    for dt in (BF16, F16, F32):
        assert pick(form("switch", dt=dt), "layer1_switch", "stage2", "dec1_waves", "dec1_unroll") == (0, ST_DECODE1, 16, 4)
    assert form("deepseek")["poll_sleep"] == 1  # at least one repetition


def test_what_takes_the_generic_launches():
    for family in FAMILIES:
        dt = F32 if family == "switch" else BF16
        # a masked batch-1 forward: the generic five launches (gate, route + index, two stages, combine)
        assert pick(form(family, dt=dt, masked=1), "selfroute", "stage1", "stage2", "can_fuse_combine") == (0, ST_GENERIC, ST_GENERIC, 0)
        if family != "deepseek":
            assert form(family, dt=dt, masked=1)["router"] == R_GATE_ROUTE_INDEX
        assert pick(form(family, dt=dt, ovr_out=1), "selfroute", "stage1", "stage2") == (0, ST_GENERIC, ST_GENERIC)
        assert pick(form(family, dt=dt, flags=ROUTE_ONLY, fast=0), "selfroute", "stage1", "stage2") == (0, ST_NONE, ST_NONE)
    assert form("deepseek", masked=1)["hide_shared"] == 1 and form("deepseek", masked=1)["router"] == R_GATE_SHARED1_ROUTE_SHARED2
    # NO_COMBINE: the gated families still self-route, stage 2 is the generic kernel; Switch's batch-1 forms need their combine
    assert pick(form("mixtral", flags=NO_COMBINE), "selfroute", "stage1", "stage2", "can_fuse_combine") == (1, ST_SELFROUTE, ST_GENERIC, 0)
    assert pick(form("switch", dt=F32, flags=NO_COMBINE), "selfroute", "layer1_switch", "stage1") == (0, 0, ST_GENERIC)
