"""fp8 slots without a GPU: the C interface (moeinf_create_ex / moeinf_slot_dtype, refusals that are decided before any device is
touched) and the gfx950 ISA of the fp8-weight kernel forms — the up-cast is the hardware conversion in registers, the weight stream
stays non-temporal 16-byte loads, nothing spills and no look-up table in LDS does the conversion."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "moe-infinity_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from moe_infinity_amd import load_library

    return load_library()


def test_header_declares_and_library_exports_the_fp8_slot_interface(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moeinf.h")).read(), flags=re.S)
    for name in ("moeinf_create_ex", "moeinf_slot_dtype"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert re.search(r"typedef struct moeinf_create_options \{\s*int32_t struct_bytes;\s*int32_t slot_dtype;\s*int32_t reserved\[6\];\s*\}", hdr)
    from moe_infinity_amd._lib import PROTOTYPES, CreateOptions

    assert C.sizeof(CreateOptions) == 32
    assert {"moeinf_create_ex", "moeinf_slot_dtype"} <= set(PROTOTYPES)


def _cfg(**kw):
    from moe_infinity_amd import _lib
    from moe_infinity_amd import config as Cf

    c = _lib.Config()
    c.abi_version = _lib.ABI_VERSION
    base = dict(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2, router_kind=Cf.ROUTER_MIXTRAL,
                dtype=Cf.DTYPE_F8E4M3, gate_dtype=Cf.DTYPE_BF16, device_memory_ratio=0.5, max_tokens=8, ep_size=1, policy=0)
    base.update(kw)
    for k, v in base.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("what,kw,reason", [
    ("bf16_dtype", dict(dtype=0, gate_dtype=0), "need fp8 experts"),
    ("nllb", dict(expert_type=2, router_kind=3), "Mixtral and DeepSeek experts only"),
    ("switch", dict(expert_type=0, router_kind=2, top_k=1), "Mixtral and DeepSeek experts only"),
    ("ep_size_2", dict(ep_size=2), "expert parallelism"),
    ("hidden_224", dict(hidden=224), "multiples of 64"),
    ("inter_96", dict(inter=96), "multiples of 64")])
def test_create_ex_refuses_what_fp8_slots_do_not_cover(lib, what, kw, reason):
    from moe_infinity_amd import _lib

    opts = _lib.CreateOptions()
    opts.struct_bytes = C.sizeof(opts)
    opts.slot_dtype = 3
    h = C.c_void_p()
    rc = lib.moeinf_create_ex(C.byref(_cfg(**kw)), C.byref(opts), C.byref(h))
    assert rc == 5 and not h.value, (what, rc)  # MOEINF_ERR_UNSUPPORTED, nothing created
    msg = lib.moeinf_last_error().decode()
    assert "fp8 slots" in msg and reason in msg, msg


def test_create_ex_checks_its_options(lib):
    from moe_infinity_amd import _lib

    h = C.c_void_p()
    opts = _lib.CreateOptions()
    opts.struct_bytes = 8
    opts.slot_dtype = 3
    assert lib.moeinf_create_ex(C.byref(_cfg()), C.byref(opts), C.byref(h)) == 1  # MOEINF_ERR_INVALID: struct_bytes
    opts.struct_bytes = C.sizeof(opts)
    opts.reserved[2] = 1
    assert lib.moeinf_create_ex(C.byref(_cfg()), C.byref(opts), C.byref(h)) == 1
    opts.reserved[2] = 0
    opts.slot_dtype = 2  # fp16 slots for fp8 experts: not built
    assert lib.moeinf_create_ex(C.byref(_cfg()), C.byref(opts), C.byref(h)) == 5
    v = C.c_int32()
    assert lib.moeinf_slot_dtype(None, C.byref(v)) == 1


# ---- ISA ------------------------------------------------------------------------------------------------
def _asm(tmp_path_factory, src):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / (src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)],
                   check=True, capture_output=True, timeout=900)
    return open(out).read().split("\n")


@pytest.fixture(scope="module")
def kernels_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "kernels.hip")


@pytest.fixture(scope="module")
def layer_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "layer_fused.hip")


def _bodies(lines, name_re):
    """every kernel whose mangled name matches -> its instruction lines (label to s_endpgm)"""
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S+):", l)
        if m and re.search(name_re, m.group(1)):
            end = next(j for j in range(i, len(lines)) if "s_endpgm" in lines[j])
            out[m.group(1)] = lines[i:end]
    return out


def _check_fp8_stream(name, body):
    code = [l.strip() for l in body if l.strip() and not l.strip().startswith((";", "."))]
    assert any(l.startswith("v_cvt_scalef32_pk_bf16_fp8") for l in code), f"{name}: no hardware fp8 -> bf16 conversion"
    nt = [i for i, l in enumerate(code) if l.startswith("global_load_dwordx4") and re.search(r"\bnt\b", l)]
    assert nt, f"{name}: the weights are not streamed with non-temporal 16-byte loads"
    mfma = [i for i, l in enumerate(code) if l.startswith("v_mfma")]
    assert mfma and any(mfma_i > nt[0] for mfma_i in mfma), name
    assert not any("scratch_" in l for l in code), f"{name}: scratch (register spills)"
    between = code[nt[0]:max(mfma) + 1]
    assert not any(re.match(r"ds_read_(u8|u16|i8|i16)", l) for l in between), f"{name}: an LDS look-up between the weight loads and the MFMAs"


@pytest.mark.parametrize("kernel", ["ffn1_selfroute_kernel", "ffn1_selfroute_multi_kernel", "ffn2_decode1_pair_kernel", "ffn2_decode1_kernel",
                                    "ffn_rows_kernel"])
def test_fp8_forms_of_the_row_dot_kernels(kernels_asm, kernel):
    bodies = _bodies(kernels_asm, r"^_ZN6moeinf\d+%sINS_5f8w_t" % kernel)
    assert bodies, f"no fp8-weight instantiation of {kernel}"
    for name, body in bodies.items():
        _check_fp8_stream(name, body)
    if kernel == "ffn_rows_kernel":  # every NW/U form, NT = 1 and NT = 4, both stages
        assert len(bodies) == 18, sorted(bodies)  # 2 stages x (7 NT = 1 forms + 2 NT = 4 forms)


def test_fp8_form_of_the_layer_front(layer_asm):
    bodies = _bodies(layer_asm, r"^_ZN6moeinf17moe_front1_kernelINS_5f8w_t")
    assert len(bodies) == 4, sorted(bodies)  # bf16 / fp32 gate x U = 4 / 8
    for name, body in bodies.items():
        _check_fp8_stream(name, body)


def test_fp8_slot_pull_keeps_four_loads_per_lane_in_flight(kernels_asm):
    """pull_retile_kernel<uint8_t, false>: fp8 host bytes straight into fp8 tiles, the tier mover's four 16-byte loads per lane in flight"""
    (name, body), = _bodies(kernels_asm, r"^_ZN6moeinf18pull_retile_kernelIhLb0EEE").items()
    ops = [l.strip() for l in body if re.search(r"global_load_dwordx4|s_waitcnt.*vmcnt\(\d+\)", l)]
    loads = [k for k, l in enumerate(ops) if "global_load_dwordx4" in l]
    assert len(loads) == 8, f"prologue + in-loop: two batches of four host loads expected, found {len(loads)}"
    for batch in (loads[:4], loads[4:]):
        assert batch == list(range(batch[0], batch[0] + 4)), "a wait sits between the four loads of a unit:\n" + "\n".join(ops)
    assert all("nt" in ops[k] for k in loads)
    assert not any("scratch_" in l for l in body)
    assert not any("v_cvt" in l and "fp8" in l for l in body), "an fp8 slot is filled with the bytes as they are"
