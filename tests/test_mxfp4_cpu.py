"""MXFP4 slots without a GPU: the quantiser (moe_infinity_amd.quant) against a restatement of the OCP MX rule, the C interface
(MOEINF_SLOT_MXFP4 through moeinf_create_ex, refusals decided before any device is touched), the gfx950 ISA of every MXFP4-weight
kernel form, and what ffn_form answers for the new slot kind — with the fp8 / bf16 answers for the same shapes pinned as they were
before MXFP4 slots existed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "moe-infinity_amd", "csrc")
SLOT_MXFP4 = 16


def _quant():
    # (the module is torch-only: loaded by path, so these tests need neither the library nor a build)
    spec = importlib.util.spec_from_file_location("_mxfp4_quant", os.path.join(ROOT, "moe-infinity_amd", "quant.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the quantiser ----------------------------------------------------------------------------------------
_TABLE = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)


def _restate(codes, scales):
    """16-entry table x 2^(b - 127), in float64, element 2j in the low nibble of byte j"""
    R, K2 = codes.shape
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(R, 2 * K2).long()
    return _TABLE[nib] * torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127).repeat_interleave(32, dim=1)


def _inputs():
    g = torch.Generator().manual_seed(4100)
    w = torch.randn(96, 512, generator=g) * 0.02
    w[3, 64:96] = 0.0                                     # an all-zero block
    w[5, :32] = torch.linspace(-7.9, 7.9, 32)             # every stretch of the grid and saturation, amax in [4, 8)
    w[6, :32] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0] * 4)   # exact ties (scale 2^0)
    w[7, 32:64] = torch.randn(32, generator=g) * 1e-30    # tiny
    w[8, 32:64] = torch.randn(32, generator=g) * 1e30     # huge
    w[9, :32] = 0.0
    w[9, 7] = -3.0                                        # one non-zero element
    return w


def test_quantize_follows_the_ocp_rule_and_its_error_bounds():
    q = _quant()
    w = _inputs()
    codes, scales = q.mxfp4_quantize(w)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    assert codes.shape == (96, 256) and scales.shape == (96, 16)
    assert int(scales.min()) >= 1 and int(scales.max()) <= 254, "scale bytes 0 and 255 are never emitted"
    what = _restate(codes, scales)
    x = w.double().reshape(96, 16, 32)
    amax = x.abs().amax(-1)
    # shared exponent: floor(log2(amax)) - 2, clamped; an all-zero block gets 127
    want_b = torch.where(amax == 0, torch.full_like(amax, 127.0), (torch.floor(torch.log2(amax.clamp_min(1e-300))) - 2 + 127).clamp(1, 254))
    assert torch.equal(scales.double(), want_b)
    assert torch.equal(what.reshape(96, 16, 32)[3, 2], torch.zeros(32, dtype=torch.float64)) and int(scales[3, 2]) == 127
    step = torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127).repeat_interleave(32, dim=1)  # 2^(b - 127)
    wd = w.double()
    inside = wd.abs() <= 6 * step
    # half of the grid's widest step (2 x 2^(b-127)) where the grid reaches, saturation at +-6 x 2^(b-127) above it
    assert bool(((wd - what).abs()[inside] <= step[inside]).all())
    assert bool((what[~inside] == torch.sign(wd[~inside]) * 6 * step[~inside]).all()) and int((~inside).sum()) > 0
    # nearest, ties to even, on the exact-tie row: 6 0.25 0.75 1.25 1.75 2.5 3.5 5 -> 6 0 1 1 2 2 4 4
    assert what[6, :8].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert what[9, 7].item() == -3.0 and int((what[9, :32] != 0).sum()) == 1


def test_dequantize_is_the_table_and_requantising_is_idempotent():
    q = _quant()
    w = _inputs()
    codes, scales = q.mxfp4_quantize(w)
    d32 = q.mxfp4_dequantize(codes, scales, torch.float32)
    assert torch.equal(d32.double(), _restate(codes, scales))
    c2, s2 = q.mxfp4_quantize(d32)
    assert torch.equal(c2, codes) and torch.equal(s2, scales), "re-quantising the dequantised weights gives the same bytes"
    # every dequantised value survives .to(bfloat16): two significant bits, bf16's exponent range
    dbf = q.mxfp4_dequantize(codes, scales)  # bfloat16 is the default
    assert dbf.dtype == torch.bfloat16
    assert torch.equal(dbf.float(), d32)
    # every (code, scale byte) pair of a range of scales, straight through dequantize
    allc = torch.arange(16, dtype=torch.uint8).repeat(16).reshape(1, 256)
    packed = (allc[:, 0::2] | (allc[:, 1::2] << 4)).repeat(15, 1).contiguous()
    sc = torch.arange(115, 130, dtype=torch.uint8).reshape(15, 1).repeat(1, 8).contiguous()
    d = q.mxfp4_dequantize(packed, sc, torch.float32)
    assert torch.equal(d.double(), _restate(packed, sc)) and torch.equal(d.to(torch.bfloat16).float(), d) and bool(torch.isfinite(d).all())


def test_quantize_rejects_shapes_it_cannot_block():
    q = _quant()
    with pytest.raises(ValueError):
        q.mxfp4_quantize(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        q.mxfp4_dequantize(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8))


# ---- the C interface --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from moe_infinity_amd import load_library

    return load_library()


def test_header_library_and_prototypes_agree(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moeinf.h")).read(), flags=re.S)
    assert re.search(r"\bMOEINF_SLOT_MXFP4\s*=\s*16\b", hdr)
    assert re.search(r"typedef struct moeinf_create_options \{\s*int32_t struct_bytes;\s*int32_t slot_dtype;\s*int32_t reserved\[6\];\s*\}", hdr)
    from moe_infinity_amd import _lib
    from moe_infinity_amd import config as Cf

    assert _lib.SLOT_MXFP4 == SLOT_MXFP4 == Cf.SLOT_MXFP4
    assert C.sizeof(_lib.CreateOptions) == 32
    assert {"moeinf_create_ex", "moeinf_slot_dtype", "moeinf_ffn_form"} <= set(_lib.PROTOTYPES)
    for name in ("moeinf_create_ex", "moeinf_slot_dtype", "moeinf_ffn_form"):
        assert hasattr(lib, name)
    import moe_infinity_amd.quant as Q

    assert callable(Q.mxfp4_quantize) and callable(Q.mxfp4_dequantize)
    with pytest.raises(ValueError):
        Cf.EngineConfig(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2,
                        router_kind=Cf.ROUTER_MIXTRAL, fp8_slots=True, mxfp4_slots=True)


def _cfg(**kw):
    from moe_infinity_amd import _lib
    from moe_infinity_amd import config as Cf

    c = _lib.Config()
    c.abi_version = _lib.ABI_VERSION
    base = dict(num_layers=1, num_experts=8, expert_type=Cf.EXPERT_MIXTRAL, hidden=256, inter=512, top_k=2, router_kind=Cf.ROUTER_MIXTRAL,
                dtype=Cf.DTYPE_BF16, gate_dtype=Cf.DTYPE_BF16, device_memory_ratio=0.5, max_tokens=8, ep_size=1, policy=0)
    base.update(kw)
    for k, v in base.items():
        setattr(c, k, v)
    return c


def _create_ex(lib, cfg, slot_dtype=SLOT_MXFP4):
    from moe_infinity_amd import _lib

    opts = _lib.CreateOptions()
    opts.struct_bytes = C.sizeof(opts)
    opts.slot_dtype = slot_dtype
    h = C.c_void_p()
    rc = lib.moeinf_create_ex(C.byref(cfg), C.byref(opts), C.byref(h))
    return rc, h, lib.moeinf_last_error().decode()


@pytest.mark.parametrize("what,kw,reason", [
    ("fp16_dtype", dict(dtype=2, gate_dtype=2), "bf16 engine"),
    ("fp32_dtype", dict(dtype=1, gate_dtype=1), "bf16 engine"),
    ("fp8_dtype", dict(dtype=3), "bf16 engine"),
    ("fp16_gate", dict(gate_dtype=2), "neither bf16 nor fp32"),
    ("hidden_8320_scale_units", dict(hidden=8320), "too long for the tier mover"),  # 65 k-tiles: four row groups' scales exceed 16 KiB
    ("nllb", dict(expert_type=2, router_kind=3), "Mixtral and DeepSeek experts only"),
    ("switch", dict(expert_type=0, router_kind=2, top_k=1), "Mixtral and DeepSeek experts only"),
    ("switch_router", dict(router_kind=2, top_k=1), "router_kind"),
    ("ep_size_2", dict(ep_size=2), "expert parallelism"),
    ("hidden_192", dict(hidden=192), "multiples of 128"),
    ("inter_320", dict(inter=320), "multiples of 128")])
def test_create_ex_refuses_what_mxfp4_slots_do_not_cover(lib, what, kw, reason):
    rc, h, msg = _create_ex(lib, _cfg(**kw))
    assert rc == 5 and not h.value, (what, rc)  # MOEINF_ERR_UNSUPPORTED, nothing created
    assert "mxfp4" in msg and reason in msg, msg


def test_create_ex_refuses_mxfp4_without_the_pull_mover(lib, monkeypatch):
    monkeypatch.setenv("MOEINF_H2D_PULL", "0")
    rc, h, msg = _create_ex(lib, _cfg())
    assert rc == 5 and not h.value
    assert "mxfp4" in msg and "MOEINF_H2D_PULL=0" in msg, msg


def test_dtype_4_and_the_slot_constant_as_a_dtype_stay_refused(lib):
    for dt in (4, SLOT_MXFP4):
        h = C.c_void_p()
        rc = lib.moeinf_create(C.byref(_cfg(dtype=dt, gate_dtype=0)), C.byref(h))
        assert rc == 5 and not h.value, dt
        rc, h, _ = _create_ex(lib, _cfg(dtype=dt, gate_dtype=0))
        assert rc == 5 and not h.value, dt


# ---- ffn_form ---------------------------------------------------------------------------------------------
# (dtype, epi, K, R, rows per expert) -> moeinf_ffn_form's fourteen numbers; 8 active experts, 256 CUs, flags 0, no knobs set.  The
# bf16 (0) and fp8-slot (3) rows were taken from the library as it was before MXFP4 slots.
_PINNED = {
    (0, 4, 4096, 14336, 1): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (0, 4, 4096, 14336, 16): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (0, 4, 4096, 14336, 17): [1, 4, 0, 0, 1, 4, 1, 0, 0, 0, 0, 0, 0, 0],
    (0, 4, 4096, 14336, 200): [3, 0, 0, 0, 0, 0, 0, 0, 0, 12, 1, 112, 768, 1024],
    (0, 4, 4096, 14336, 4096): [5, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0],
    (0, 0, 14336, 4096, 1): [0, 8, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (0, 0, 14336, 4096, 16): [0, 8, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (0, 0, 14336, 4096, 17): [3, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 32, 0, 256],
    (0, 0, 14336, 4096, 200): [3, 0, 0, 0, 0, 0, 0, 0, 0, 12, 0, 32, 0, 256],
    (0, 0, 14336, 4096, 4096): [5, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0],
    (3, 4, 4096, 14336, 1): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (3, 4, 4096, 14336, 16): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (3, 4, 4096, 14336, 17): [1, 4, 0, 0, 1, 4, 1, 0, 0, 0, 0, 0, 0, 0],
    (3, 4, 4096, 14336, 200): [3, 0, 0, 0, 0, 0, 0, 0, 0, 12, 1, 112, 768, 1024],
    (3, 4, 4096, 14336, 4096): [2, 8, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0],
    (3, 0, 14336, 4096, 1): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (3, 0, 14336, 4096, 16): [0, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (3, 0, 14336, 4096, 17): [3, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 32, 0, 256],
    (3, 0, 14336, 4096, 200): [3, 0, 0, 0, 0, 0, 0, 0, 0, 12, 0, 32, 0, 256],
    (3, 0, 14336, 4096, 4096): [2, 8, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0],
}
_KNOBS = [k for k in os.environ if k.startswith(("MOEINF_FFN_", "MOEINF_GEMM_", "MOEINF_RING"))]


def _form(lib, dt, epi, K, R, rows):
    out = (C.c_int32 * 14)()
    assert lib.moeinf_ffn_form(dt, epi, K, 0, R, 8, rows, 256, 0, out) == 0
    return list(out)


def test_ffn_form_keeps_its_bf16_and_fp8_answers(lib, monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k)
    for (dt, epi, K, R, rows), want in _PINNED.items():
        assert _form(lib, dt, epi, K, R, rows) == want, (dt, epi, K, R, rows)


@pytest.mark.parametrize("rows", [1, 16, 17, 200, 4096])
def test_ffn_form_gives_an_mxfp4_stage_the_row_kernel_at_every_row_count(lib, monkeypatch, rows):
    for k in _KNOBS:
        monkeypatch.delenv(k)
    for epi, K, R in ((4, 4096, 14336), (0, 14336, 4096)):
        f = _form(lib, SLOT_MXFP4, epi, K, R, rows)
        assert f[0] == 0, (rows, f)  # FFN_ROWS
        assert f[3] == (1 if rows <= 16 else 4), (rows, f)  # token tiles per pass: NT = 4 above 16 rows per expert
        assert f[1] in (4, 8, 16) and f[4:] == [0] * 10
    # a reduction that is not whole 128-k tiles, or an epilogue MXFP4 slots do not have: no kernel
    assert _form(lib, SLOT_MXFP4, 4, 4096 + 64, 14336, 1)[0] == -1
    assert _form(lib, SLOT_MXFP4, 3, 4096, 14336, 1)[0] == -1


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


def _check_mx4_stream(name, body, mask_byte=False, whole_dwords=True):
    """mask_byte: the kernel carries the generic router (its one byte load is the token's mask byte); whole_dwords: the form takes
    four or eight consecutive k-tiles per batch, so a lane's scales are whole dwords, shifted into place with v_alignbyte_b32"""
    code = [l.strip() for l in body if l.strip() and not l.strip().startswith((";", "."))]
    assert any(l.startswith("v_cvt_scalef32_pk_bf16_fp4") for l in code), f"{name}: no hardware fp4 -> bf16 conversion"
    nt = [i for i, l in enumerate(code) if l.startswith("global_load_dwordx4") and re.search(r"\bnt\b", l)]
    assert nt, f"{name}: the weights are not streamed with non-temporal 16-byte loads"
    mfma = [i for i, l in enumerate(code) if l.startswith("v_mfma")]
    assert mfma and any(mfma_i > nt[0] for mfma_i in mfma), name
    assert not any("scratch_" in l for l in code), f"{name}: scratch (register spills)"
    between = code[nt[0]:max(mfma) + 1]
    assert not any(re.match(r"ds_read_(u8|u16|i8|i16)", l) for l in between), f"{name}: an LDS look-up between the weight loads and the MFMAs"
    # the scales never come as one-byte (or two-byte) loads per tile: dwords, one per four tiles where a batch holds four
    narrow = [l for l in code if re.match(r"global_load_(u|s)(byte|short)", l)]
    assert len(narrow) <= (1 if mask_byte else 0), f"{name}: byte / short global loads {narrow}"
    assert any(re.match(r"global_load_dword\b", l) for l in code), f"{name}: no 4-byte loads"
    if whole_dwords:
        assert any(l.startswith("v_alignbyte_b32") for l in code), f"{name}: the scale dwords of a four-tile batch are not shifted into place"


@pytest.mark.parametrize("kernel", ["ffn1_selfroute_kernel", "ffn1_selfroute_multi_kernel", "ffn2_decode1_pair_kernel", "ffn2_decode1_kernel",
                                    "ffn_rows_kernel"])
def test_mxfp4_forms_of_the_row_dot_kernels(kernels_asm, kernel):
    bodies = _bodies(kernels_asm, r"^_ZN6moeinf\d+%sINS_6mx4w_t" % kernel)
    assert bodies, f"no MXFP4-weight instantiation of {kernel}"
    for name, body in bodies.items():
        whole = True
        if kernel == "ffn_rows_kernel":  # <mx4w_t, NMAT, NW, U, NT>: U = 1 / 2 forms, and the sixteen-wave gated form (two tiles per batch)
            nmat, nw, u, nt = (int(v) for v in re.search(r"mx4w_tELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups())
            whole = u % 4 == 0 and not (nmat == 2 and nw == 16)
        _check_mx4_stream(name, body, mask_byte=kernel == "ffn1_selfroute_multi_kernel", whole_dwords=whole)
    if kernel == "ffn_rows_kernel":  # every NW/U form, NT = 1 and NT = 4, both stages: as many as fp8 slots have
        fp8 = _bodies(kernels_asm, r"^_ZN6moeinf\d+ffn_rows_kernelINS_5f8w_t")
        assert len(bodies) == len(fp8) == 18, (sorted(bodies), sorted(fp8))


def test_mxfp4_form_of_the_layer_front(layer_asm):
    bodies = _bodies(layer_asm, r"^_ZN6moeinf17moe_front1_kernelINS_6mx4w_t")
    assert len(bodies) == 4, sorted(bodies)  # bf16 / fp32 gate x U = 4 / 8
    for name, body in bodies.items():
        _check_mx4_stream(name, body, mask_byte=True)


def test_mxfp4_slot_pull_keeps_four_loads_per_lane_in_flight(kernels_asm):
    """pull_retile_mx4_kernel: codes and scales of the host blob with the tier mover's four 16-byte loads per lane in flight"""
    (name, body), = _bodies(kernels_asm, r"^_ZN6moeinf22pull_retile_mx4_kernel").items()
    ops = [l.strip() for l in body if re.search(r"global_load_dwordx4|s_waitcnt.*vmcnt\(\d+\)", l)]
    loads = [k for k, l in enumerate(ops) if "global_load_dwordx4" in l]
    assert len(loads) == 8, f"prologue + in-loop: two batches of four host loads expected, found {len(loads)}"
    for batch in (loads[:4], loads[4:]):
        assert batch == list(range(batch[0], batch[0] + 4)), "a wait sits between the four loads of a unit:\n" + "\n".join(ops)
    assert all("nt" in ops[k] for k in loads)
    assert not any("scratch_" in l for l in body)
    assert not any("v_cvt" in l and "fp4" in l for l in body), "an MXFP4 slot is filled with the codes as they are"
