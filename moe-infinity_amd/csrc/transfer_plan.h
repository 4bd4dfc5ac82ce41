// transfer_plan.h — what the tier mover decides before it touches a device, as pure host functions (no HIP call):
//   weight_format   the three dtypes of an engine (arithmetic, host blob, HBM slot) or the refusal of the combination asked for
//   make_layout / make_dev_layout   the host blob and the tiled slot of one expert in those dtypes
//   transfer_plan   how one expert travels host -> slot: the mover's form, its steps in copy order, its events
// with MoverKnobs, every environment knob that steers them.  create_engine (engine.cpp) computes all of it once; issue_copy executes
// the plan.  moeinf_transfer_plan exports it and tests/test_transfer_plan_cpu.py pins it against tests/golden/transfer_plans.json
// (recorded from the stream commands of the control flow it replaced) and DESIGN.md section 5.1.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/moeinf.h"
#include "kernels.h"

using namespace moeinf;

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
static constexpr int64_t kAioAlignment = 4096;  // core/aio/archer_aio_utils.h kAioAlignment (model_topology.cpp:429-431)

// every environment knob of the tier mover: read once per moeinf_create* call and kept on the engine, per call by the export
struct MoverKnobs {
  static constexpr int kMaxFenceEvery = 32;  // (kMirrorPool / 4, engine_internal.h)
  int pull = 1;                 // MOEINF_H2D_PULL: 0 = experts travel through SDMA copies and the staging ring, not the pull kernel
  int64_t whole_blob_mb = 64;   // MOEINF_H2D_WHOLE_BLOB_MB: experts up to this size travel in one piece (0: always stage 1's tensors first)
  int pull_wgs = 16;            // MOEINF_H2D_PULL_WGS: workgroups per pull launch (>= 1; 8: -3 %, 32: -2...6 %, profiles/r06_tier_mover_pull_vs_sdma_ab.txt)
  int prealloc = 1;             // MOEINF_PREALLOC: 0 = an HBM slot is allocated by the first miss that needs it, not at creation
  int fence_every = 16;         // MOEINF_FENCE_EVERY: a sync-free forward records its fence every so many forwards (1..kMaxFenceEvery)
  int prefetch_window = 2;      // MOEINF_PREFETCH_WINDOW: experts in flight on the prefetch lane at most (>= 1)
  int aio_threads = 4;          // MOEINF_AIO_THREADS: threads of the disk tier's block reader
  static MoverKnobs from_env() {
    auto env = [](const char* n, int64_t d) { const char* v = getenv(n); return v ? atoll(v) : d; };
    MoverKnobs k;
    k.pull = env("MOEINF_H2D_PULL", k.pull) != 0; k.whole_blob_mb = env("MOEINF_H2D_WHOLE_BLOB_MB", k.whole_blob_mb);
    k.pull_wgs = std::max(1, (int)env("MOEINF_H2D_PULL_WGS", k.pull_wgs)); k.prealloc = env("MOEINF_PREALLOC", k.prealloc) != 0;
    k.fence_every = std::min(std::max(1, (int)env("MOEINF_FENCE_EVERY", k.fence_every)), kMaxFenceEvery);
    k.prefetch_window = std::max(1, (int)env("MOEINF_PREFETCH_WINDOW", k.prefetch_window));
    k.aio_threads = (int)env("MOEINF_AIO_THREADS", k.aio_threads);
    return k;
  }
};

// ---- the weight format ---------------------------------------------------------------------------------------------------------
// dt: arithmetic, activations, the shared expert; host_dt / slot_dt: the routed experts in the host tier (and on the link) / in their
// HBM slots — dt, DT_F8 or DT_MX4 each.  fp8 experts (the reference's dtype id 3, core/parallel/expert_module.h:23,118-119) are e4m3fn
// bytes in the host tier and a bf16 engine behind the tier mover: y = FFN(x; W.to(bf16)), what torch::linear over up-cast weights
// computes; with fp8 slots they stay e4m3fn in HBM, too.  MXFP4 slots: a bf16 engine whose routed experts are OCP MXFP4 in both tiers.
struct WeightFormat {
  int dt = DT_BF16, host_dt = DT_BF16, slot_dt = DT_BF16;
  int gate_dt = DT_BF16;  // the gate weight as moe_forward reads it (an fp8 gate_dtype with fp8 experts means bf16)
  int err = MOEINF_OK;    // MOEINF_ERR_UNSUPPORTED: the combination is refused, `why` says which part of it
  char why[256] = "";
};
// slot: moeinf_create_options.slot_dtype, < 0 when none was given (moeinf_create: slots in the arithmetic dtype).  fp8 and MXFP4 slots
// cover what their kernels cover (kernels.hip / layer_fused.hip: the row-dot forms and grouped GEMMs of the gated families, on whole
// 64-k / 128-k tiles, no expert parallelism); both, and fp8 experts, are moved by the pull form only.  dtype itself is validate()'s.
inline WeightFormat weight_format(int dtype, int gate_dtype, int slot, int expert_type, int router_kind, int ep_size, int H, int F, const MoverKnobs& k) {
  WeightFormat w;
  auto refuse = [&w](const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(w.why, sizeof w.why, fmt, ap);
    va_end(ap);
    w.err = MOEINF_ERR_UNSUPPORTED;
    return w;
  };
  const bool f8 = dtype == MOEINF_DTYPE_F8E4M3;
  w.dt = w.host_dt = w.slot_dt = f8 ? DT_BF16 : dtype;
  w.gate_dt = (f8 && gate_dtype == MOEINF_DTYPE_F8E4M3) ? DT_BF16 : gate_dtype;
  if (f8) w.host_dt = DT_F8;
  const char* kind = nullptr;  // the slot kind asked for, and the k of one of its tiles
  int tile = 0;
  if (slot == MOEINF_SLOT_MXFP4) {
    if (dtype != MOEINF_DTYPE_BF16) return refuse("mxfp4 slots need a bf16 engine (dtype %d, not %d): the experts are up-cast to bf16 in registers", MOEINF_DTYPE_BF16, dtype);
    if (gate_dtype != MOEINF_DTYPE_BF16 && gate_dtype != MOEINF_DTYPE_F32) return refuse("mxfp4 slots: gate_dtype %d is neither bf16 nor fp32", gate_dtype);
    kind = "mxfp4"; tile = 128; w.host_dt = w.slot_dt = DT_MX4;
  } else if (slot == MOEINF_DTYPE_F8E4M3) {
    if (!f8) return refuse("fp8 slots need fp8 experts (dtype %d, not %d)", MOEINF_DTYPE_F8E4M3, dtype);
    kind = "fp8"; tile = 64; w.slot_dt = DT_F8;
  } else if (slot >= 0 && slot != w.dt) {
    return refuse("slot_dtype %d with dtype %d: only fp8 slots (%d) for fp8 experts are built", slot, dtype, MOEINF_DTYPE_F8E4M3);
  }
  if (kind) {
    if (expert_type != MOEINF_EXPERT_MIXTRAL && expert_type != MOEINF_EXPERT_DEEPSEEK)
      return refuse("%s slots are built for Mixtral and DeepSeek experts only (expert_type %d)", kind, expert_type);
    if (router_kind != MOEINF_ROUTER_MIXTRAL && router_kind != MOEINF_ROUTER_SOFTMAX_TOPK && router_kind != MOEINF_ROUTER_DEEPSEEK && router_kind != MOEINF_ROUTER_DEEPSEEK_V3)
      return refuse("%s slots: router_kind %d is not one of the Mixtral / DeepSeek families'", kind, router_kind);
    if (ep_size != 1) return refuse("%s slots are not built for expert parallelism (ep_size %d)", kind, ep_size);
    if (H <= 0 || F <= 0 || H % tile || F % tile)
      return refuse("%s slots need hidden and inter to be multiples of %d (one %s tile: %d k), not %d / %d", kind, tile, kind, tile, H, F);
  }
  const bool mx4 = slot == MOEINF_SLOT_MXFP4;
  if (mx4)  // the tier mover re-orders the scales of whole row groups through 16 KiB of LDS (kernels.hip: mx4_scale_groups)
    for (int K : {H, F}) {
      const int KB = K / 128, ga = (KB % 4 == 0) ? 1 : ((KB % 2 == 0) ? 2 : 4);
      if (ga * KB * 64 > 16384) return refuse("mxfp4 slots: a reduction length of %d is too long for the tier mover's scale units", K);
    }
  // the fp8 pull loads 16 source bytes (sixteen elements) per lane: matrices' k and the bias vectors (NLLB, FSGPT: F and H elements)
  if (f8 && (H % 16 || F % 16)) return refuse("fp8 experts (dtype 3): hidden / inter (and bias lengths) must be multiples of 16");
  if ((f8 || mx4) && !k.pull)
    return refuse("%s travel by the PULL tier mover only: not with MOEINF_H2D_PULL=0", f8 ? "fp8 experts (dtype 3)" : "mxfp4 slots");
  return w;
}

// ---- blob layout ---------------------------------------------------------------------------------------------------------------
struct BlobLayout {
  int n = 0;
  int64_t off[4] = {0, 0, 0, 0}, size[4] = {0, 0, 0, 0};
  int64_t total = 0;
};
// host_dt == DT_MX4 (the routed experts of an MXFP4-slot engine; gated families only): every matrix is ONE tensor, its packed e2m1
// codes [R, K/2] followed by its e8m0 scales [R, K/32] (include/moeinf.h)
static BlobLayout make_layout(int expert_type, int64_t H, int64_t F, int host_dt) {
  BlobLayout b;
  const int64_t es = dt_bytes(host_dt);
  auto add = [&](int64_t bytes) {
    b.off[b.n] = b.total;
    b.size[b.n] = bytes;
    b.total += align_up(bytes, kAioAlignment);
    ++b.n;
  };
  switch (expert_type) {
    case MOEINF_EXPERT_MIXTRAL:   // w1[F,H] w2[H,F] w3[F,H]
    case MOEINF_EXPERT_DEEPSEEK:  // gate[F,H] up[F,H] down[H,F]
    case MOEINF_EXPERT_SWITCH_GATED:  // wi_0[F,H] wi_1[F,H] wo[H,F] (expert_module.cpp:46-52)
      if (host_dt == DT_MX4) { add(mx4_host_bytes(F, H)); add(mx4_host_bytes(F, H)); add(mx4_host_bytes(F, H)); break; }  // (= mx4_host_bytes(H, F))
      add(F * H * es); add(F * H * es); add(F * H * es);
      break;
    case MOEINF_EXPERT_NLLB:
    case MOEINF_EXPERT_FSGPT:  // fc1.w fc1.b fc2.w fc2.b
      add(F * H * es); add(F * es); add(H * F * es); add(H * es);
      break;
    case MOEINF_EXPERT_SWITCH:  // wi wo
      add(F * H * es); add(H * F * es);
      break;
    default: break;
  }
  return b;
}

// Device-side (HBM slot) layout: matrices in MFMA-tile order (kernels.hip), biases raw; 4 KiB aligned.  slot_dt: the SLOT's element
// (DT_F8 for fp8 slots: 64 k per 1-KiB tile, half of bf16's bytes; DT_MX4 for MXFP4 slots: 128 k per 1-KiB code tile and the matrix's
// scale dwords behind its code tiles, kernels.h tiled_bytes)
struct DevLayout {
  int n = 0;
  int64_t off[4] = {0, 0, 0, 0}, size[4] = {0, 0, 0, 0};
  int R[4] = {0, 0, 0, 0}, K[4] = {0, 0, 0, 0};  // K == 0: not a matrix (bias vector, copied as is)
  int64_t total = 0;
};
static DevLayout make_dev_layout(int expert_type, int64_t H, int64_t F, int slot_dt) {
  DevLayout d;
  auto mat = [&](int64_t R, int64_t K) {
    d.off[d.n] = d.total; d.R[d.n] = (int)R; d.K[d.n] = (int)K; d.size[d.n] = tiled_bytes(R, K, slot_dt);
    d.total += align_up(d.size[d.n], kAioAlignment); ++d.n;
  };
  auto vec = [&](int64_t n) {
    d.off[d.n] = d.total; d.R[d.n] = (int)n; d.K[d.n] = 0; d.size[d.n] = n * dt_bytes(slot_dt);
    d.total += align_up(d.size[d.n], kAioAlignment); ++d.n;
  };
  switch (expert_type) {
    case MOEINF_EXPERT_MIXTRAL: mat(F, H); mat(H, F); mat(F, H); break;
    case MOEINF_EXPERT_DEEPSEEK: case MOEINF_EXPERT_SWITCH_GATED: mat(F, H); mat(F, H); mat(H, F); break;
    case MOEINF_EXPERT_NLLB: case MOEINF_EXPERT_FSGPT: mat(F, H); vec(F); mat(H, F); vec(H); break;
    case MOEINF_EXPERT_SWITCH: mat(F, H); mat(H, F); break;
    default: break;
  }
  return d;
}

// ---- the transfer plan ---------------------------------------------------------------------------------------------------------
// The three movers.  PULL (kernels.hip: pull_retile_kernel): a kernel of the lane's COPY stream reads the pinned host blob and writes
// the tiled slot; it times itself in tick records (no queue packets).  The SDMA forms copy into the lane's staging ring
// (hipMemcpyAsync, copy stream) and re-tile from there (re-tile stream), bracketed by an event pair: the whole contiguous blob with
// one copy and one re-tile launch (as the reference copies it, model_topology.cpp:102-119), or tensor by tensor.
enum { MOVE_PULL = 0, MOVE_SDMA_BLOB = 1, MOVE_SDMA_TENSORS = 2 };
struct TransferStep {  // one launch (PULL, SDMA_BLOB) or one staged tensor (SDMA_TENSORS)
  int n = 0;
  int tensor[4] = {0, 0, 0, 0};                                      // indices into the layouts, in copy order
  int64_t src_off[4] = {0, 0, 0, 0}, dst_off[4] = {0, 0, 0, 0};      // ... their place in the host blob / the slot
  int64_t bytes[4] = {0, 0, 0, 0};                                   // ... their bytes in the host blob
  int R[4] = {0, 0, 0, 0}, K[4] = {0, 0, 0, 0};                      // ... as a RetileBlob takes them (K == 0: a vector of R 16-byte pieces)
  bool ready1_after = false;  // the tensors FFN stage 1 reads are in the slot: `ready1` is recorded behind this step
};
struct TransferPlan {
  int form = MOVE_PULL;
  int n_steps = 0;
  TransferStep step[4];
  bool one_event = false;     // no step records `ready1`: `ready` serves both stages (Node::ready1_is_ready), one event record less per copy
  bool src_f8 = false;        // up-cast on the way: fp8 host blob, bf16 slot (fp8 slots: bytes as they are)
  int pull_wgs = 16;
  bool write_on_copy = true;  // the stream the first write into the slot is ordered on, and `ready` recorded on: copy (PULL) or re-tile
  bool tick_timing = true;    // link-busy time from the pull kernels' tick records; false: from an event pair around the copies
  int64_t stage_bytes = 0;    // one staging buffer: the biggest tensor of a blob (the shared expert's up-cast ones included), or the whole blob
  int64_t h2d_bytes = 0;      // credited to moeinf_stats.h2d_bytes per transfer
};
// lay_sh: the shared expert's blob (n == 0: none); it is registered through the same staging buffers (moeinf_register_shared)
inline TransferPlan transfer_plan(const BlobLayout& lay, const DevLayout& dlay, const BlobLayout& lay_sh, int expert_type, const WeightFormat& w, const MoverKnobs& k) {
  TransferPlan p;
  // Copy order: what FFN stage 1 reads first (w1 AND w3 / gate AND up / fc1 + bias / wi), then the stage-2 tensors — so the compute
  // stream can start stage 1 while the down projection is still on the link.  n1: the stage-1 tensors.
  int order[4] = {0, 1, 2, 3}, n1 = 2;
  if (expert_type == MOEINF_EXPERT_MIXTRAL) { order[1] = 2; order[2] = 1; }  // w1 w3 | w2
  else if (expert_type == MOEINF_EXPERT_SWITCH) n1 = 1;                        // wi | wo
  // the pull kernel and the whole-blob re-tile move 16-byte pieces: no bias vector of another length
  bool vec_ok = true;
  for (int i = 0; i < dlay.n; ++i) if (dlay.K[i] == 0 && (dlay.size[i] % 16) != 0) vec_ok = false;
  // small experts travel in one piece (DeepSeek-V2-Lite's 16.5 MiB: 46 -> 54.5 GB/s, round 5 offload leg), big ones (Mixtral: 336 MiB)
  // stage 1's tensors first
  const bool whole = lay.total <= (k.whole_blob_mb << 20) && vec_ok;
  p.form = (k.pull && vec_ok) ? MOVE_PULL : (whole ? MOVE_SDMA_BLOB : MOVE_SDMA_TENSORS);
  p.write_on_copy = p.tick_timing = p.form == MOVE_PULL;
  p.src_f8 = w.host_dt == DT_F8 && w.slot_dt != DT_F8;
  p.pull_wgs = k.pull_wgs;
  auto add = [&](TransferStep& s, int i) {
    const int j = s.n++;
    s.tensor[j] = i; s.src_off[j] = lay.off[i]; s.dst_off[j] = dlay.off[i]; s.bytes[j] = lay.size[i];
    s.K[j] = dlay.K[i]; s.R[j] = dlay.K[i] > 0 ? dlay.R[i] : (int)(dlay.size[i] / 16);
  };
  if (p.form == MOVE_SDMA_TENSORS) {
    for (int j = 0; j < lay.n; ++j) { add(p.step[j], order[j]); p.step[j].ready1_after = j == n1 - 1; }
    p.n_steps = lay.n;
  } else if (p.form == MOVE_SDMA_BLOB || whole || n1 >= lay.n) {
    for (int j = 0; j < lay.n; ++j) add(p.step[0], p.form == MOVE_PULL ? order[j] : j);  // (the staged blob is re-tiled in layout order)
    p.n_steps = 1;
  } else {
    for (int j = 0; j < lay.n; ++j) add(p.step[j < n1 ? 0 : 1], order[j]);
    p.step[0].ready1_after = true;
    p.n_steps = 2;
  }
  p.one_event = p.n_steps == 1;
  for (int i = 0; i < 4; ++i)
    p.stage_bytes = std::max(p.stage_bytes, std::max(align_up(lay.size[i], kAioAlignment), align_up(lay_sh.size[i] * (w.host_dt == DT_F8 ? 2 : 1), kAioAlignment)));
  if (whole) p.stage_bytes = std::max(p.stage_bytes, align_up(lay.total, kAioAlignment));
  p.h2d_bytes = lay.total;
  return p;
}
