// kernels.h — launch wrappers of the gfx950 kernels (implemented in kernels.hip).
// Host code (engine.cpp, engine_ep.cpp) sees only these plain-C++ declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace moeinf {

enum { DT_BF16 = 0, DT_F32 = 1, DT_F16 = 2 };  // = the reference's dtype ids (core/parallel/expert_module.h:20-23)
// fp8 (OCP e4m3fn) as the dtype of an HBM SLOT only (fp8 slots, moeinf_create_ex): the weights of routed experts; activations and
// arithmetic stay bf16.  Never a stage's (activation) dtype.
constexpr int DT_F8 = 3;
// OCP MXFP4 (e2m1 codes, one e8m0 scale per 32 k of a row) as the dtype of an HBM SLOT only (MXFP4 slots, moeinf_create_ex with
// MOEINF_SLOT_MXFP4): like DT_F8 the weights of routed experts; activations and arithmetic stay bf16.  Not a dtype id of the C ABI.
constexpr int DT_MX4 = 4;
inline int dt_bytes(int dtype) { return dtype == DT_F32 ? 4 : (dtype == DT_F8 ? 1 : 2); }
// bytes of an [R, K] matrix in its MXFP4 HOST tensor: the packed codes [R, K/2], then the scales [R, K/32]
inline int64_t mx4_host_bytes(int64_t R, int64_t K) { return R * (K / 2) + R * (K / 32); }
struct EpFuse;

// ---- direct peer-store exchange (expert parallelism without a collective; host side: ep_peer.h) ------------------
// Every rank owns one exchange WINDOW in uncached device memory, mapped into every other rank's address space
// (hipIpc* between processes, plain pointers inside one process):
//   [0, 2048)     recv flags: word p * 32 = the last exchange whose rows from rank p have landed in this window
//   [2048, 4096)  ret flags:  word p * 32 = the last exchange whose expert outputs from owner p have landed
//   recv_off      [ep_size][cap_rows] rows of H activations + 16-byte tail (segment p is written by rank p)
//   ret_off       [ep_size][cap_rows] rows of H expert outputs            (segment p is written by owner p)
// Producers store rows STRAIGHT into the consumer's window (system-scope write-through stores), drain them
// (s_waitcnt vmcnt(0)), and publish the exchange number in the consumer's flag word; consumers poll their own flags.
// One flag word per cache line; the number only grows, so nothing is ever reset.
constexpr int EP_MAX_PEERS = 16;
constexpr int EP_FLAG_WORDS = 32;  // 128 bytes between two flag words
constexpr int64_t EP_RET_FLAGS_OFF = 2048, EP_WINDOW_HDR = 4096;
struct EpPeers {
  uint64_t base[EP_MAX_PEERS];  // window of rank p as mapped in THIS process (base[rank] = this rank's own)
  int64_t recv_off, ret_off;    // byte offsets of the two regions (the same on every rank)
  int64_t recv_row_bytes, ret_row_bytes;  // (H + tail) * element size, H * element size
  int64_t timeout_ticks;        // bound of every poll, wall_clock64 ticks (100 MHz); on expiry *err = 2 and the kernel goes on
  int32_t* done;                // arrival counter of many-workgroup producers (this device, zero between launches)
  int32_t* err;
  uint32_t epoch;               // number of this exchange (1, 2, ...)
  int64_t bcast_off;            // broadcast region: [ep_size] x bcast_stride bytes (the E gate logits of rank p's token)
  int bcast_stride;
  int rank, size, cap_rows;
  int on;                       // 0: the classic form (send buffer + a collective); the rest of the struct is unused
  int poll;                     // 1: consumer kernels poll their flags themselves; 0: a one-wave wait kernel runs in front
};
struct EpWait {  // poll `n` flag words (stride EP_FLAG_WORDS) until each has reached `epoch`
  const uint32_t* flags;
  int n;
  uint32_t epoch;
  int64_t timeout_ticks;
  int32_t* err;
};
hipError_t launch_ep_wait(const EpWait& w, hipStream_t st);

// epilogues of the row-dot (weight-streaming) FFN kernel
enum {
  EPI_NONE = 0,       // out = Tr(acc)                      (down / w2 / wo projections)
  EPI_BIAS = 1,       // out = Tr(Tr(acc) + bias)           (NLLB fc2)
  EPI_RELU = 2,       // out = relu(Tr(acc))                (Switch wi)
  EPI_BIAS_RELU = 3,  // out = relu(Tr(Tr(acc) + bias))     (NLLB fc1)
  EPI_GATED_SILU = 4, // out = Tr(Tr(silu(Tr(acc0))) * Tr(acc1))   (Mixtral w1/w3, DeepSeek gate/up)
  EPI_GATED_GELU = 5  // out = Tr(Tr(gelu(Tr(acc0))) * Tr(acc1))   (gelu-gated Switch wi_0/wi_1, expert_module.cpp:54-59; erf form = torch::gelu's
                      // default).  Round 5: runs the row kernel at every size (the tuned grouped GEMMs are built for the SiLU gate only).
};

struct CombineArgs {
  const void* x;            // [T,H] (Switch/NLLB passthrough)
  const void* y;            // [rows,H] expert outputs, expert-sorted
  void* out;                // [T,H]
  const int32_t* topk_idx;  // [T,K]
  const float* topk_w;      // [T,K]
  const int32_t* pair_slot; // [T,K]
  const int32_t* pair_order;// [T,K]
  const float* router_prob; // [T] Switch
  const void* y_shared;           // non-null: DeepSeek shared-expert outputs, row t at y_shared[(row0 + t) * H]
  const int32_t* shared_offsets;  // row0 = shared_offsets ? shared_offsets[shared_E] : 0 (device value)
  int shared_E;
  int T, H, K;
  int kind;                 // MOEINF_ROUTER_* (selects the reference block's combine semantics)
  int dtype;
};

// One stage (x -> h, or h -> y) of the grouped expert FFN for every active expert of a layer.
struct FfnStage {
  const void* in;          // B-operand rows: x [tokens, ld_in] (stage 1) or h [rows, ld_in] (stage 2)
  int64_t ld_in;           // elements
  const int32_t* row_map;  // stage 1: expert-sorted row -> token id (fused gather); nullptr: identity
  void* out;               // [rows, ld_out]
  int64_t ld_out;
  const int32_t* out_map;  // expert-sorted row -> output row (scatter fused into the epilogue); nullptr: identity
  const uint64_t* wptr;    // [E+1] device base pointer of every expert blob of this layer (0 = absent);
                           // entry E is the shared expert (DeepSeek) or 0
  const int32_t* active;   // [<= E+1] ids of experts with tokens, ascending
  const int32_t* n_active; // device scalar (used when n_active_host < 0)
  int n_active_host;       // >= 0: number of entries of `active` to process (chunked dispatch)
  const int32_t* counts;   // [E+1] rows per expert
  const int32_t* offsets;  // [E+2] first expert-sorted row of each expert
  int32_t* miss_flag;      // set to 1 if an active expert has wptr == 0
  int E;                   // number of routed experts (index of the shared pseudo-expert)
  int K, R;                // routed experts: reduction length, output rows
  int K_sh, R_sh;          // shared expert
  int64_t off_a, off_b, off_bias;           // byte offsets inside a routed expert blob
  int64_t off_a_sh, off_b_sh;               // inside the shared blob
  int epi;
  int dtype;
  // decode-sized fused combine (stage 2 of a forward with <= 16 tokens, Mixtral/DeepSeek combine semantics): the
  // LAST block to finish a 16-column tile of y (over all active experts; arrival counter + agent-scope fences)
  // combines those 16 columns for every token, so the combine needs no launch of its own and stays deterministic
  int fuse_combine;
  // DT_F8: the ROUTED experts' matrices are fp8 tiles (16 rows x 64 k per KiB, up-cast in registers); anything else: `dtype`.  The
  // shared expert (off_*_sh) is always `dtype`.  (Kept in what was padding in front of tile_done: the struct's size and layout stay.)
  int wdtype;
  int32_t* tile_done;      // [ceil(R/16)] arrival counters, zero between launches (the last block resets its own)
  CombineArgs comb;
  // batch-1 decode records (self-routing path): written by the meta block of ffn1_selfroute, read by ffn2_decode1
  uint64_t* dec_w;         // [8] blob pointer of the u-th active expert (ascending expert id)
  float* dec_cw;           // [8] the token's combine weight of that expert
  // ffn_gemm_ring2 with a split tail (set by its launcher): 1-D grid over units = (expert slot, 128-row block); units from
  // ring2_split on are dealt to TWO workgroups of four working waves each (64 rows), so a half-empty last round fills the chip
  int ring2_nblk;          // row blocks per expert (0: the plain 2-D grid)
  int ring2_split;
  // upper bound of the row index the stage reads from `in` (engine: max_tokens * (K + 1)); 0 = unknown.  ffn_gemm_ring2 keeps
  // element offsets into `in` in 32 bits: ffn_form does not pick it for a stage whose rows_bound * ld_in does not fit (round-4 advice)
  int64_t rows_bound;
};

// ---- which kernel, and which form of it, an FFN stage takes: pure host logic in plain C++ (engine.cpp includes this header).  ONE
// function, ffn_form, decides for every dtype; launch_ffn_stage (kernels.hip) and the introspection exports (moeinf_ffn_form,
// moeinf_ffn_ring2_form, moeinf_ffn_f8_gemm_form; engine.cpp) call it, and tests/test_ffn_form_cpu.py,
// tests/test_kernel_selection_cpu.py and tests/test_fp8_gemm_selection_cpu.py pin it against DESIGN.md section 4.3.  (Round 4: the
// launcher once asked for max_rows <= 192 where the sync-free path's estimate is 193 — the kernel silently never ran and six
// experiments measured its predecessor.)

// every environment knob that steers the choice (sweeps only): the launch path reads them once per process, the exports per call
struct FfnKnobs {
  int nw = 0;              // MOEINF_FFN_NW: waves per workgroup of the row kernel (0: by the rule in ffn_form)
  int u = 0;               // MOEINF_FFN_U: its unroll (0: 4)
  int nt = 0;              // MOEINF_FFN_NT: 1 = the row kernel at every size, > 1 = the grouped GEMMs at every size (0: by rows)
  int many_rows = 16;      // MOEINF_FFN_MANY_ROWS: up to here the row kernel (decode)
  int use_gemm = 2;        // MOEINF_FFN_GEMM: 0 = the row kernel's four-token-tile form, 1 = the register GEMM, 2 = by rows, 3 = hybrid
  int gemm_nt = 0;         // MOEINF_FFN_GEMM_NT: token groups per pass of the register GEMM (0: 4)
  int rgb_plain = 0;       // MOEINF_FFN_GEMM_RGB: row groups per LDS-kernel workgroup, plain stage (0: by the rule in ffn_form)
  int rgb_gated = 4;       // MOEINF_FFN_GEMM_RGB2: ... gated stage (MXFP4: always 4, the 128-row gated forms are not built)
  int big = 1;             // MOEINF_GEMM_BIG: 0 = never the 256 x 256 kernel
  int big_rows = 256;      // MOEINF_GEMM_BIG_ROWS: the 256 x 256 kernel above
  int hyb_rows = 0;        // MOEINF_GEMM_HYB_ROWS (0: 128 with <= 16 active experts, else 64)
  int hyb_kk = 4;          // MOEINF_GEMM_HYB_KK: k-tiles per stage of the hybrid kernel (2 or 4; MXFP4: always 4 = one code tile)
  int xl = 1;              // MOEINF_GEMM_XL: full-line activation staging (hybrid, LDS); an MXFP4 stage keeps it under 0 (only those forms are built)
  int wide = -1;           // MOEINF_GEMM_WIDE: the LDS kernel's 8 waves (-1: above 128 rows)
  int ring2_bits = 3;      // MOEINF_GEMM_RING2: bit 0 gated stage, bit 1 plain stage
  int ring2_min_k = 4096;  // MOEINF_RING_MIN_K
  int ring2_max_rows = 340;  // MOEINF_RING2_MAX_ROWS: above, a second pass over the weights begins -> the big-tile kernel
  int ring2_min_gated = 0;   // MOEINF_RING2_MIN_ROWS_GATED (0: where the hybrid kernel stops)
  int ring2_min_plain = 16;  // MOEINF_RING2_MIN_ROWS_PLAIN
  int ring2_tail = 1;        // MOEINF_RING2_TAIL: split a half-empty last round of the gated stage into half workgroups
  static FfnKnobs from_env() {
    auto env = [](const char* n, int d) { const char* v = getenv(n); return v && *v ? atoi(v) : d; };
    FfnKnobs k;
    k.nw = env("MOEINF_FFN_NW", k.nw); k.u = env("MOEINF_FFN_U", k.u); k.nt = env("MOEINF_FFN_NT", k.nt);
    k.many_rows = env("MOEINF_FFN_MANY_ROWS", k.many_rows); k.use_gemm = env("MOEINF_FFN_GEMM", k.use_gemm);
    k.gemm_nt = env("MOEINF_FFN_GEMM_NT", k.gemm_nt); k.rgb_plain = env("MOEINF_FFN_GEMM_RGB", k.rgb_plain);
    k.rgb_gated = env("MOEINF_FFN_GEMM_RGB2", k.rgb_gated); k.big = env("MOEINF_GEMM_BIG", k.big);
    k.big_rows = env("MOEINF_GEMM_BIG_ROWS", k.big_rows); k.hyb_rows = env("MOEINF_GEMM_HYB_ROWS", k.hyb_rows);
    k.hyb_kk = env("MOEINF_GEMM_HYB_KK", k.hyb_kk); k.xl = env("MOEINF_GEMM_XL", k.xl); k.wide = env("MOEINF_GEMM_WIDE", k.wide);
    k.ring2_bits = env("MOEINF_GEMM_RING2", k.ring2_bits); k.ring2_min_k = env("MOEINF_RING_MIN_K", k.ring2_min_k);
    k.ring2_max_rows = env("MOEINF_RING2_MAX_ROWS", k.ring2_max_rows);
    k.ring2_min_gated = env("MOEINF_RING2_MIN_ROWS_GATED", k.ring2_min_gated);
    k.ring2_min_plain = env("MOEINF_RING2_MIN_ROWS_PLAIN", k.ring2_min_plain); k.ring2_tail = env("MOEINF_RING2_TAIL", k.ring2_tail);
    return k;
  }
};
// rows per expert up to which the hybrid kernel runs (17 ..): 128 when at most 16 experts are active, else 64.  Measured: 17-64 rows
// (e.g. NLLB's 128 experts at a 2048-token batch) are too many for the row kernel and too few to amortise staging the weights in
// LDS (-15 % on that shape, sweep in profiles/); up to 128 rows with few active experts (big matrices, few workgroups — Mixtral at
// 192 / 256 / 320 tokens: down projection 213 -> 174, 227 -> 208, 232 -> 226 us; with NLLB's 128 experts at 4096 tokens the same
// switch costs +11 %)
inline int hyb_rows_for(int active, const FfnKnobs& k) { return k.hyb_rows ? k.hyb_rows : (active <= 16 ? 128 : 64); }

struct Ring2Form {
  int ntb = 0;    // 0: not ring2; else token groups per pass: 8 / 12 / 16 (128 / 192 / 256 tokens)
  int tail = 0;   // 1: 1-D grid with a split tail (gated stage only)
  int nblk = 0;   // row blocks (128 rows) per expert
  int split = 0;  // first unit that is dealt to two half workgroups
  int blocks = 0; // workgroups launched
};
// which form of ffn_gemm_ring2 a 2-byte stage takes.  f16: the gated stage starts at 65 rows there; row_groups = ceil(max(R, R_sh) /
// 16); active = grid.y (upper bound of experts with rows); max_rows: see launch_ffn_stage
inline Ring2Form ring2_form(bool f16, int nmat, int K, int K_sh, int row_groups, int active, int max_rows, int num_cus, const FfnKnobs& k) {
  Ring2Form f;
  if (!(k.ring2_bits & (nmat == 2 ? 1 : 2))) return f;
  const bool k_ok = (K % 64) == 0 && K >= k.ring2_min_k && (K_sh == 0 || ((K_sh % 64) == 0 && K_sh >= k.ring2_min_k));
  const int min_rows = nmat == 2 ? (k.ring2_min_gated ? k.ring2_min_gated : (f16 ? 64 : hyb_rows_for(active, k))) : k.ring2_min_plain;
  if (!k_ok || max_rows <= min_rows || max_rows > k.ring2_max_rows) return f;
  f.ntb = max_rows <= 128 ? 8 : (max_rows <= 208 ? 12 : 16);
  f.nblk = (row_groups + 7) / 8;
  const int units = f.nblk * active, rem = num_cus > 0 ? units % num_cus : 0;
  f.blocks = units;
  if (nmat == 2 && k.ring2_tail && units > num_cus && rem > 0 && rem <= num_cus / 2) {
    f.tail = 1; f.split = units - rem; f.blocks = units + rem;
  }
  return f;
}

// what the choice reads from an FfnStage
struct FfnShape {
  int dtype = DT_BF16;       // activation dtype: DT_BF16, DT_F16, anything else runs as fp32
  bool f8w = false;          // the routed experts' weights are an fp8 slot (FfnStage::wdtype == DT_F8)
  bool mx4w = false;         // ... an MXFP4 slot (FfnStage::wdtype == DT_MX4)
  bool mx4_gemm = false;     // ... of an engine with the MXFP4 grouped GEMMs switched on (moeinf_set_mxfp4_gemm; not in FfnStage, which
                             // is a kernel argument: launch_ffn_stage sets it from an argument of its own)
  int nmat = 1;              // 2: gated stage, 1: plain
  int epi = EPI_NONE;
  int K = 0, K_sh = 0;       // reduction lengths of the routed / shared experts (K_sh = 0: no shared expert in the launch)
  int row_groups = 0;        // ceil(max(R, R_sh) / 16) = grid.x
  bool out_aligned = true;   // ld_out % 8 == 0 (16-byte row stores)
  bool rows_fit = true;      // rows_bound * ld_in fits in 32 bits (ring2 keeps element offsets into the activations in 32 bits)
  bool fuse_combine = false;
  int64_t row_bytes = 0;     // bytes of one weight row, the longer of the routed and the shared expert's
};
inline FfnShape ffn_shape(const FfnStage& s) {
  FfnShape h;
  h.dtype = s.dtype;
  h.f8w = s.wdtype == DT_F8;
  h.nmat = (s.epi == EPI_GATED_SILU || s.epi == EPI_GATED_GELU) ? 2 : 1;
  h.epi = s.epi;
  h.K = s.K;
  h.K_sh = s.R_sh > 0 ? s.K_sh : 0;
  h.row_groups = ((s.R > s.R_sh ? s.R : s.R_sh) + 15) / 16;
  h.out_aligned = s.ld_out % 8 == 0;
  h.rows_fit = !(s.rows_bound > 0 && s.rows_bound * s.ld_in >= (int64_t(1) << 32));
  h.fuse_combine = s.fuse_combine != 0;
  h.row_bytes = (int64_t)(s.K > s.K_sh ? s.K : s.K_sh) * (h.f8w ? 1 : dt_bytes(s.dtype));
  if (s.wdtype == DT_MX4) {  // (the longer of the routed expert's code row and the bf16 shared expert's row)
    h.mx4w = true;
    h.row_bytes = s.K / 2 > (int64_t)s.K_sh * dt_bytes(s.dtype) ? s.K / 2 : (int64_t)s.K_sh * dt_bytes(s.dtype);
  }
  return h;
}

// FFN_NONE: an fp8 stage no kernel takes (launch_ffn_stage: hipErrorInvalidValue).  The numbers are those of the exports.
enum { FFN_NONE = -1, FFN_ROWS = 0, FFN_HYB = 1, FFN_LDS = 2, FFN_RING2 = 3, FFN_GEMM = 4, FFN_BIG = 5 };
struct FfnForm {
  int kernel = FFN_ROWS;  // ffn_rows_kernel | ffn_gemm_hyb_kernel | ffn_gemm_lds_kernel | ffn_gemm_ring2_kernel | ffn_gemm_kernel | ffn_gemm_big_kernel
  int nmat = 1;           // matrices per stage (2: gated)
  int waves = 0;          // per workgroup: rows 4 / 8 / 16, hybrid 4, LDS 4 / 8, register GEMM 4
  int unroll = 0;         // rows with one token tile: 2 / 4 / 8
  int nt = 0;             // token groups of 16 per pass: rows 1 / 4, register GEMM 4 / 8
  int rw = 0;             // hybrid: row groups per wave
  int kk = 0;             // hybrid: k-tiles per stage
  int xl = 0;             // hybrid, LDS: full-line activation staging
  int rgb = 0;            // LDS: row groups per workgroup
  int passes = 0;         // big: passes over the tokens one launch holds (at most 8)
  int num_cus = 0;        // big: compute units of the device (its short-pass rule)
  Ring2Form ring;         // ring2
};
// the LDS-staged kernel in 128-row blocks (else 64).  Plain stage: 128-row blocks need >= 2 blocks per CU to hide the DMA latency
inline bool lds_rows128(const FfnShape& s, int active, const FfnKnobs& k) {
  return s.nmat == 2 ? k.rgb_gated == 8 : (k.rgb_plain ? k.rgb_plain == 8 : ((s.row_groups + 7) / 8) * active >= 512 && s.K >= 4096);
}
// active = grid.y (upper bound of experts with rows); max_rows: see launch_ffn_stage
inline FfnForm ffn_form(const FfnShape& s, int active, int max_rows, int num_cus, const FfnKnobs& k) {
  FfnForm f;
  f.nmat = s.nmat;
  // fp8 slots: bf16 activations, whole fp8 tiles, and only the gated-SiLU and plain no-epilogue stages (Mixtral / DeepSeek)
  if (s.f8w && (s.dtype != DT_BF16 || s.K % 64 != 0 || (s.epi != EPI_GATED_SILU && s.epi != EPI_NONE))) { f.kernel = FFN_NONE; return f; }
  // MXFP4 slots: the same stages on whole 128-k code tiles
  if (s.mx4w && (s.dtype != DT_BF16 || s.K % 128 != 0 || (s.epi != EPI_GATED_SILU && s.epi != EPI_NONE))) { f.kernel = FFN_NONE; return f; }
  // the row kernel: long reductions get 8 waves per workgroup (more bytes in flight per CU), short ones 4 ... and a grid of at most
  // one workgroup per CU (Switch-base-8 at batch 1: 192 / 48 workgroups for 256 CUs) SIXTEEN: a CU that owns a single work item has
  // nothing else to hide its load latency behind, so the whole item goes in flight at once (round 4: stage 2 of Switch-base-8
  // streamed 9.45 MB in 16.8 us = 0.07 of HBM peak with 48 four-wave workgroups)
  const bool few = (int64_t)s.row_groups * active <= 256 && s.row_bytes / 64 >= 32 && !s.fuse_combine;
  const int nw = k.nw ? k.nw : (few ? 16 : (s.row_bytes >= 16384 ? 8 : 4));
  // it re-streams an expert's weights for every 16 rows: from 17 rows on, the GEMM kernels (one pass per 128/256 rows) win —
  // Mixtral at 64 tokens: 761 -> 549 us per layer (profiles/r01_ffn_sweep_midsize.txt)
  const bool many = !s.fuse_combine && (k.nt ? k.nt > 1 : max_rows > k.many_rows);
  if (!many) {
    const int u = k.u ? k.u : 4;
    f.nt = 1;
    f.waves = nw == 16 || nw == 8 ? nw : 4;
    f.unroll = nw != 16 && (u == 2 || u == 8) ? u : 4;
    return f;
  }
  // what the grouped GEMMs below decline: the row kernel looping four token tiles
  f.nt = 4;
  f.waves = nw == 8 ? 8 : 4;
  // the grouped GEMMs are built for the SiLU gate only: the gelu gate runs the row kernel at every size
  if (s.epi == EPI_GATED_GELU) return f;
  // ... and so does an MXFP4 slot of an engine that has not switched the MXFP4 grouped GEMMs on (moeinf_set_mxfp4_gemm; the default)
  if (s.mx4w && !s.mx4_gemm) return f;
  if (s.mx4w) {
    // MXFP4 with the switch on: the fp8 rule on the two forms that are built (ffn_gemm_mx4.hip: hybrid and LDS-staged, full-line
    // staging only; no ring2, no big kernel — DESIGN.md section 11).  The row kernel up to MOEINF_FFN_MANY_ROWS also under a forced
    // MOEINF_FFN_NT > 1, under MOEINF_FFN_GEMM=0, and with a shared expert whose reduction is not whole 128-byte lines (K_sh % 64;
    // K % 128 == 0 was checked above); fuse_combine never gets here.  The hybrid takes one code tile = four activation k-tiles per
    // stage (MOEINF_GEMM_HYB_KK does not apply), both keep xl = 1 under MOEINF_GEMM_XL=0, and the gated LDS form is 64-row blocks.
    // The 17-row and 128 / 64-row thresholds are the bf16 / fp8 ones.
    if (max_rows <= k.many_rows || k.use_gemm == 0 || s.K_sh % 64 != 0) return f;
    FfnForm g;
    g.nmat = s.nmat; g.xl = 1;
    if (k.use_gemm == 3 || max_rows <= hyb_rows_for(active, k)) {
      g.kernel = FFN_HYB; g.waves = 4; g.rw = s.nmat == 2 ? 1 : 2; g.kk = 4;
    } else {
      g.kernel = FFN_LDS;
      g.waves = (k.wide >= 0 ? k.wide != 0 : max_rows > 128) ? 8 : 4;
      g.rgb = s.nmat == 1 && lds_rows128(s, active, k) ? 8 : 4;
    }
    return g;
  }
  const int ept = (s.dtype == DT_BF16 || s.dtype == DT_F16) ? 32 : 16;  // activation elements per 64-byte k-tile
  const bool k_ok = s.K % ept == 0 && s.K_sh % ept == 0;
  int use_gemm = k.use_gemm;
  if (s.f8w) {
    // fp8: up to MOEINF_FFN_MANY_ROWS the row kernel even where a forced MOEINF_FFN_NT > 1 sends bf16 into the GEMMs (kept as it was).
    // No fp8 register GEMM: where bf16 takes it for a reduction that is not whole k-tiles (K_sh % 32), fp8 takes the row kernel.
    if (max_rows <= k.many_rows || !k_ok) return f;
    // kept as it was: under MOEINF_FFN_GEMM=1 (any value but 0 and 3) fp8 takes the hybrid / LDS / ring2 choice, bf16 the register GEMM
    if (use_gemm != 0 && use_gemm != 3) use_gemm = 2;
  }
  FfnForm g;
  g.nmat = s.nmat;
  // long reductions (K >= 4096: Mixtral's two stages, NLLB's second), 17 (plain) / hyb_rows+1 (gated) .. 340 rows per expert: the
  // software-pipelined register ring (ring2_form).  Measured against what ran there before (profiles/r04_ffn_sweep_ring2_*.txt,
  // Mixtral-8x7B, us per layer, gate-up / down):
  //   tokens   96       224       336       384       512       640       768       896
  //   before   320/162  337/196   365/233   404/252   441/261   494/274   492/342   510/347   (hybrid | ring + lds | big)
  //   ring2    (hyb)/147 (hyb)/157 (hyb)/173 347/178   374/202   401/233   438/256   487/287
  // gated stage below 129 rows: the hybrid kernel is 1-2 % ahead and stays.  Above ~256 rows per expert (the row estimate of the
  // sync-free path is 1.5 x the mean + 1 = 337 at 896 tokens, 385 at 1 024) a second pass over the weights begins and the big-tile
  // kernel takes over.  An expert with more rows than a pass holds takes another pass; correctness never depends on the estimate.
  // Kept as it was: fp16 tries the ring before it looks at MOEINF_FFN_GEMM.  fp8: ring2's fp8 form takes routed experts only (the
  // shared expert's weights are bf16), so not with a shared expert in the launch.
  const bool ring = s.f8w ? use_gemm == 2 && s.K_sh == 0 : (s.dtype == DT_F16 || (s.dtype == DT_BF16 && use_gemm == 2));
  if (ring && s.rows_fit) {
    g.ring = ring2_form(s.dtype == DT_F16, s.nmat, s.K, s.K_sh, s.row_groups, active, max_rows, num_cus, k);
    if (g.ring.ntb) { g.kernel = FFN_RING2; return g; }
  }
  // long prefills: the 256 x 256 / 32x32x16-MFMA kernel (ffn_gemm_big.hip; bf16 and fp16 — no fp8 form; 16-byte row stores).
  // Measured (profiles/r03_ffn_sweep_prefill_big_*.txt): it beats ffn_gemm_lds from 257 rows per expert on (Mixtral down projection
  // at 2048 tokens 846 -> 730 us, DeepSeek-V2-Lite at 4096 tokens 2.54 -> 1.96 ms per layer).  The register-ring kernel (gated
  // stage, K >= 4096) held out to ~640 rows against the first ping-pong version; with the short-last-pass variant the big kernel
  // wins from 257 rows on (Mixtral gate/up: 768 tokens 503 vs 535 us, 1024 tokens 647 vs 748, 1536 tokens 845 vs 1 031, 2048
  // tokens 1 010 vs 1 250), so both stages switch at the same row count now; below it (512 tokens: 436 vs 450 gate/up but 324 vs
  // 265 down) ring / lds stay
  if (use_gemm == 2 && k.big && !s.f8w && (s.dtype == DT_BF16 || s.dtype == DT_F16) && max_rows > k.big_rows && s.K % 64 == 0 &&
      s.K_sh % 64 == 0 && s.out_aligned) {
    const int passes = max_rows <= 256 ? 1 : (max_rows + 255) / 256;
    g.kernel = FFN_BIG; g.passes = passes > 8 ? 8 : passes; g.num_cus = num_cus;
    return g;
  }
  const bool xl = k.xl && s.K % (2 * ept) == 0 && s.K_sh % (2 * ept) == 0;
  if ((use_gemm == 3 || (use_gemm == 2 && max_rows <= hyb_rows_for(active, k))) && k_ok) {  // weights -> registers, activations -> LDS
    g.kernel = FFN_HYB; g.waves = 4; g.rw = s.nmat == 2 ? 1 : 2; g.kk = k.hyb_kk == 2 ? 2 : 4; g.xl = xl;
  } else if (use_gemm == 2 && k_ok) {  // LDS-staged
    g.kernel = FFN_LDS;
    g.waves = (k.wide >= 0 ? k.wide != 0 : max_rows > 128) ? 8 : 4;  // 8 waves: 256 tokens per pass over the weights
    // plain stage: 128-row blocks need >= 2 blocks per CU to hide the DMA latency; 64-row blocks otherwise
    g.rgb = lds_rows128(s, active, k) ? 8 : 4; g.xl = xl;
  } else if (use_gemm) {  // the register GEMM (never fp8: k_ok)
    // measured: (RG,NT)=(2,4)/(4,4) beats (1,8)/(2,8) at t_e ~128 (profiles/r01_ffn_sweep_prefill_gemm.txt)
    g.kernel = FFN_GEMM; g.waves = 4; g.nt = (k.gemm_nt ? k.gemm_nt : 4) <= 4 ? 4 : 8;
  } else {
    return f;
  }
  return g;
}

// ---- which launches make up a forward, and which form every decode launcher takes: the other half of the choice, again ONE pure
// function (layer_form).  moe_forward (engine.cpp) builds a LayerShape, calls it once and executes the answer; the decode launchers
// map its parts to their instantiations; moeinf_layer_form exports it and tests/test_layer_form_cpu.py pins it against
// tests/golden/layer_forms.json (recorded from the launches of the control flow it replaced) and DESIGN.md section 4.3.

// every environment knob that steers it (sweeps only): the launch path reads them once per process (layer_knobs), the export per call
struct LayerKnobs {
  int hide_shared = 1;             // MOEINF_HIDE_SHARED: 0 = the shared expert always runs behind the router
  int selfroute = 1;               // MOEINF_SELFROUTE: 0 = never the self-routing stage 1
  int selfroute_multi = 8;         // MOEINF_SELFROUTE_MULTI: tokens up to which a decode batch self-routes (at most 8; < 2: never)
  int selfroute_multi_pairs = 24;  // MOEINF_SELFROUTE_MULTI_PAIRS: ... and (token, expert) pairs (at most 64)
  int layer1_switch = 1;           // MOEINF_LAYER1_SWITCH: 0 = Switch batch 1 as three launches
  int front1 = -1;                 // MOEINF_FRONT1: 1 / 0 = the gate always / never in stage 1's launch (-1: with a hidden shared expert)
  int index_wide_pairs = 2048;     // MOEINF_INDEX_WIDE_PAIRS: more pairs than this take the many-workgroup index
  int fuse_combine = 1;            // MOEINF_FUSE_COMBINE: 0 = the combine is always a launch of its own
  int wide_out = 0;                // MOEINF_WIDE_OUT: 1 = the fused combine's hand-off rows leave as 16-byte stores (fuse mode 2)
  int layer1_sleep = 2;            // MOEINF_LAYER1_SLEEP: s_sleep(2) repetitions between two polls of a fused layer's counters (>= 1)
  int sr_lds_kb = -1;              // MOEINF_SR_LDS_KB: dynamic LDS per self-routing workgroup (-1: by the rule in selfroute_form)
  int sr_u = 0;                    // MOEINF_SR_U: its tiles per wave, matrix and batch, 8 or 4 (0: by the rule)
  int sr_order = 0;                // MOEINF_SR_ORDER: 1 = the hidden shared expert's work items are dispatched last
  int dec1_pair = 1;               // MOEINF_DEC1_PAIR: 0 = always the arrival-counter form; 8 = eight waves per expert (bf16)
  int dec1_pair_u = 4;             // MOEINF_DEC1_PAIR_U: tiles per wave and batch of the pair form: 2 (bf16) / 4 / 8
  int dec1_u = 4;                  // MOEINF_DEC1_U: ... of the arrival-counter form, short reductions: 4 / 8 / 12 (bf16)
  int dec1_switch_u = 12;          // MOEINF_DEC1_SWITCH_U: ... of its Switch form: 12 or 4
  int sh1_u = 8;                   // MOEINF_SH1_U: tiles per wave, matrix and batch of gate_shared1's four-wave form: 8 or 4
  int sh1_nw = 8;                  // MOEINF_SH1_NW: its waves per workgroup: 8 or 4
  int sh2_nw = 8;                  // MOEINF_SH2_NW: waves per workgroup of route_shared2: 4 / 8 / 16
  int sh2_u = 4;                   // MOEINF_SH2_U: its tiles per wave and batch: 4 or 8
  int gate_mfma_tiles = 128;       // MOEINF_GATE_MFMA_TILES: 16 x 16 logit tiles from which the gate runs on the fp64 MFMA (0: never)
  static LayerKnobs from_env() {
    auto env = [](const char* n, int d) { const char* v = getenv(n); return v ? atoi(v) : d; };
    LayerKnobs k;
    k.hide_shared = env("MOEINF_HIDE_SHARED", k.hide_shared); k.selfroute = env("MOEINF_SELFROUTE", k.selfroute);
    k.selfroute_multi = env("MOEINF_SELFROUTE_MULTI", k.selfroute_multi);
    k.selfroute_multi_pairs = env("MOEINF_SELFROUTE_MULTI_PAIRS", k.selfroute_multi_pairs);
    k.layer1_switch = env("MOEINF_LAYER1_SWITCH", k.layer1_switch); k.front1 = env("MOEINF_FRONT1", k.front1);
    k.index_wide_pairs = env("MOEINF_INDEX_WIDE_PAIRS", k.index_wide_pairs); k.fuse_combine = env("MOEINF_FUSE_COMBINE", k.fuse_combine);
    k.wide_out = env("MOEINF_WIDE_OUT", k.wide_out);
    k.layer1_sleep = env("MOEINF_LAYER1_SLEEP", k.layer1_sleep); if (k.layer1_sleep < 1) k.layer1_sleep = 1;
    k.sr_lds_kb = env("MOEINF_SR_LDS_KB", k.sr_lds_kb); k.sr_u = env("MOEINF_SR_U", k.sr_u); k.sr_order = env("MOEINF_SR_ORDER", k.sr_order);
    k.dec1_pair = env("MOEINF_DEC1_PAIR", k.dec1_pair); k.dec1_pair_u = env("MOEINF_DEC1_PAIR_U", k.dec1_pair_u);
    k.dec1_u = env("MOEINF_DEC1_U", k.dec1_u); k.dec1_switch_u = env("MOEINF_DEC1_SWITCH_U", k.dec1_switch_u);
    k.sh1_u = env("MOEINF_SH1_U", k.sh1_u); k.sh1_nw = env("MOEINF_SH1_NW", k.sh1_nw);
    k.sh2_nw = env("MOEINF_SH2_NW", k.sh2_nw); k.sh2_u = env("MOEINF_SH2_U", k.sh2_u);
    k.gate_mfma_tiles = env("MOEINF_GATE_MFMA_TILES", k.gate_mfma_tiles);
    return k;
  }
};
inline const LayerKnobs& layer_knobs() { static const LayerKnobs k = LayerKnobs::from_env(); return k; }  // the launch path's: read once

// router kinds and expert types as the choice reads them (= MOEINF_ROUTER_* / MOEINF_EXPERT_* of include/moeinf.h; engine.cpp asserts it)
enum { RK_MIXTRAL = 0, RK_DEEPSEEK = 1, RK_SWITCH = 2 };
enum { ET_SWITCH = 0, ET_MIXTRAL = 4, ET_DEEPSEEK = 5 };
constexpr int HIDE_SHARED_MAX_TOKENS = 16;  // forwards up to this many tokens hide the shared expert under the router
enum { LAYER_ROUTE_ONLY = 1, LAYER_NO_COMBINE = 2 };  // = MOEINF_FWD_*

// the plain values the choice reads: no pointers, no engine
struct LayerShape {
  int router_kind = RK_MIXTRAL;  // MOEINF_ROUTER_* as the engine keeps it (V3 and the no-renorm kinds folded into DEEPSEEK / MIXTRAL)
  int expert_type = ET_MIXTRAL;  // MOEINF_EXPERT_*
  int dtype = DT_BF16;           // activations (and the shared expert's weights)
  int gate_dtype = DT_BF16;
  int slot_dtype = DT_BF16;      // the routed experts' weights in their HBM slots: `dtype`, DT_F8 or DT_MX4
  int T = 1, K = 2, E = 8, H = 0, F = 0, Fs = 0;
  int has_shared = 0;
  int n_group = 1;
  int v3 = 0;                    // DeepSeek-V3's gate
  int capacity = 0;              // Switch per-row expert capacity (IndexArgs::capacity; <= 0: unlimited)
  int flags = 0;                 // LAYER_ROUTE_ONLY | LAYER_NO_COMBINE
  int masked = 0;                // the forward has a token mask
  int fast = 1;                  // sync-free path (MirrorPlan::fast); 0: the decision path
  int ovr_out = 0;               // stage 2 writes to an override buffer (expert-parallel owner side)
  int num_cus = 256;
  int l1_wgs_per_cu = 0;         // workgroups of the Switch one-launch kernel a CU holds (layer1_switch_wgs_per_cu, asked once; 0: unknown)
};

// decode-sized DeepSeek forwards: the shared expert (routing-independent, always resident) runs INSIDE the two router launches
// instead of behind them.  The one predicate for it: layer_form and the expert-parallel route (engine_ep.cpp) call it.
// (fp16 since round 5: gate_shared1 / route_shared2 / moe_front1 on half_t; fp32 experts keep the shared expert behind the router)
// (the gate is in the model dtype or fp32: moeinf_create refuses the mixed pairs)
inline bool can_hide_shared(const LayerShape& s, const LayerKnobs& k) {
  return k.hide_shared && s.has_shared && (s.dtype == DT_BF16 || s.dtype == DT_F16) && s.T <= HIDE_SHARED_MAX_TOKENS && s.T * s.K <= 64 &&
         s.router_kind == RK_DEEPSEEK;
}

// the gate's own form: GATE_MFMA = gate_logits_mfma_kernel, else gate_logits_kernel with TT = 1 / 4 tokens per workgroup.
// The fp64-matrix form from 128 (16-token x 16-expert) tiles on — below that its few workgroups lose to the decode-shaped
// kernel (measured: DeepSeek-V2-Lite 4096 / 512 / 128 tokens route 207 -> 75, 58 -> 47, 36 -> 39 us; NLLB 2048 tokens
// 195 -> 71; Mixtral, one padded tile: 4096 tokens 46 -> 30, 512 tokens 27 -> 39).  MOEINF_GATE_MFMA_TILES=0: never.
// One token (batch-1 decode, the gate launch in front of the self-routing stage 1): ONE cross-lane reduction per workgroup
// instead of four (the fp64 shuffles of the three absent tokens were most of the kernel: round 5, seen in the timelines of
// csrc/layer_fused.hip — gate done after 1.6 us instead of 2.6)
enum { GATE_NONE = 0, GATE_TT1 = 1, GATE_TT4 = 4, GATE_MFMA = 16 };
inline int gate_form(int T, int E, int H, const LayerKnobs& k) {
  if (k.gate_mfma_tiles > 0 && (int64_t)((T + 15) / 16) * ((E + 15) / 16) >= k.gate_mfma_tiles && (H & 63) == 0) return GATE_MFMA;
  return T == 1 ? GATE_TT1 : GATE_TT4;
}
// long prefills: the index over many workgroups (one workgroup walks 1024-pair chunks serially, ~12 us each); not with a Switch
// per-row capacity (a sequential pass).  moe_forward and launch_index_auto share it.
inline bool index_is_wide(int capacity, int64_t pairs, const LayerKnobs& k) { return capacity <= 0 && pairs > k.index_wide_pairs; }

struct RowsForm { int waves = 0, unroll = 0; };  // of a ffn_rows_item that rides in a router launch
// gate_shared1: 8 tiles per wave and matrix per batch: 1.035 -> 1.007 ms/token (DeepSeek-V2-Lite).  MOEINF_SH1_NW=8: eight waves per
// workgroup (a shared-expert work item of 16 rows x 2 matrices x K = 128 KB for DeepSeek-V2-Lite then goes in flight in ONE batch of
// loads per wave instead of two); round 4: 0.984 -> 0.968 ms/token (A/B/A in one run); 4 = the four-wave form.  fp16 model (round 5):
// the default eight-wave form only
inline RowsForm shared1_form(int dtype, const LayerKnobs& k) {
  if (dtype == DT_F16 || k.sh1_nw == 8) return {8, 8};
  return {4, k.sh1_u == 8 ? 8 : 4};
}
// route_shared2 (fp16: the default form only)
inline RowsForm shared2_form(int dtype, const LayerKnobs& k) {
  if (dtype == DT_F16) return {8, 4};
  return {k.sh2_nw == 16 ? 16 : (k.sh2_nw == 4 ? 4 : 8), k.sh2_u == 8 ? 8 : 4};
}

// the geometry of a self-routing stage 1, ONE rule for launch_ffn1_selfroute, launch_ffn1_selfroute_multi and launch_moe_front1
// (the expert-parallel broadcast stage 1, launch_ffn_epb_stage1 in ep_kernels.hip, keeps a copy of its LDS / tiles part: not a layer_form launch)
enum { ST_NONE = 0, ST_GENERIC = 1, ST_SELFROUTE = 2, ST_SELFROUTE_MULTI = 3, ST_FRONT1 = 4, ST_LAYER1_SWITCH = 5, ST_DECODE1 = 6 };
struct SelfRouteForm {
  int waves = 0;       // per workgroup: 4 (gated), 16 (plain experts: Switch)
  int tiles = 0;       // per wave, matrix and batch: 8 or 4
  int lds_kb = 0;      // dynamic LDS per workgroup (a cap on the workgroups resident per CU)
  int shared_last = 0; // the hidden shared expert's work items are dispatched last
  int grid = 0;
};
// launcher: ST_SELFROUTE / ST_SELFROUTE_MULTI / ST_FRONT1; gated: a gated-SiLU stage (else Switch's plain experts);
// n_rg / n_sh1 / n_sh2: row groups of the routed stage 1 and of the hidden shared expert's stages carried by the launch; slots: K
// (batch 1) or min(E, T * K) expert slots
inline SelfRouteForm selfroute_form(int launcher, bool gated, int dtype, int slot_dtype, int E, int slots, int n_rg, int n_sh1, int n_sh2,
                                    const LayerKnobs& k) {
  SelfRouteForm f;
  f.grid = (launcher == ST_FRONT1 ? E + n_sh1 : 0) + 1 + n_sh2 + slots * n_rg;
  if (!gated) {
    // plain experts (Switch, top-1): a grid of at most one workgroup per CU gets sixteen waves per workgroup — the whole
    // work item in flight at once (see ffn_form)
    f.waves = 16; f.tiles = 4;
    return f;
  }
  // Extra dynamic LDS per workgroup = a cap on the workgroups resident per CU.  A grid of several workgroups per CU
  // (Mixtral: 1793) streams best with FOUR resident per CU (8 + 30 KB of LDS each), the rest dispatched as they retire:
  // 3.942 / 3.935 / 3.920 / 3.891 / 3.939 ms per token at 7 / 6 / 5 / 4 / 3 per CU — fewer concurrent DRAM streams,
  // staggered finishes.  Small grids (DeepSeek: 657 workgroups, all resident anyway) are left alone.
  // Tiles per wave and matrix fetched per batch: 8 for grids that are resident all at once (DeepSeek-V2-Lite: 657
  // workgroups, 1.035 -> 1.009 ms/token), 4 for multi-round grids (Mixtral: 1793 workgroups at four per CU).
  // Kept as it was: the multi-token launcher follows the rule but neither MOEINF_SR_LDS_KB nor MOEINF_SR_U; MOEINF_SR_ORDER is
  // honoured by the batch-1 launcher with bf16 weights only.
  const bool multi_round = f.grid > 4 * 256, knobs = launcher != ST_SELFROUTE_MULTI;
  f.waves = 4;
  f.lds_kb = knobs && k.sr_lds_kb >= 0 ? k.sr_lds_kb : (multi_round ? 30 : 0);
  f.tiles = (knobs && k.sr_u ? k.sr_u : (multi_round ? 4 : 8)) == 8 ? 8 : 4;
  f.shared_last = launcher == ST_SELFROUTE && k.sr_order && n_sh2 > 0 && dtype == DT_BF16 && slot_dtype == DT_BF16;
  return f;
}

// the form of launch_ffn2_decode1 (stage 2 of a batch-1 self-routed forward, combine in its tail), ONE rule for bf16 / fp16 / fp32
// activations and fp8 / MXFP4 slots
struct Decode1Form {
  int pair = 0;    // 1: ffn2_decode1_pair_kernel (one workgroup owns 16 output columns for BOTH chosen experts), 0: the arrival-counter form
  int waves = 0;   // pair: per expert (the workgroup has twice as many); counter: per workgroup
  int unroll = 0;  // k-tiles per wave fetched per batch
  int grid_x = 0, grid_y = 0;
};
constexpr int DEC1_LONG_ROW_BYTES = 16384;  // a weight row of this many bytes gets eight waves per workgroup in the arrival-counter form
// kind: router kind (the combine's semantics); top_k = the token's experts; K / R: stage 2's reduction length / output rows;
// shared: the combine adds a shared expert's row
inline Decode1Form decode1_form(int dtype, int slot_dtype, int kind, int top_k, int K, int R, bool shared, const LayerKnobs& k) {
  Decode1Form f;
  const bool slot = slot_dtype == DT_F8 || slot_dtype == DT_MX4, b16 = dtype == DT_BF16 && !slot;
  f.grid_x = (R + 15) / 16;
  // K = 2 (Mixtral): 4 waves per expert (8 per CU), batches of 4 tiles: 38.9 us per Mixtral launch; 8 waves per expert 40.5; the
  // arrival-counter form 41.9.  Kept as it was: fp16 takes the default pair form only; MOEINF_DEC1_PAIR=8 and _PAIR_U=2 are bf16's.
  if (k.dec1_pair && top_k == 2 && kind <= RK_DEEPSEEK && !(kind == RK_DEEPSEEK && shared) &&
      (slot || ((dtype == DT_BF16 || dtype == DT_F16) && K % 32 == 0))) {
    f.pair = 1; f.grid_y = 1; f.waves = 4; f.unroll = 4;
    if (b16 && k.dec1_pair == 8) f.waves = 8;
    else if ((b16 || slot) && k.dec1_pair_u == 8) f.unroll = 8;
    else if (b16 && k.dec1_pair_u == 2) f.unroll = 2;
    return f;
  }
  // (K = 3..8 — DeepSeek: six routed experts + the hidden shared expert — keeps the arrival-counter form.  ONE workgroup per column
  // block with every chosen expert and the combine inside it was built twice: on half tiles, eight columns, 256 workgroups (round 3)
  // and on whole tiles, 128 workgroups of twelve waves (round 6); both measured slower than the tail they remove — 33.3 / 33.0-33.5
  // against 32.5 us per DeepSeek-V2-Lite layer, profiles/r06_deepseek_stage2_group_forms_rejected.txt — and both are deleted.)
  f.grid_y = top_k;
  if (kind == RK_SWITCH) {
    // Switch, top-1: H/16 workgroups (48 for Switch-base) of sixteen waves.  Twelve tiles per wave and batch: Switch-base's down
    // projection is 192 tiles per row group = 16 waves x 12, i.e. the workgroup's whole 197 KB in flight at once
    // (MOEINF_DEC1_SWITCH_U=4: three batches of four, 10.6 us per launch)
    f.waves = 16; f.unroll = k.dec1_switch_u == 12 ? 12 : 4;
    return f;
  }
  // by weight bytes per row: long reductions get eight waves per workgroup, short ones four and MOEINF_DEC1_U tiles per batch
  // (kept as it was: 12 is bf16's, fp16 takes 4 only)
  const int64_t row_bytes = slot_dtype == DT_MX4 ? K / 2 : (slot_dtype == DT_F8 ? K : (int64_t)K * 2);
  if (row_bytes >= DEC1_LONG_ROW_BYTES) { f.waves = 8; f.unroll = 4; return f; }
  f.waves = 4; f.unroll = 4;
  if ((b16 || slot) && k.dec1_u == 8) f.unroll = 8;
  else if (b16 && k.dec1_u == 12) f.unroll = 12;
  return f;
}

// what launch_moe_layer1_switch takes: x and experts in one dtype (fp32 for Switch-base, bf16), gate in the model dtype or fp32, every
// workgroup resident at once (what the chip HOLDS is asked — wgs_per_cu, an occupancy query —, not assumed; at most two per CU even
// if more fit), a reduction the four-way split covers.  R1 x K1 / R2 x K2: the two stages' matrices
inline bool layer1_switch_fits(int dtype, int gate_dtype, int slot_dtype, int E, int top_k, int R1, int K1, int R2, int K2, int num_cus,
                               int wgs_per_cu) {
  constexpr int KS = 4, P2 = 6, NW = 8;
  const int grid = E + 1 + (R1 + 15) / 16 + KS * ((R2 + 15) / 16), ept = dtype == DT_F32 ? 16 : 32;
  const int per_cu = wgs_per_cu > 0 ? (wgs_per_cu < 2 ? wgs_per_cu : 2) : 0;
  if (slot_dtype == DT_F8 || slot_dtype == DT_MX4 || dtype == DT_F16 || top_k != 1) return false;
  if (per_cu == 0 || grid > per_cu * num_cus || K2 % (ept * KS) != 0 || K1 % ept != 0 || K2 / ept / KS > NW * P2) return false;
  return dtype == DT_F32 ? gate_dtype == DT_F32 : (gate_dtype == DT_BF16 || gate_dtype == DT_F32);
}

// the router launches of a forward
enum {
  ROUTER_NONE = 0,              // nothing here: stage 1's launch carries the gate (front1, the Switch one-launch layer)
  ROUTER_GATE = 1,              // the gate; stage 1 routes for itself
  ROUTER_GATE_SHARED1 = 2,      // ... with the hidden shared expert's stage 1 in the gate launch
  ROUTER_GATE_SHARED1_ROUTE_SHARED2 = 3,  // gate + shared stage 1, then top-k + index + shared stage 2
  ROUTER_GATE_ROUTE_INDEX = 4,  // gate, then top-k + dispatch index in one launch (up to 64 tokens)
  ROUTER_GATE_TOPK_INDEX = 5,   // gate, top-k, the one-workgroup index
  ROUTER_GATE_TOPK_WIDE = 6     // gate, top-k, the many-workgroup index (three launches)
};
enum { SR_NONE = 0, SR_BATCH1 = 1, SR_MULTI = 2 };
enum { L1_NO = 0, L1_ONE_LAUNCH = 1, L1_DECLINED = 2 };  // declined: chosen, but the launcher does not take the shape — the three launches
struct LayerForm {
  int hide_shared = 0;
  int selfroute = SR_NONE;
  int front1 = 0;
  int layer1_switch = L1_NO;
  int router = ROUTER_GATE_ROUTE_INDEX;
  int gate = GATE_NONE;        // form of a gate launch of its own (GATE_NONE: the gate rides in another launch; gate_shared1 is TT = 4)
  int stage1 = ST_GENERIC;     // ST_NONE (route only) | ST_GENERIC (launch_ffn_stage: ffn_form) | ST_SELFROUTE | ST_SELFROUTE_MULTI | ST_FRONT1 | ST_LAYER1_SWITCH
  SelfRouteForm sr;            // ST_SELFROUTE / _MULTI / ST_FRONT1
  int stage2 = ST_GENERIC;     // ST_NONE (route only, inside the one-launch layer) | ST_GENERIC | ST_DECODE1
  Decode1Form dec1;            // ST_DECODE1
  RowsForm shared1, shared2;   // gate_shared1 / route_shared2, where the router launches them
  int can_fuse_combine = 0;    // stage 2 may carry the combine in its epilogue (decision path: when the layer runs as one chunk)
  int fuse_mode = 1;           // FfnStage::fuse_combine of such a stage 2
  int kt1 = 1;                 // stage 1 is ONE launch and carries the profiling timer on its own dispatch packet
  int poll_sleep = 0;          // ST_FRONT1 / ST_LAYER1_SWITCH: s_sleep(2) repetitions between two polls of a counter (LayerSync::sleep)
};
inline LayerForm layer_form(const LayerShape& s, const LayerKnobs& k) {
  LayerForm f;
  const int T = s.T, K = s.K, E = s.E;
  const bool route_only = s.flags & LAYER_ROUTE_ONLY, no_combine = s.flags & LAYER_NO_COMBINE;
  const bool hide = !route_only && can_hide_shared(s, k);
  f.hide_shared = hide;
  // batch-1 decode on the sync-free path (gated families, bf16): no top-k/index launch at all — FFN stage 1 routes for
  // itself from the gate logits (ffn1_selfroute_kernel) and one extra block of it writes the routing outputs
  const bool sr_gated = s.dtype != DT_F32 &&
                        (s.router_kind == RK_MIXTRAL || (s.router_kind == RK_DEEPSEEK && s.n_group <= 1 && !s.v3)) &&
                        (s.expert_type == ET_MIXTRAL || s.expert_type == ET_DEEPSEEK) && (!s.has_shared || hide);
  // (round 4) Switch: top-1, plain ReLU experts, bf16 or fp32; a single token can never exceed the per-row capacity
  const bool sr_switch = s.router_kind == RK_SWITCH && s.expert_type == ET_SWITCH && K == 1 && !s.has_shared && !no_combine && s.capacity != 0;
  // (round 4) decode batches of 2..8 tokens of the gated families: the same idea, every workgroup routes every token
  // Measured (profiles/r04_small_batch_selfroute.txt): DeepSeek-V2-Lite batch 2 / 4: 1.530 -> 1.373 / 2.163 -> 2.056 ms per step;
  // batch 8 (48 pairs over 64 experts): 3.17 -> 3.61 — every workgroup of the worst-case grid (48 expert slots) pays eight
  // routings before it knows that its slot is empty.  Hence at most 24 (token, expert) pairs; Mixtral (8 experts, all of them
  // active from batch 4 on) gains 2.3 / 0.9 / 0.6 % at batch 2 / 4 / 8.
  const bool sr_multi = T >= 2 && T <= (k.selfroute_multi < 8 ? k.selfroute_multi : 8) &&
                        T * K <= (k.selfroute_multi_pairs < 64 ? k.selfroute_multi_pairs : 64) && sr_gated;
  // A token mask takes the generic router launches (route_core reads the mask): the self-routing forms (selfroute, multi,
  // moe_front1, the Switch one-launch layer) and the fused combine assume every token keeps its K experts, so stage 2 always runs.
  const bool selfroute = k.selfroute && !s.masked && !route_only && s.fast && K <= 8 && E <= 64 && !s.ovr_out &&
                         ((T == 1 && (sr_gated || sr_switch)) || sr_multi);
  f.selfroute = !selfroute ? SR_NONE : (T == 1 ? SR_BATCH1 : SR_MULTI);
  // decode-sized Mixtral/DeepSeek forwards (every token keeps K experts, so stage 2 always runs): the combine
  // rides in the epilogue of FFN stage 2.  (Switch: only the batch-1 stage 2 knows its combine)
  f.can_fuse_combine = !route_only && k.fuse_combine && !no_combine && T <= 16 && !s.masked &&
                       (s.router_kind == RK_MIXTRAL || s.router_kind == RK_DEEPSEEK || (selfroute && sr_switch));
  // FfnStage::fuse_combine: 1 = the hand-off rows leave as sixteen 2-byte write-through stores; 2 (MOEINF_WIDE_OUT=1) = gathered
  // through LDS into 16-byte ones — measured SLOWER (DeepSeek-V2-Lite 1.031/1.038 vs 1.022/1.031 ms/token, stage 2 +0.6 us: the
  // extra LDS round trip and barrier cost more than the fabric writes they save), so off by default
  f.fuse_mode = k.wide_out ? 2 : 1;
  // (the whole DeepSeek layer as ONE persistent launch was built in round 5, measured slower — 1.09 vs 0.958 ms/token — and
  // removed in round 6: DESIGN.md section 4.5.1 keeps the analysis)
  // Switch (top-1, no shared expert): the one-launch form is the DEFAULT — three launches of 3-10 us for 18.9 MB are pure fixed
  // cost, and with hardly any traffic in flight a flag costs ~1 us (MOEINF_LAYER1_SWITCH=0: the three launches)
  if (k.layer1_switch && selfroute && T == 1 && sr_switch && !sr_gated && !no_combine && s.dtype != DT_F16)
    f.layer1_switch = f.can_fuse_combine && layer1_switch_fits(s.dtype, s.gate_dtype, s.slot_dtype, E, K, s.F, s.H, s.H, s.F, s.num_cus, s.l1_wgs_per_cu)
                          ? L1_ONE_LAUNCH : L1_DECLINED;
  // the gated families: the gate (and the hidden shared expert) can ride in FRONT of the self-routing stage 1, in the same
  // launch (round 5, launch_moe_front1).  Measured A/B/A/B (profiles/r05_front1_gate_and_stage1_in_one_launch.txt): DeepSeek-V2-Lite
  // 0.949-0.967 -> 0.937 ms/token (two launches per layer instead of three) = the default with a hidden shared expert; Mixtral
  // 3.708-3.726 -> 3.723-3.728 (nothing: the hop costs what the gate launch cost) = off unless MOEINF_FRONT1=1; =0: never
  f.front1 = (k.front1 < 0 ? hide : k.front1 != 0) && selfroute && T == 1 && sr_gated && s.dtype != DT_F32 && (hide || !s.has_shared) &&
             (s.gate_dtype == s.dtype || s.gate_dtype == DT_F32);
  const bool one_launch = f.layer1_switch == L1_ONE_LAUNCH;
  if (one_launch || f.front1) f.router = ROUTER_NONE;
  else if (selfroute) f.router = hide ? ROUTER_GATE_SHARED1 : ROUTER_GATE;
  else if (hide) f.router = ROUTER_GATE_SHARED1_ROUTE_SHARED2;
  else if (T <= 64) f.router = ROUTER_GATE_ROUTE_INDEX;  // decode: top-k + dispatch index in one launch
  else f.router = index_is_wide(s.capacity, (int64_t)T * K, k) ? ROUTER_GATE_TOPK_WIDE : ROUTER_GATE_TOPK_INDEX;
  if (f.router == ROUTER_GATE_SHARED1 || f.router == ROUTER_GATE_SHARED1_ROUTE_SHARED2) f.shared1 = shared1_form(s.dtype, k);
  else if (f.router != ROUTER_NONE) f.gate = gate_form(T, E, s.H, k);
  if (f.router == ROUTER_GATE_SHARED1_ROUTE_SHARED2) f.shared2 = shared2_form(s.dtype, k);
  if (route_only) { f.stage1 = f.stage2 = ST_NONE; return f; }
  f.stage1 = one_launch ? ST_LAYER1_SWITCH : (f.front1 ? ST_FRONT1 : (!selfroute ? ST_GENERIC : (T > 1 ? ST_SELFROUTE_MULTI : ST_SELFROUTE)));
  if (f.stage1 == ST_SELFROUTE || f.stage1 == ST_SELFROUTE_MULTI || f.stage1 == ST_FRONT1)
    f.sr = selfroute_form(f.stage1, !sr_switch, s.dtype, s.slot_dtype, E, T == 1 ? K : (E < T * K ? E : T * K), (s.F + 15) / 16,
                          hide && f.front1 ? (s.Fs + 15) / 16 : 0, hide ? (s.H + 15) / 16 : 0, k);
  f.stage2 = one_launch ? ST_NONE : (selfroute && f.can_fuse_combine && T == 1 ? ST_DECODE1 : ST_GENERIC);
  if (f.stage2 == ST_DECODE1) f.dec1 = decode1_form(s.dtype, s.slot_dtype, s.router_kind, K, s.F, s.H, s.has_shared != 0, k);
  // decode launchers that carry the timer on their own dispatch packet: no event-record packets inside the interval
  // (every FFN-stage launcher is ONE launch and carries the timer; the small-batch self-routing stage 1 is the exception)
  f.kt1 = f.stage1 != ST_SELFROUTE_MULTI;
  if (f.stage1 == ST_FRONT1 || f.stage1 == ST_LAYER1_SWITCH) f.poll_sleep = k.layer1_sleep;
  return f;
}

// max_rows_per_expert: upper bound of rows any one expert receives (selects the kernel and its form); num_cus: of the device
// mx4_gemm: FfnShape::mx4_gemm (read for MXFP4 slots only); kernel_out: if not NULL, the FFN_* id the stage took
hipError_t launch_ffn_stage(const FfnStage& s, int max_active, int max_rows_per_expert, int num_cus, hipStream_t st, bool mx4_gemm = false,
                            int* kernel_out = nullptr);
// the grouped GEMMs, one launcher per translation unit: each maps the form ffn_form chose to its instantiation
void launch_ffn_gemm(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);             // ffn_gemm.hip: bf16, fp32
void launch_ffn_gemm_f16(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);         // ffn_gemm_f16.hip
void launch_ffn_gemm_f8(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);          // ffn_gemm_f8.hip: fp8 slots
void launch_ffn_gemm_mx4(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);         // ffn_gemm_mx4.hip: MXFP4 slots (hybrid, LDS)
void launch_ffn_gemm_ring2_bf16(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);  // ffn_gemm_ring2.hip
void launch_ffn_gemm_ring2_f16(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);   // ffn_gemm_ring2_f16.hip
void launch_ffn_gemm_big(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st);         // ffn_gemm_big.hip: bf16, fp16
// row-major [R,K] -> MFMA A-operand tiles (see kernels.hip); dst needs tiled_bytes(R,K) bytes
hipError_t launch_retile(const void* src, void* dst, int R, int K, int dtype, hipStream_t st);
// all tensors of one staged blob in one launch: tensor t = (src + src_off[t]) row-major [R, K] -> (dst + dst_off[t]) tiled;
// K == 0: a vector of R 16-byte pieces, copied as is
struct RetileBlob {
  const void* src;
  void* dst;
  int n;
  int64_t src_off[4], dst_off[4];
  int R[4], K[4];
  int src_f8;  // pull form only: the source blob holds fp8 (e4m3fn) elements, the slot bf16 (1 source byte per destination element)
               // (an fp8 SLOT — launch_pull_retile with dtype DT_F8 — copies the bytes as they are: src_f8 = 0)
};
hipError_t launch_retile_blob(const RetileBlob& b, int dtype, hipStream_t st);
// the same from PINNED HOST memory (b.src = device-visible host pointer): the tier mover's pull form, `workgroups` x 256 threads
// ts: nullptr, or a 4 x u64 timing record in device memory {start tick of the copy's first launch (written when first != 0), max end tick, finished workgroups, -}
hipError_t launch_pull_retile(const RetileBlob& b, int dtype, int workgroups, hipStream_t st, unsigned long long* ts = nullptr, int first = 1);
inline int64_t tiled_bytes(int64_t R, int64_t K, int dtype) {
  // an MXFP4 slot: code tiles of 16 rows x 128 k (K % 128 == 0), then one scale dword per lane and FOUR consecutive tiles (kdev.h)
  if (dtype == DT_MX4) { const int64_t tiles = ((R + 15) / 16) * (K / 128); return tiles * 1024 + ((tiles + 3) / 4) * 256; }
  const int64_t ept = dtype == DT_F32 ? 16 : (dtype == DT_F8 ? 64 : 32);
  return ((R + 15) / 16) * ((K + ept - 1) / ept) * 1024;
}

struct RouteArgs {
  const void* x;        // [T,H] dtype x_dtype
  const void* gate_w;   // [E,H] dtype gate_dtype
  float* logits;        // [T,E]
  int T, H, E, K;
  int x_dtype, gate_dtype;
  int kind;             // MOEINF_ROUTER_*
  int norm_topk_prob;
  float scale;
  int n_group, topk_group;
  int32_t* topk_idx;    // [T,K]
  float* topk_w;        // [T,K]
  int32_t* pair_valid;  // [T,K]
  int32_t* pair_order;  // [T,K] k-indices sorted by ascending expert id
  float* router_prob;   // [T] (Switch: max prob)
  int v3;               // kind DEEPSEEK only: 1 = DeepSeek-V3's gate (sigmoid scores, e_score_correction_bias, top-2-sum groups; modeling_deepseek_v3 MoEGate)
  const float* e_bias;  // ... its e_score_correction_bias [E] (fp32, device), or nullptr = zeros
  int no_renorm;        // kind MIXTRAL only: 1 = the top-k probabilities are NOT renormalised (Grok / Arctic, grok.py:38-45)
  const uint8_t* token_mask;  // [T] device bytes, 0 = masked token (every pair dropped, no slot), or nullptr = all tokens real
};
hipError_t launch_gate_logits(const RouteArgs& a, hipStream_t st);
hipError_t launch_route_topk(const RouteArgs& a, hipStream_t st);

struct IndexArgs {
  const int32_t* topk_idx;  // [T,K]; entries < 0 are never dispatched
  int idx_stride;           // distance between consecutive entries of topk_idx in int32 units (0/1: contiguous)
  int32_t* pair_valid;      // [T,K] in/out (Switch capacity clears entries); nullptr: all valid
  int T, K, E;
  int rows;                 // batch rows B (T = B*S); capacity applies per row
  int capacity;             // <=0: unlimited
  int shared;               // 1: append the shared pseudo-expert E with all T tokens
  int32_t* counts;          // [E+1]
  int32_t* offsets;         // [E+2]
  int32_t* active;          // [E+1]
  int32_t* n_active;        // scalar
  int32_t* pair_slot;       // [T,K]
  int32_t* slot_token;      // [T*K + T] expert-sorted row -> token id
  int32_t* slot_pair;       // [T*K + T] expert-sorted row -> pair id t*K+k (shared rows: -1)
  int slot_cap;             // mask_index: rows the slot_token/slot_pair buffers hold (<= 0: unchecked)
  int32_t* mirror;          // pinned HOST buffer {n_active, counts[E+1], active[E+1]} written by the kernel itself
                            // (counts pre-zeroed by the host; only active experts' counts are guaranteed written)
};
hipError_t launch_dispatch_index(const IndexArgs& a, hipStream_t st);
// the same index over many workgroups (3 launches) for long prefills; chunk_scratch: [ceil(T*K/1024) * E] ints.
// Not for a.capacity > 0 (Switch per-row capacity is a sequential pass).
hipError_t launch_dispatch_index_wide(const IndexArgs& a, int32_t* chunk_scratch, hipStream_t st);
// dispatch index from a dense router_mask[T,E] (element size 1, 4 or 8 bytes, non-zero = routed)
// keep: nullptr, or E bytes (device-visible): columns with keep[e] == 0 are treated as all-false
hipError_t launch_mask_index(const void* mask, int mask_elem_bytes, int T, int E, const IndexArgs& a, hipStream_t st, const uint8_t* keep = nullptr);
// fused route_topk + dispatch_index in one single-workgroup launch (use for T <= 64)
hipError_t launch_route_index(const RouteArgs& r, const IndexArgs& a, hipStream_t st, const EpFuse* pack = nullptr);
// Decode-sized DeepSeek forwards (bf16, T*K <= 64): the shared expert's FFN rides along with the router.
//   gate_shared1: gate logits + stage 1 of the shared expert (s = its stage-1 descriptor: in = x, row_map = nullptr,
//                 out = h_shared [T, R_sh]);
//   route_shared2: top-k + dispatch index (a.shared must be 0) + stage 2 of the shared expert (s: in = h_shared,
//                 out = y_shared [T, R_sh == H]).
hipError_t launch_gate_shared1(const RouteArgs& a, const FfnStage& s, hipStream_t st);
hipError_t launch_route_shared2(const RouteArgs& r, const IndexArgs& a, const FfnStage& s, hipStream_t st, const EpFuse* pack = nullptr);

// Batch-1 decode of the gated families (bf16, T == 1, K <= 8, T*K <= 64, every owned expert resident): FFN stage 1 that
// routes for itself from the gate logits (no top-k/index launch).  r/a as for launch_route_index (a.shared must be 0),
// s1 = the routed stage-1 descriptor, sh2 = the hidden shared expert's stage-2 descriptor or nullptr.
// Profiling: events armed here ride on the NEXT launch made through the KL macro (kdev.h: every FFN-stage launcher — launch_ffn_stage's
// kernels, launch_ffn1_selfroute, launch_ffn2_decode1, launch_moe_front1, launch_moe_layer1_switch) as hipExtLaunchKernel's start / stop events — the kernel's own begin and end on its dispatch packet.  An event
// RECORD in front of and behind a launch puts the command processor's barrier packets inside the interval (2.5-4 us per launch:
// the round-3..5 bench lines sat that far above rocprofv3's durations).  Thread-local; consumed by one launch.
void arm_kernel_timer(hipEvent_t start, hipEvent_t stop);
bool take_kernel_timer(hipEvent_t* start, hipEvent_t* stop);
inline void disarm_kernel_timer() { hipEvent_t a, b; (void)take_kernel_timer(&a, &b); }  // after a launch that may have failed before taking it
hipError_t launch_ffn1_selfroute(const RouteArgs& r, const IndexArgs& a, const FfnStage& s1, const FfnStage* sh2, const SelfRouteForm& f, hipStream_t st);
// The same for decode batches of 2..8 tokens (bf16 / fp16 gated families, T*K <= 64): the meta block routes every token and
// builds the index, every other workgroup routes the tokens for itself; stage 2 is the generic launch_ffn_stage (combine fused).
// max_active = min(E, T*K).  f (here and above, and for launch_moe_front1): the geometry selfroute_form chose.
hipError_t launch_ffn1_selfroute_multi(const RouteArgs& r, const IndexArgs& a, const FfnStage& s1, const FfnStage* sh2, int max_active, const SelfRouteForm& f, hipStream_t st);
// ... and its stage 2 (s2.fuse_combine set, K = s2.comb.K active experts, one token): blob pointers and combine weights
// come from the records the self-routing launch left in s2.dec_w / s2.dec_cw; f: the form decode1_form chose
hipError_t launch_ffn2_decode1(const FfnStage& s2, const Decode1Form& f, hipStream_t st);
// A whole batch-1 decode layer (gated family, hidden shared expert) in ONE launch (layer_fused.hip): gate | shared stage 1 |
// meta | self-routing stage 1 | shared stage 2 | stage 2 + combine as workgroups of one grid; what used to be a kernel boundary
// is a counter that only grows.  ctr: LAYER1_CTRS words, LAYER1_CTR_STRIDE apart (one cache line each), zeroed once; launch =
// 1, 2, ... per counter set (every launch of a set must have the same shapes: the targets are launch * arrivals per launch).
constexpr int LAYER1_CTR_STRIDE = 1024, LAYER1_CTRS = 3 + 8;  // (one 4 KB page per counter: polls of different counters land on different memory channels)
struct LayerSync {
  uint32_t* ctr;
  uint32_t launch;
  int64_t timeout_ticks;  // bound of every wait, wall_clock64 ticks (100 MHz); on expiry *err = 4 and the workgroup goes on
  int32_t* err;
  int32_t* err_host;          // pinned, device-visible copy of the flag (nullptr: none): the host reads it on the forward path
  unsigned long long* trace;  // debugging (MOEINF_LAYER1_TRACE=<file>): [workgroup][4] wall-clock ticks (start, first wait over, second wait over, end); else nullptr
  int sleep;                  // s_sleep(2) repetitions between two polls
  int scalar_poll;            // 1: the counters are polled with scalar loads (they live in uncached memory); 0: agent-scope vector loads
  float* part;                // Switch form: [4][H] fp32 partial sums of the split stage-2 reduction
};
// the FRONT of a batch-1 layer of the gated families in one launch: gate | (shared stage 1) | meta | self-routing stage 1 |
// (shared stage 2); stage 2 + combine stay launch_ffn2_decode1.  sh1 / sh2: the hidden shared expert's stages or nullptr.
hipError_t launch_moe_front1(const RouteArgs& r, const IndexArgs& a, const FfnStage* sh1, const FfnStage* sh2, const FfnStage& s1, const LayerSync& sy, const SelfRouteForm& f, hipStream_t st);
// the Switch form (top-1, plain experts, no shared expert): E + 1 + F/16 + 4 * H/16 workgroups of eight waves, all resident at once;
// false: not handled (layer1_switch_fits says so beforehand: layer_form then plans the three launches)
bool launch_moe_layer1_switch(const RouteArgs& r, const IndexArgs& a, const FfnStage& s1, const FfnStage& s2, const LayerSync& sy, int num_cus, int wgs_per_cu, hipStream_t st);
// workgroups of that kernel one CU holds at a time (hipOccupancyMaxActiveBlocksPerMultiprocessor of the instantiation; 0: unknown)
int layer1_switch_wgs_per_cu(int x_dtype, int gate_dtype);

hipError_t launch_combine(const CombineArgs& a, hipStream_t st, const EpWait* wait = nullptr);  // wait: poll these flags first (peer-store exchange)
// out[i] = valid[i] ? idx[i] : -1
hipError_t launch_masked_idx(const int32_t* idx, const int32_t* valid, int32_t* out, int n, hipStream_t st);
// index arrays for "only the shared pseudo-expert E is active, with T rows" (expert-parallel path)
hipError_t launch_shared_only_index(const IndexArgs& a, hipStream_t st);

// residency-table update: table[idx[i]] = val[i], i < n (n <= 16), stream-ordered
struct PokeArgs {
  uint64_t* table;
  int n;
  int32_t idx[16];
  uint64_t val[16];
};
hipError_t launch_poke(const PokeArgs& a, hipStream_t st);

// expert-parallel helpers
// key[p] = valid pair ? topk_idx[p] % ep_size : -1   (destination rank of every (token,k) pair);
// also resets pair_pos[p] = -1 when pair_pos != nullptr
hipError_t launch_ep_dest_key(const int32_t* topk_idx, const int32_t* pair_valid, int32_t* key, int32_t* pair_pos,
                              int n_pairs, int ep_size, hipStream_t st);
struct EpPackArgs {
  const void* x;              // [T,H]
  void* send;                 // [ep_size*cap_rows, ld_send]: H activations + a 16-byte tail whose first int32 is
                              // the expert id of the row (-1 = padding) -> rows and ids travel in ONE all-to-all
  int64_t ld_send;            // elements per send row (H + 16/sizeof(elem))
  int32_t* pair_pos;          // [T*K] row of every pair inside `send`, -1 if not dispatched
  const int32_t* topk_idx;    // [T*K]
  const int32_t* counts;      // [ep_size] rows per destination (from dispatch_index on the dest keys)
  const int32_t* offsets;     // [ep_size+1]
  const int32_t* slot_pair;   // [T*K] destination-sorted slot -> pair id
  int K, H, ep_size, cap_rows, dtype;
};
hipError_t launch_ep_pack(const EpPackArgs& a, hipStream_t st, const EpPeers* peers = nullptr);
// the pack riding in the single-workgroup router launch of a decode-sized forward (launch_route_index /
// launch_route_shared2): on != 0 makes the workgroup that routed and indexed the tokens write the send rows as well
struct EpFuse {
  EpPackArgs a;
  const int32_t* pair_valid;
  int32_t* send_counts;  // optional [ep_size]
  int on;
  EpPeers peers;         // peers.on: the rows go straight into the destination ranks' windows (a.send unused)
};
// compact, destination-sorted send rows (variable-split exchange): row r = r-th pair in destination order
hipError_t launch_ep_pack_compact(const EpPackArgs& a, int n_pairs, hipStream_t st);
// n_pairs <= 64: dest keys + stable ranks + row copy in one launch (counts/offsets/slot_pair of `a` unused);
// send_counts (optional, [ep_size]) receives the rows per destination
hipError_t launch_ep_pack_small(const EpPackArgs& a, const int32_t* pair_valid, int n_pairs, int32_t* send_counts, hipStream_t st,
                                const EpPeers* peers = nullptr);

// Expert-parallel exchange, owner side, decode-sized (<= 64 received row slots, every owned expert resident): one FFN
// stage that INDEXES FOR ITSELF — every workgroup reads the expert ids in the received rows' tails, derives "its"
// expert (the blockIdx.y-th smallest id present) and that expert's rows, and streams the weights once over them: no
// dispatch-index launch between the all-to-all and the FFN.  stage 1: in = recv rows, out = h (expert-sorted rows);
// stage 2: in = h, out = the reply buffer, every row at its ARRIVAL position (no un-sort pass).
struct EpOwnArgs {
  const void* recv;     // [nrows, ld_recv]: H activations + 16-byte tail (first int32 = expert id, -1 = padding)
  int64_t ld_recv;      // elements
  int H;                // activation elements per received row
  int nrows;            // <= 64
  int ep_size, ep_rank;
  int stage;            // 1 or 2
  int max_active;       // grid.y
  int32_t* mirror;      // stage 1 only (optional): pinned routing mirror {n_active, counts[E+1], active[E+1]}
  // stage 1 leaves, per expert slot u, what stage 2 needs ("decode record", as dec_w / dec_cw of the local batch-1 path): stage 2
  // then starts with one round of loads from ordinary memory instead of re-deriving the index from the row tails
  struct Rec { uint64_t w; int32_t cnt, off, present, pad; int32_t rows[64]; };
  Rec* rec;             // [max_active] (nullptr: both stages index for themselves)
  int32_t* tile_done;   // [ceil(R/16)] zeroed counters: stage 2 of the peer-store exchange arrives per column tile first
  EpPeers peers;        // peers.on: recv = this rank's window; stage 1 polls the recv flags (peers.poll), stage 2 stores
                        // every output row straight into its home rank's window and the last workgroup publishes
};
hipError_t launch_ffn_ep_stage(const FfnStage& s, const EpOwnArgs& o, hipStream_t st);
// ---- batch-1 decode over the peer-store exchange, BROADCAST form (every rank brings ONE token; round 4) -------------------
// The routed form needs a router launch between the gate and the exchange (route_index + pack).  With one token per rank the
// home rank instead BROADCASTS (its token's row, its E gate logits) to every rank, and every owner's FFN stage 1 routes for
// itself — for all ep_size tokens — exactly as the local batch-1 path does for one (ffn1_selfroute, route_set_lean): the same
// logits through the same instructions give the same top-k on every rank, so the owners agree with the home rank's combine
// without a word of routing crossing the fabric.  Launches per layer: gate -> stage 1 (block 0: broadcast + home routing;
// others: poll, route ep_size tokens, stream) -> stage 2 (from stage 1's records, outputs stored home) -> combine.
struct EpBcastArgs {
  const void* x;          // [1, H] this rank's token
  int32_t* pair_pos;      // [K] -> ret row of every pair of the home token (owner * cap_rows + position)
  int32_t* mirror;        // pinned routing mirror of the OWNER side (optional)
  EpPeers peers;
};
// stage 1.  r / a: router arguments of the home token (r.logits = its gate logits, written by the gate launch); s1: routed
// stage-1 descriptor (in = this rank's recv region, ld_in = exchange row elements); sh2: hidden shared expert's stage 2 or
// nullptr; rec: stage-2 records.  with_bcast = 0: block 0's work was done by launch_ep_bcast (fallback paths).
hipError_t launch_ffn_epb_stage1(const RouteArgs& r, const FfnStage& s1, const FfnStage* sh2, const EpBcastArgs& b, EpOwnArgs::Rec* rec,
                                 int max_active, int with_bcast, hipStream_t st);
// the broadcast + the home token's routing as a launch of its own
hipError_t launch_ep_bcast(const RouteArgs& r, const EpBcastArgs& b, hipStream_t st);
// owner side, slow path (an owned expert is not resident: the host must see the routing): wait for the broadcasts, route the
// ep_size tokens and write what the ROUTED form would have delivered — rows with expert-id tails — into a local staging buffer
// `recv_like` [ep_size*cap_rows, ld] so that the generic owner path can take over
hipError_t launch_ep_bcast_unpack(const RouteArgs& r, const EpBcastArgs& b, void* recv_like, int64_t ld, int dtype, hipStream_t st);

// peer-store exchange, owner side, generic path (more rows than the self-indexing kernel takes): copy the valid rows of
// y [ep_size*cap_rows, H] (valid = the received row's tail >= 0) into their home ranks' windows and publish
hipError_t launch_ep_push(const void* y, const void* recv, int64_t ld_recv, int H, int dtype, const EpPeers& peers, hipStream_t st);
// transport self-test: rank r writes a tagged pattern into segment r of every peer's two regions and publishes `peers.epoch`
// on both flag sets; check: after both flag sets arrived, every segment p of this rank's regions must hold rank p's tag
hipError_t launch_ep_selftest_send(const EpPeers& peers, int words, hipStream_t st);
hipError_t launch_ep_selftest_check(const EpPeers& peers, int words, int32_t* ok_dev, hipStream_t st);
// [T,K] routing of a caller that kept its own router -> the engine's pair arrays (moeinf_combine): idx < 0 = dropped pair
hipError_t launch_prep_pairs(const int32_t* idx_in, const float* w_in, int T, int K, int32_t* topk_idx, float* topk_w,
                             int32_t* pair_valid, int32_t* pair_order, hipStream_t st);

}  // namespace moeinf
