// ffn_gemm_mx4_kernels.h — the bodies of the MXFP4-slot forms of ffn_gemm_lds_kernel and ffn_gemm_hyb_kernel (T = mx4w_t; the kernels
// in ffn_gemm_kernels.h branch here at compile time).  Included by ffn_gemm_mx4.hip only.
// A workgroup of a routed expert multiplies MXFP4 code tiles (16 rows x 128 k per KiB, lane l: row l & 15, k 32(l >> 4) .. +31 = one MX
// block; the e8m0 scales behind the matrix's code tiles, byte t & 3 of lane l's dword t >> 2 for tile t — kdev.h) up-cast in registers
// by v_cvt_scalef32_pk_bf16_fp4 against bf16 activations.  The activation image in LDS is the bf16 kernels' full-line one (XL: pieces
// of 8 token rows x 128 B = two k-tiles, 16-byte chunk ch of row r at r * 128 + ((ch ^ r) << 4)); only XL forms are built, K % 128 == 0
// guarantees whole lines.  A workgroup of the shared expert (e == s.E, bf16 weights) takes the bf16 body — a block-uniform branch;
// that body is written out here again (as in ffn_gemm_f8_kernels.h) rather than factored out of ffn_gemm_kernels.h.
//
// LDS banks (ds_read_b128 is served in four groups of sixteen lanes — lanes of quads {0, 1} or {2, 3}, every token row r = n & 7 once per
// quad — and a group is conflict-free when its sixteen 16-byte slots (r & 1) * 8 + (ch ^ r) differ):
//   hybrid: quad q's 32 codes are the whole activation k-tile q of the stage, chunks 4(q & 1) + c of k-tile pair q >> 1.  Read in the
//     order c = 0..3 by every lane, quads 0 and 1 land on the same slots (ch and ch + 4 have the same parity: 2-way conflicts in every
//     group).  So odd quads swap the code dwords 0 <-> 1, 2 <-> 3 once per tile (four v_cndmask) and read chunk 4(q & 1) + (c ^ 1) in
//     step c: opposite parity, sixteen distinct slots, conflict-free.  Quads 2 and 3 read another 16 KiB (pair 1) and another group.
//   LDS-staged: step i of a stage takes chunk 2q + (i ^ (q & 1)) of the stage's line (the fp8 body's chunks 2q, 2q + 1, with odd quads
//     in the other order for the same reason), conflict-free; the codes are ds_read_b64 at 16 * row + 8 * (q & 1) of one 256-byte MX
//     block (32 lanes, 256 contiguous bytes: conflict-free), the scale dwords ds_read_b32 of 16 consecutive dwords (broadcast).
#pragma once
#include "ffn_gemm_kernels.h"

namespace moeinf {

// 8 e2m1 codes (one dword, element 2j in the low nibble of byte j) x 2^(b - 127) -> one bf16x8 MFMA fragment
__device__ __forceinline__ u32x4 mx4x8_to_bf16(const uint32_t w, const uint32_t b) {
  const float sc = __uint_as_float(b << 23);
#define CVT(sel) __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, (sel)))
  return u32x4{CVT(0), CVT(1), CVT(2), CVT(3)};
#undef CVT
}

// LDS-staged.  Static LDS: the bf16 form's 2 x (2 * NMAT * RGB + 2 * NTB) KiB array, which the shared expert's bf16 body needs whole:
// 96 KiB for the largest forms that are built (gated 64-row blocks with 8 waves; plain 128-row blocks with 8 waves), 48 KiB for the
// smallest (plain, 64-row blocks, 4 waves).  The MXFP4 body uses less of it: two activation stages of 2 * NTB KiB
// (two k-tiles each, the bf16 DMA), two code buffers of NMAT * RGB KiB (ONE code tile per matrix and row group = two activation
// stages, refilled by the LDS DMA every second stage) and two scale buffers of NMAT * RGB * 256 B (the scale dwords of those tiles,
// 4-byte LDS DMA from the global address space: one dword holds the scales of four consecutive tiles) — 64 + 16 + 4 = 84 of the 96 KiB in both
// of the largest forms (NMAT * RGB = 8, NTB = 16).
template <int NMAT, int RGB, int NWV, bool XL>
__device__ __forceinline__ void ffn_gemm_lds_kernel_mx4w(const FfnStage& s) {
  static_assert(XL, "MXFP4 forms stage the activations in full lines");
  using A = uint16_t;
  constexpr int EPV = DT<A>::EPV;
  constexpr int EPT = 4 * EPV;
  constexpr int RGW = RGB / 2;
  constexpr int WC = NWV / 2;          // wave columns
  constexpr int NTW = 4, NTB = WC * NTW;
  constexpr int XPW = 2 * NTB / NWV;   // activation DMA pieces per wave and k-tile pair
  constexpr int KK = 2;
  constexpr int A_TILES = KK * NMAT * RGB;
  constexpr int B_TILES = KK * NTB;
  constexpr int STAGE = (A_TILES + B_TILES) * 1024;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  // the MXFP4 body's carving of smem
  constexpr int XB = B_TILES * 1024;             // one activation stage
  constexpr int CB = NMAT * RGB * 1024;          // one code buffer
  constexpr int SB = NMAT * RGB * 256;           // one scale buffer
  constexpr int C_OFF = 2 * XB, S_OFF = C_OFF + 2 * CB;
  static_assert(S_OFF + 2 * SB <= 2 * STAGE, "the MXFP4 buffers fit the bf16 form's LDS");

  const int u = blockIdx.y, bx = blockIdx.x;
  if (u >= (s.n_active_host >= 0 ? s.n_active_host : *s.n_active)) return;
  const int e = s.active[u];
  const bool sh = (e == s.E);
  const int K = sh ? s.K_sh : s.K;
  const int R = sh ? s.R_sh : s.R;
  const int rg0 = bx * RGB;
  const int nrg_total = (R + 15) / 16;
  if (rg0 >= nrg_total) return;
  const int cnt = s.counts[e];
  const int off = s.offsets[e];
  const char* W = reinterpret_cast<const char*>(s.wptr[e]);
  if (W == nullptr) {
    if (threadIdx.x == 0 && bx == 0) atomicExch(s.miss_flag, 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int n = lane & 15, q = lane >> 4;
  const int KB = K / EPT;  // activation k-tiles; K % 64 == 0 (ffn_form)
  const int KS = KB / KK;  // stages
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  auto body = [&](auto wtag) {
  constexpr bool MX = std::is_same<decltype(wtag), mx4w_t>::value;
  const int KBW = MX ? KB / 4 : KB;  // weight tiles per row group (MXFP4: K % 128 == 0)
  const size_t rg_stride = (size_t)KBW * 1024;
  const char* am[NMAT];
  am[0] = W + (sh ? s.off_a_sh : s.off_a) + (size_t)rg0 * rg_stride + lane * 16;
  if (NMAT == 2) am[NMAT - 1] = W + (sh ? s.off_b_sh : s.off_b) + (size_t)rg0 * rg_stride + lane * 16;
  // MXFP4: the scale dwords behind the matrix's code tiles, [tile / 4][lane]
  const char* sm[NMAT];
  sm[0] = W + s.off_a + (size_t)nrg_total * rg_stride + lane * 4;
  if (NMAT == 2) sm[NMAT - 1] = W + s.off_b + (size_t)nrg_total * rg_stride + lane * 4;

  for (int tile0 = 0; tile0 * 16 < cnt; tile0 += NTB) {
    const int ntl = min(NTB, (cnt - tile0 * 16 + 15) / 16);
    // activation rows this wave DMA-loads: the 8-row pieces `wave + NWV*i` (8 rows x 128 B, source chunk swizzled)
    const A* xrp[XPW];
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int trow = tile0 * 16 + (wave + NWV * i) * 8 + (lane >> 3);
      const int srow = off + min(trow, cnt - 1);
      const int64_t xrow = s.row_map ? (int64_t)s.row_map[srow] : (int64_t)srow;
      xrp[i] = reinterpret_cast<const A*>(s.in) + xrow * s.ld_in + (((lane & 7) ^ (lane >> 3)) * EPV);
    }
    f32x4 acc[RGW][NTW][NMAT];
#pragma unroll
    for (int a = 0; a < RGW; ++a)
#pragma unroll
      for (int b = 0; b < NTW; ++b)
#pragma unroll
        for (int m = 0; m < NMAT; ++m) acc[a][b][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the activation image of stage ks: x_off = where it starts in smem
    auto issue_x = [&](int ks, int x_off) {
#pragma unroll
      for (int i = 0; i < XPW; ++i) {
        const int pc = wave + NWV * i;  // 8-row piece; token group pc/2
        if (pc < 2 * ntl)
          __builtin_amdgcn_global_load_lds((gptr_t)(xrp[i] + (size_t)ks * KK * EPT), (lptr_t)(smem + x_off + pc * 1024), 16, 0, 0);
      }
    };

    if constexpr (MX) {
      // code tile kt of every (matrix, row group) of the block and the dwords that hold its scales -> buffer kt & 1
      auto issue_w = [&](int kt) {
        char* cbase = smem + C_OFF + (kt & 1) * CB;
        char* sbase = smem + S_OFF + (kt & 1) * SB;
#pragma unroll
        for (int i = 0; i < (RGB + NWV - 1) / NWV; ++i) {
          const int rg_l = wave + NWV * i;
          if (rg_l < RGB && rg0 + rg_l < nrg_total) {
            const int t = (rg0 + rg_l) * KBW + kt;  // the tile's number in the matrix
#pragma unroll
            for (int m = 0; m < NMAT; ++m) {
              __builtin_amdgcn_global_load_lds((gptr_t)(am[m] + rg_l * rg_stride + (size_t)kt * 1024), (lptr_t)(cbase + (m * RGB + rg_l) * 1024), 16, 0, 0);
              __builtin_amdgcn_global_load_lds((gptr_t)(sm[m] + (size_t)(t >> 2) * 256), (lptr_t)(sbase + (m * RGB + rg_l) * 256), 4, 0, 0);
            }
          }
        }
      };
      issue_x(0, 0);
      issue_w(0);
      for (int ks = 0; ks < KS; ++ks) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of stage ks has landed
        __syncthreads();                                   // ... everybody's has, and stage ks-1 is fully consumed
        if (ks + 1 < KS) {
          issue_x(ks + 1, ((ks + 1) & 1) * XB);
          if (!((ks + 1) & 1)) issue_w((ks + 1) >> 1);  // (its buffer was last read in stages ks-3, ks-2)
        }
        // stage ks = half h of code tile kt: MX blocks 2h, 2h+1.  Quad q takes block 2h + (q >> 1), its dwords 2(q & 1), 2(q & 1) + 1 —
        // k 16q .. 16q+15 of the stage, i.e. chunks 2q, 2q+1 of the token's line — odd quads in the other order (header: banks)
        const int h = ks & 1, kt = ks >> 1, odd = q & 1;
        const char* cp = smem + C_OFF + (kt & 1) * CB + ((2 * h + (q >> 1)) * 16 + n) * 16 + odd * 8;
        const char* sp = smem + S_OFF + (kt & 1) * SB + ((2 * h + (q >> 1)) * 16 + n) * 4;
        const char* xb = smem + (ks & 1) * XB;
        const int r = n & 7;
        u32x4 bf[2][NTW];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int ch = 2 * q + (i ^ odd);
#pragma unroll
          for (int b = 0; b < NTW; ++b)
            bf[i][b] = *reinterpret_cast<const u32x4*>(xb + ((wc * NTW + b) * 2 + (n >> 3)) * 1024 + r * 128 + ((ch ^ r) << 4));
        }
#pragma unroll
        for (int a = 0; a < RGW; ++a) {
          const int rg_l = wr * RGW + a;
          if (rg0 + rg_l < nrg_total) {
            const int sh8 = (((rg0 + rg_l) * KBW + kt) & 3) * 8;  // (wave-uniform)
            uint2 w[NMAT];
            uint32_t sc[NMAT];
#pragma unroll
            for (int m = 0; m < NMAT; ++m) {
              w[m] = *reinterpret_cast<const uint2*>(cp + (m * RGB + rg_l) * 1024);
              sc[m] = (*reinterpret_cast<const uint32_t*>(sp + (m * RGB + rg_l) * 256) >> sh8) & 255u;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              u32x4 af[NMAT];
#pragma unroll
              for (int m = 0; m < NMAT; ++m) af[m] = mx4x8_to_bf16((i ^ odd) ? w[m].y : w[m].x, sc[m]);
#pragma unroll
              for (int b = 0; b < NTW; ++b) {
                if (wc * NTW + b < ntl) {
                  mma16<A>(acc[a][b][0], af[0], bf[i][b]);
                  if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], af[NMAT - 1], bf[i][b]);
                }
              }
            }
          }
        }
      }
    } else {
      // the shared expert: the bf16 form's loop (ffn_gemm_kernels.h), full-line staging
      auto issue = [&](int ks, int buf) {
        char* base = smem + buf * STAGE;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const int kb = ks * KK + kk;
#pragma unroll
          for (int i = 0; i < (RGB + NWV - 1) / NWV; ++i) {
            const int rg_l = wave + NWV * i;
            if (rg_l < RGB && rg0 + rg_l < nrg_total) {
#pragma unroll
              for (int m = 0; m < NMAT; ++m)
                __builtin_amdgcn_global_load_lds((gptr_t)(am[m] + rg_l * rg_stride + (size_t)kb * 1024),
                                                 (lptr_t)(base + ((kk * NMAT + m) * RGB + rg_l) * 1024), 16, 0, 0);
            }
          }
        }
        issue_x(ks, buf * STAGE + A_TILES * 1024);
      };
      issue(0, 0);
      for (int ks = 0; ks < KS; ++ks) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of stage ks has landed
        __syncthreads();                                   // ... everybody's has, and stage ks-1 is fully consumed
        if (ks + 1 < KS) issue(ks + 1, (ks + 1) & 1);
        const char* base = smem + (ks & 1) * STAGE + lane * 16;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          u32x4 af[RGW][NMAT], bf[NTW];
#pragma unroll
          for (int a = 0; a < RGW; ++a) {
            const int rg_l = wr * RGW + a;
#pragma unroll
            for (int m = 0; m < NMAT; ++m) af[a][m] = *reinterpret_cast<const u32x4*>(base + ((kk * NMAT + m) * RGB + rg_l) * 1024);
          }
#pragma unroll
          for (int b = 0; b < NTW; ++b) {
            const int r = n & 7, ch = kk * 4 + q;
            bf[b] = *reinterpret_cast<const u32x4*>(smem + (ks & 1) * STAGE + (A_TILES + (wc * NTW + b) * 2 + (n >> 3)) * 1024 + r * 128 + ((ch ^ r) << 4));
          }
#pragma unroll
          for (int a = 0; a < RGW; ++a) {
            if (rg0 + wr * RGW + a < nrg_total) {
#pragma unroll
              for (int b = 0; b < NTW; ++b) {
                if (wc * NTW + b < ntl) {
                  mma16<A>(acc[a][b][0], af[a][0], bf[b]);
                  if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], af[a][NMAT - 1], bf[b]);
                }
              }
            }
          }
        }
      }
    }
    // epilogue straight from the accumulators (no K split): lane holds 4 consecutive rows of one token
    epi_switch<NMAT>(s.epi, [&](auto epic) {
      constexpr int EPI = decltype(epic)::value;
      const A* bias = reinterpret_cast<const A*>(W + s.off_bias);
      const bool aligned = (s.ld_out & 3) == 0;
#pragma unroll
      for (int b = 0; b < NTW; ++b) {
        const int tok = (tile0 + wc * NTW + b) * 16 + n;
        if (tok < cnt) {
          A* orow_p = reinterpret_cast<A*>(s.out) + (size_t)(s.out_map ? s.out_map[off + tok] : off + tok) * s.ld_out;
#pragma unroll
          for (int a = 0; a < RGW; ++a)
            if (rg0 + wr * RGW + a < nrg_total)
              epi_quad<A, EPI>(acc[a][b][0], acc[a][b][NMAT - 1], bias, (rg0 + wr * RGW + a) * 16 + q * 4, R, aligned, orow_p);
        }
      }
    });
    __syncthreads();  // the next pass re-uses the buffers of stage 0
  }
  };
  if (sh) body(A{});  // block-uniform
  else body(mx4w_t{});
}

// Hybrid.  A stage is KK = 4 activation k-tiles (two full-line pairs, the bf16 DMA) = ONE code tile per row group and matrix in
// registers, with the dword that holds its scale (a 4-byte load through the global address space, in the same register ring; a
// stage is one tile, so four consecutive stages read the same dword again from the cache).  K % 128 == 0: no short last stage.
// Static LDS: 2 x 32 KiB, the bf16 form's.
template <int NMAT, int RW, int KK, bool XL>
__device__ __forceinline__ void ffn_gemm_hyb_kernel_mx4w(const FfnStage& s) {
  static_assert(XL && KK == 4, "an MXFP4 code tile is four activation k-tiles, staged in full lines");
  using A = uint16_t;
  constexpr int EPV = DT<A>::EPV;
  constexpr int EPT = 4 * EPV;
  constexpr int NTB = 8;
  constexpr int RGB = 4 * RW;            // row groups per block
  constexpr int STAGE = KK * NTB * 1024;  // activation bytes per stage
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int u = blockIdx.y;
  if (u >= (s.n_active_host >= 0 ? s.n_active_host : *s.n_active)) return;
  const int e = s.active[u];
  const bool sh = (e == s.E);
  const int K = sh ? s.K_sh : s.K;
  const int R = sh ? s.R_sh : s.R;
  const int nrg_total = (R + 15) / 16;
  if ((int)blockIdx.x * RGB >= nrg_total) return;
  const int cnt = s.counts[e];
  const int off = s.offsets[e];
  const char* W = reinterpret_cast<const char*>(s.wptr[e]);
  if (W == nullptr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicExch(s.miss_flag, 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, q = lane >> 4;
  const int KB = K / EPT;  // activation k-tiles; K % 64 == 0 (ffn_form)
  const int KS = (KB + KK - 1) / KK;
  const int rgw0 = blockIdx.x * RGB + wave * RW;  // first row group of this wave
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  auto body = [&](auto wtag) {
  constexpr bool MX = std::is_same<decltype(wtag), mx4w_t>::value;
  constexpr int KKW = MX ? 1 : KK;     // weight tiles per stage
  const int KBW = MX ? KB / 4 : KB;    // weight tiles per row group
  const size_t rg_stride = (size_t)KBW * 1024;
  // row groups past the end (R not a multiple of the block's rows) re-read the last one; their results are dropped
  const char* ap[RW][NMAT];
  const char* sp[RW][NMAT];  // MXFP4: lane's scale dwords, [tile / 4][lane] behind the matrix's code tiles
  int t0[RW];                // ... and the number of the row group's first tile in the matrix
#pragma unroll
  for (int a = 0; a < RW; ++a) {
    const int rg = min(rgw0 + a, nrg_total - 1);
    ap[a][0] = W + (sh ? s.off_a_sh : s.off_a) + (size_t)rg * rg_stride + lane * 16;
    if (NMAT == 2) ap[a][NMAT - 1] = W + (sh ? s.off_b_sh : s.off_b) + (size_t)rg * rg_stride + lane * 16;
    sp[a][0] = W + s.off_a + (size_t)nrg_total * rg_stride + lane * 4;
    if (NMAT == 2) sp[a][NMAT - 1] = W + s.off_b + (size_t)nrg_total * rg_stride + lane * 4;
    t0[a] = rg * KBW;
  }

  for (int tile0 = 0; tile0 * 16 < cnt; tile0 += NTB) {
    const int ntl = min(NTB, (cnt - tile0 * 16 + 15) / 16);
    constexpr int XPW = 4;
    const A* xrp[XPW];  // activation rows this wave DMA-loads: the 8-row pieces `wave + 4i`
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int trow = tile0 * 16 + (wave + 4 * i) * 8 + (lane >> 3);
      const int srow = off + min(trow, cnt - 1);
      const int64_t xrow = s.row_map ? (int64_t)s.row_map[srow] : (int64_t)srow;
      xrp[i] = reinterpret_cast<const A*>(s.in) + xrow * s.ld_in + (((lane & 7) ^ (lane >> 3)) * EPV);
    }
    f32x4 acc[RW][NTB][NMAT];
#pragma unroll
    for (int a = 0; a < RW; ++a)
#pragma unroll
      for (int b = 0; b < NTB; ++b)
#pragma unroll
        for (int m = 0; m < NMAT; ++m) acc[a][b][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 af[2][KKW][RW][NMAT];  // two register sets of weight fragments / code tiles (current / next stage)
    uint32_t sf[2][RW][NMAT];    // MXFP4: the scale dwords of those tiles
    auto issue = [&](int ks, int buf, u32x4 (&dst)[KKW][RW][NMAT], uint32_t (&sdst)[RW][NMAT]) {
      char* base = smem + buf * STAGE;
      if constexpr (MX) {
#pragma unroll
        for (int a = 0; a < RW; ++a)
#pragma unroll
          for (int m = 0; m < NMAT; ++m) {
            dst[0][a][m] = ld16_nt_global(ap[a][m] + (size_t)ks * 1024);
            sdst[a][m] = ld4_global(sp[a][m] + (size_t)((t0[a] + ks) >> 2) * 256);
          }
      } else {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const int kb = min(ks * KK + kk, KB - 1);  // a short last stage re-reads tile KB-1 (never multiplied)
#pragma unroll
          for (int a = 0; a < RW; ++a)
#pragma unroll
            for (int m = 0; m < NMAT; ++m) dst[kk][a][m] = ld16_nt(ap[a][m] + (size_t)kb * 1024);
        }
      }
#pragma unroll
      for (int j = 0; j < KK / 2; ++j) {
        const int pr = min(ks * (KK / 2) + j, KB / 2 - 1);  // k-tile pair (a short last stage re-reads the last pair)
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
          const int pc = wave + 4 * i;
          if (pc < 2 * ntl)
            __builtin_amdgcn_global_load_lds((gptr_t)(xrp[i] + (size_t)pr * 2 * EPT), (lptr_t)(base + (j * 2 * NTB + pc) * 1024), 16, 0, 0);
        }
      }
    };
    auto compute = [&](int ks, int buf, const u32x4 (&cur)[KKW][RW][NMAT], const uint32_t (&scur)[RW][NMAT]) {
      const int r = n & 7;
      if constexpr (MX) {
        // quad q's 32 codes are activation k-tile q of the stage: chunks 4(q & 1) + c of pair q >> 1; odd quads take c in the order
        // 1, 0, 3, 2 (code dwords swapped here, header: banks)
        const int odd = q & 1;
        u32x4 fa[RW][NMAT][4];
#pragma unroll
        for (int a = 0; a < RW; ++a) {
          const int sh8 = ((t0[a] + ks) & 3) * 8;  // (wave-uniform)
#pragma unroll
          for (int m = 0; m < NMAT; ++m) {
            const u32x4 w = cur[0][a][m];
            const u32x4 ws = {odd ? w[1] : w[0], odd ? w[0] : w[1], odd ? w[3] : w[2], odd ? w[2] : w[3]};
            mx4x32_to_bf16(ws, (scur[a][m] >> sh8) & 255u, fa[a][m]);
          }
        }
#pragma unroll
        for (int b = 0; b < NTB; ++b) {
          if (b < ntl) {
            const char* xp = smem + buf * STAGE + ((q >> 1) * 2 * NTB + b * 2 + (n >> 3)) * 1024 + r * 128;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int ch = odd * 4 + (c ^ odd);
              const u32x4 bf = *reinterpret_cast<const u32x4*>(xp + ((ch ^ r) << 4));
#pragma unroll
              for (int a = 0; a < RW; ++a) {
                mma16<A>(acc[a][b][0], fa[a][0][c], bf);
                if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], fa[a][NMAT - 1][c], bf);
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          if (ks * KK + kk < KB) {
#pragma unroll
            for (int b = 0; b < NTB; ++b) {
              if (b < ntl) {
                const int ch = (kk & 1) * 4 + q;
                const u32x4 bf = *reinterpret_cast<const u32x4*>(smem + buf * STAGE + ((kk >> 1) * 2 * NTB + b * 2 + (n >> 3)) * 1024 + r * 128 + ((ch ^ r) << 4));
#pragma unroll
                for (int a = 0; a < RW; ++a) {
                  mma16<A>(acc[a][b][0], cur[kk][a][0], bf);
                  if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], cur[kk][a][NMAT - 1], bf);
                }
              }
            }
          }
        }
      }
    };

    issue(0, 0, af[0], sf[0]);
    for (int ks = 0; ks < KS; ks += 2) {  // unrolled by two so both register sets are indexed statically (KS may be odd: K = 1408)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage ks: this wave's fragments and activation DMA landed
      __syncthreads();                                   // ... everybody's DMA has, and stage ks-1 is fully consumed
      if (ks + 1 < KS) issue(ks + 1, 1, af[1], sf[1]);
      compute(ks, 0, af[0], sf[0]);
      if (ks + 1 < KS) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (ks + 2 < KS) issue(ks + 2, 0, af[0], sf[0]);
        compute(ks + 1, 1, af[1], sf[1]);
      }
    }
    // epilogue straight from the accumulators (no K split): lane holds 4 consecutive rows of one token
    epi_switch<NMAT>(s.epi, [&](auto epic) {
      constexpr int EPI = decltype(epic)::value;
      const A* bias = reinterpret_cast<const A*>(W + s.off_bias);
      const bool aligned = (s.ld_out & 3) == 0;
#pragma unroll
      for (int b = 0; b < NTB; ++b) {
        const int tok = (tile0 + b) * 16 + n;
        if (tok < cnt) {
          A* orow_p = reinterpret_cast<A*>(s.out) + (size_t)(s.out_map ? s.out_map[off + tok] : off + tok) * s.ld_out;
#pragma unroll
          for (int a = 0; a < RW; ++a)
            if (rgw0 + a < nrg_total)
              epi_quad<A, EPI>(acc[a][b][0], acc[a][b][NMAT - 1], bias, (rgw0 + a) * 16 + q * 4, R, aligned, orow_p);
        }
      }
    });
    __syncthreads();  // the next pass re-uses LDS buffer 0
  }
  };
  if (sh) body(A{});  // block-uniform
  else body(mx4w_t{});
}

}  // namespace moeinf
