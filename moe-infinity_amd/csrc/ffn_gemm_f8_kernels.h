// ffn_gemm_f8_kernels.h — the bodies of the fp8-slot forms of ffn_gemm_lds_kernel and ffn_gemm_hyb_kernel (T = f8w_t; the kernels
// in ffn_gemm_kernels.h branch here at compile time).  Included by ffn_gemm_f8.hip only.
// A workgroup of a routed expert multiplies fp8 tiles (16 rows x 64 k per KiB, lane l: row l & 15, k 16(l >> 4) .. +15) up-cast in
// registers by f8x16_to_bf16 against bf16 activations; the activation DMA into LDS is the bf16 kernels' own, only the per-lane
// fragment read differs (the lane's 16 weights meet x[n][16q .. +7] and x[n][16q+8 .. +15]).  A workgroup of the shared expert
// (e == s.E, bf16 weights) takes the bf16 body — a block-uniform branch.  The bf16 body is written out here again rather than shared
// with the kernels in ffn_gemm_kernels.h: factoring it out of them changed the gfx950 code of their bf16 / fp16 / fp32 forms.
#pragma once
#include "ffn_gemm_kernels.h"

namespace moeinf {

template <int NMAT, int RGB, int NWV, bool XL>
__device__ __forceinline__ void ffn_gemm_lds_kernel_f8w(const FfnStage& s) {
  using T = f8w_t;
  // T = f8w_t (fp8 slots, ffn_gemm_f8.hip): bf16 activations (A); a stage's two activation k-tiles are ONE fp8 weight tile per row
  // group and matrix (64 k per KiB: half the weight DMA, the activation DMA unchanged); the shared expert takes the bf16 body
  using A = typename act_of<T>::type;
  constexpr int EPV = DT<A>::EPV;
  constexpr int EPT = 4 * EPV;
  constexpr int RGW = RGB / 2;
  constexpr int WC = NWV / 2;          // wave columns
  constexpr int NTW = 4, NTB = WC * NTW;
  constexpr int XPW = XL ? 2 * NTB / NWV : NTB / NWV;  // activation DMA pieces per wave and k-tile pair
  constexpr int KK = 2;
  constexpr int A_TILES = KK * NMAT * RGB;
  constexpr int B_TILES = KK * NTB;
  constexpr int STAGE = (A_TILES + B_TILES) * 1024;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

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
  const int KB = K / EPT;  // K % EPT == 0 (checked by the launcher)
  const int KS = (KB + KK - 1) / KK;
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  auto body = [&](auto wtag) {
  constexpr bool F8 = std::is_same<decltype(wtag), f8w_t>::value;
  const size_t rg_stride = (size_t)(F8 ? KB / 2 : KB) * 1024;
  const char* am[NMAT];
  am[0] = W + (sh ? s.off_a_sh : s.off_a) + (size_t)rg0 * rg_stride + lane * 16;
  if (NMAT == 2) am[NMAT - 1] = W + (sh ? s.off_b_sh : s.off_b) + (size_t)rg0 * rg_stride + lane * 16;

  for (int tile0 = 0; tile0 * 16 < cnt; tile0 += NTB) {
    const int ntl = min(NTB, (cnt - tile0 * 16 + 15) / 16);
    // activation rows this wave DMA-loads: token groups `wave`, `wave + NWV` (16 rows x 64 B each), or with XL the
    // 8-row pieces `wave + NWV*i` (8 rows x 128 B, source chunk swizzled)
    const A* xrp[XPW];
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int trow = XL ? (tile0 * 16 + (wave + NWV * i) * 8 + (lane >> 3)) : ((tile0 + wave + NWV * i) * 16 + n);
      const int srow = off + min(trow, cnt - 1);
      const int64_t xrow = s.row_map ? (int64_t)s.row_map[srow] : (int64_t)srow;
      xrp[i] = reinterpret_cast<const A*>(s.in) + xrow * s.ld_in + (XL ? (((lane & 7) ^ (lane >> 3)) * EPV) : q * EPV);
    }
    f32x4 acc[RGW][NTW][NMAT];
#pragma unroll
    for (int a = 0; a < RGW; ++a)
#pragma unroll
      for (int b = 0; b < NTW; ++b)
#pragma unroll
        for (int m = 0; m < NMAT; ++m) acc[a][b][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto issue = [&](int ks, int buf) {
      char* base = smem + buf * STAGE;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int kb = ks * KK + kk;
        if (kb < KB) {
          if (!F8 || kk == 0) {  // (fp8: tile ks holds both k-tiles of the stage)
#pragma unroll
          for (int i = 0; i < (RGB + NWV - 1) / NWV; ++i) {
            const int rg_l = wave + NWV * i;
            if (rg_l < RGB && rg0 + rg_l < nrg_total) {
#pragma unroll
              for (int m = 0; m < NMAT; ++m)
                __builtin_amdgcn_global_load_lds((gptr_t)(am[m] + rg_l * rg_stride + (size_t)(F8 ? ks : kb) * 1024),
                                                 (lptr_t)(base + ((kk * NMAT + m) * RGB + rg_l) * 1024), 16, 0, 0);
            }
          }
          }
          if constexpr (!XL) {
#pragma unroll
            for (int i = 0; i < XPW; ++i) {
              const int tg_l = wave + NWV * i;
              if (tg_l < ntl)
                __builtin_amdgcn_global_load_lds((gptr_t)(xrp[i] + (size_t)kb * EPT),
                                                 (lptr_t)(base + (A_TILES + kk * NTB + tg_l) * 1024), 16, 0, 0);
            }
          }
        }
      }
      if constexpr (XL) {
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
          const int pc = wave + NWV * i;  // 8-row piece; token group pc/2
          if (pc < 2 * ntl)
            __builtin_amdgcn_global_load_lds((gptr_t)(xrp[i] + (size_t)ks * KK * EPT), (lptr_t)(base + (A_TILES + pc) * 1024), 16, 0, 0);
        }
      }
    };

    issue(0, 0);
    for (int ks = 0; ks < KS; ++ks) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of stage ks has landed
      __syncthreads();                                   // ... everybody's has, and stage ks-1 is fully consumed
      if (ks + 1 < KS) issue(ks + 1, (ks + 1) & 1);
      const char* base = smem + (ks & 1) * STAGE + lane * 16;
      if constexpr (F8) {
        // the lane's 16 fp8 weights are k 16q .. 16q+15 of the stage: activation fragments x[n][16q .. +7], x[n][16q+8 .. +15] =
        // chunks 2q, 2q+1 of the token's 128-byte line (XL), or slots (n, 2(q&1)), (n, 2(q&1)+1) of k-tile q/2
        u32x4 alo[RGW][NMAT], ahi[RGW][NMAT], blo[NTW], bhi[NTW];
#pragma unroll
        for (int a = 0; a < RGW; ++a) {
          const int rg_l = wr * RGW + a;
#pragma unroll
          for (int m = 0; m < NMAT; ++m) f8x16_to_bf16(*reinterpret_cast<const u32x4*>(base + (m * RGB + rg_l) * 1024), alo[a][m], ahi[a][m]);
        }
#pragma unroll
        for (int b = 0; b < NTW; ++b) {
          if constexpr (XL) {
            const int r = n & 7;
            const char* xp = smem + (ks & 1) * STAGE + (A_TILES + (wc * NTW + b) * 2 + (n >> 3)) * 1024 + r * 128;
            blo[b] = *reinterpret_cast<const u32x4*>(xp + (((2 * q) ^ r) << 4));
            bhi[b] = *reinterpret_cast<const u32x4*>(xp + (((2 * q + 1) ^ r) << 4));
          } else {
            const char* xp = smem + (ks & 1) * STAGE + (A_TILES + (q >> 1) * NTB + wc * NTW + b) * 1024 + ((q & 1) * 32 + n) * 16;
            blo[b] = *reinterpret_cast<const u32x4*>(xp);
            bhi[b] = *reinterpret_cast<const u32x4*>(xp + 256);
          }
        }
#pragma unroll
        for (int a = 0; a < RGW; ++a) {
          if (rg0 + wr * RGW + a < nrg_total) {
#pragma unroll
            for (int b = 0; b < NTW; ++b) {
              if (wc * NTW + b < ntl) {
                mma16<A>(acc[a][b][0], alo[a][0], blo[b]);
                if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], alo[a][NMAT - 1], blo[b]);
                mma16<A>(acc[a][b][0], ahi[a][0], bhi[b]);
                if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], ahi[a][NMAT - 1], bhi[b]);
              }
            }
          }
        }
      } else {
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        if (ks * KK + kk < KB) {
          u32x4 af[RGW][NMAT], bf[NTW];
#pragma unroll
          for (int a = 0; a < RGW; ++a) {
            const int rg_l = wr * RGW + a;
#pragma unroll
            for (int m = 0; m < NMAT; ++m) af[a][m] = *reinterpret_cast<const u32x4*>(base + ((kk * NMAT + m) * RGB + rg_l) * 1024);
          }
#pragma unroll
          for (int b = 0; b < NTW; ++b) {
            if constexpr (XL) {
              const int r = n & 7, ch = kk * 4 + q;
              bf[b] = *reinterpret_cast<const u32x4*>(smem + (ks & 1) * STAGE + (A_TILES + (wc * NTW + b) * 2 + (n >> 3)) * 1024 + r * 128 + ((ch ^ r) << 4));
            } else {
              bf[b] = *reinterpret_cast<const u32x4*>(base + (A_TILES + kk * NTB + wc * NTW + b) * 1024);
            }
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
    __syncthreads();  // the next pass re-uses buffer 0
  }
  };
  if constexpr (std::is_same<T, f8w_t>::value) {
    if (sh) body(A{});  // block-uniform
    else body(T{});
  } else {
    body(T{});
  }
}

template <int NMAT, int RW, int KK, bool XL>
__device__ __forceinline__ void ffn_gemm_hyb_kernel_f8w(const FfnStage& s) {
  using T = f8w_t;
  static_assert(!XL || KK % 2 == 0, "full-line staging moves k-tiles in pairs");
  // T = f8w_t (fp8 slots, ffn_gemm_f8.hip): bf16 activations (A), the routed experts' weights fp8 tiles (64 k per KiB) — a stage
  // still spans KK activation k-tiles (the same DMA), i.e. KK / 2 weight tiles; the shared expert (e == s.E) takes the bf16 body
  using A = typename act_of<T>::type;
  static_assert(!std::is_same<T, f8w_t>::value || KK % 2 == 0, "a 64-k fp8 tile spans two activation k-tiles");
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
  const int KB = K / EPT;  // K % EPT == 0 (checked by the launcher)
  const int KS = (KB + KK - 1) / KK;
  const int rgw0 = blockIdx.x * RGB + wave * RW;  // first row group of this wave
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  auto body = [&](auto wtag) {
  constexpr bool F8 = std::is_same<decltype(wtag), f8w_t>::value;
  constexpr int KKW = F8 ? KK / 2 : KK;  // weight tiles per stage
  const int KBW = F8 ? KB / 2 : KB;      // weight tiles per row group
  const size_t rg_stride = (size_t)KBW * 1024;
  // row groups past the end (R not a multiple of the block's rows) re-read the last one; their results are dropped
  const char* ap[RW][NMAT];
#pragma unroll
  for (int a = 0; a < RW; ++a) {
    const int rg = min(rgw0 + a, nrg_total - 1);
    ap[a][0] = W + (sh ? s.off_a_sh : s.off_a) + (size_t)rg * rg_stride + lane * 16;
    if (NMAT == 2) ap[a][NMAT - 1] = W + (sh ? s.off_b_sh : s.off_b) + (size_t)rg * rg_stride + lane * 16;
  }

  for (int tile0 = 0; tile0 * 16 < cnt; tile0 += NTB) {
    const int ntl = min(NTB, (cnt - tile0 * 16 + 15) / 16);
    constexpr int XPW = XL ? 4 : 2;
    const A* xrp[XPW];  // activation rows this wave DMA-loads: token groups `wave`, `wave + 4` / 8-row pieces `wave + 4i`
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int trow = XL ? (tile0 * 16 + (wave + 4 * i) * 8 + (lane >> 3)) : ((tile0 + wave + 4 * i) * 16 + n);
      const int srow = off + min(trow, cnt - 1);
      const int64_t xrow = s.row_map ? (int64_t)s.row_map[srow] : (int64_t)srow;
      xrp[i] = reinterpret_cast<const A*>(s.in) + xrow * s.ld_in + (XL ? (((lane & 7) ^ (lane >> 3)) * EPV) : q * EPV);
    }
    f32x4 acc[RW][NTB][NMAT];
#pragma unroll
    for (int a = 0; a < RW; ++a)
#pragma unroll
      for (int b = 0; b < NTB; ++b)
#pragma unroll
        for (int m = 0; m < NMAT; ++m) acc[a][b][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 af[2][KKW][RW][NMAT];  // two register sets of weight fragments (current / next stage)
    auto issue = [&](int ks, int buf, u32x4 (&dst)[KKW][RW][NMAT]) {
      char* base = smem + buf * STAGE;
      if constexpr (F8) {
#pragma unroll
        for (int jj = 0; jj < KKW; ++jj) {
          const int kbw = min(ks * KKW + jj, KBW - 1);  // a short last stage re-reads tile KBW-1 (never multiplied)
#pragma unroll
          for (int a = 0; a < RW; ++a)
#pragma unroll
            for (int m = 0; m < NMAT; ++m) dst[jj][a][m] = ld16_nt_global(ap[a][m] + (size_t)kbw * 1024);
        }
      }
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int kb = min(ks * KK + kk, KB - 1);  // a short last stage re-reads tile KB-1 (never multiplied)
        if constexpr (!F8) {
#pragma unroll
          for (int a = 0; a < RW; ++a)
#pragma unroll
            for (int m = 0; m < NMAT; ++m) dst[kk][a][m] = ld16_nt(ap[a][m] + (size_t)kb * 1024);
        }
        if constexpr (!XL) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int tg_l = wave + 4 * i;
            if (tg_l < ntl)
              __builtin_amdgcn_global_load_lds((gptr_t)(xrp[i] + (size_t)kb * EPT), (lptr_t)(base + (kk * NTB + tg_l) * 1024), 16, 0, 0);
          }
        }
      }
      if constexpr (XL) {
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
      }
    };
    auto compute = [&](int ks, int buf, const u32x4 (&cur)[KKW][RW][NMAT]) {
      const char* base = smem + buf * STAGE + lane * 16;
      if constexpr (F8) {
        // fp8 tile jj = activation k-tiles 2jj, 2jj+1: the lane's 16 weights are k 16q .. 16q+15 of the tile, so its two activation
        // fragments are x[n][16q .. +7] and x[n][16q+8 .. +15] — chunks 2q, 2q+1 of the 128-byte line (XL), or slots
        // (n, 2(q&1)) and (n, 2(q&1)+1) of k-tile 2jj + q/2
        const int r = n & 7;
#pragma unroll
        for (int jj = 0; jj < KKW; ++jj) {
          if (ks * KKW + jj < KBW) {
            u32x4 wlo[RW][NMAT], whi[RW][NMAT];
#pragma unroll
            for (int a = 0; a < RW; ++a)
#pragma unroll
              for (int m = 0; m < NMAT; ++m) f8x16_to_bf16(cur[jj][a][m], wlo[a][m], whi[a][m]);
#pragma unroll
            for (int b = 0; b < NTB; ++b) {
              if (b < ntl) {
                const char* xp = XL ? smem + buf * STAGE + (jj * 2 * NTB + b * 2 + (n >> 3)) * 1024 + r * 128
                                    : smem + buf * STAGE + ((2 * jj + (q >> 1)) * NTB + b) * 1024 + ((q & 1) * 32 + n) * 16;
                const u32x4 blo = *reinterpret_cast<const u32x4*>(XL ? xp + (((2 * q) ^ r) << 4) : xp);
                const u32x4 bhi = *reinterpret_cast<const u32x4*>(XL ? xp + (((2 * q + 1) ^ r) << 4) : xp + 256);
#pragma unroll
                for (int a = 0; a < RW; ++a) {
                  mma16<A>(acc[a][b][0], wlo[a][0], blo);
                  if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], wlo[a][NMAT - 1], blo);
                  mma16<A>(acc[a][b][0], whi[a][0], bhi);
                  if (NMAT == 2) mma16<A>(acc[a][b][NMAT - 1], whi[a][NMAT - 1], bhi);
                }
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
              const int r = n & 7, ch = (kk & 1) * 4 + q;
              const u32x4 bf = XL ? *reinterpret_cast<const u32x4*>(smem + buf * STAGE + ((kk >> 1) * 2 * NTB + b * 2 + (n >> 3)) * 1024 + r * 128 + ((ch ^ r) << 4))
                                  : *reinterpret_cast<const u32x4*>(base + (kk * NTB + b) * 1024);
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

    issue(0, 0, af[0]);
    for (int ks = 0; ks < KS; ks += 2) {  // unrolled by two so both register sets are indexed statically
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage ks: this wave's fragments and activation DMA landed
      __syncthreads();                                   // ... everybody's DMA has, and stage ks-1 is fully consumed
      if (ks + 1 < KS) issue(ks + 1, 1, af[1]);
      compute(ks, 0, af[0]);
      if (ks + 1 < KS) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (ks + 2 < KS) issue(ks + 2, 0, af[0]);
        compute(ks + 1, 1, af[1]);
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
  if constexpr (std::is_same<T, f8w_t>::value) {
    if (sh) body(A{});  // block-uniform
    else body(T{});
  } else {
    body(T{});
  }
}

}  // namespace moeinf
