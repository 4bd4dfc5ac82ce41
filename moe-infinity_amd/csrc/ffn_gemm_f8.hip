// ffn_gemm_f8.hip — fp8-slot forms (T = f8w_t: bf16 activations, the routed experts' weights fp8 tiles up-cast in registers) of
// the grouped-GEMM kernels for experts with many rows: the hybrid, the LDS-staged and the register-ring kernel (ffn_gemm_f8_kernels.h,
// ffn_ring2_kernel.h).  Which one a stage takes: f8_gemm_form (kernels.h).  Called by launch_ffn_f8w (kernels.hip); false: not
// handled (the row kernel runs the stage).  Its own translation unit, so the bf16 and fp16 units do not grow.
#include "ffn_gemm_f8_kernels.h"
#include "ffn_ring2_kernel.h"

namespace moeinf {

template <int NMAT>
static void launch_f8(const FfnStage& s, dim3 grid, const F8GemmForm& f, hipStream_t st) {
  static const int kk = env_int("MOEINF_GEMM_HYB_KK", 4);
  static const int xl_env = env_int("MOEINF_GEMM_XL", 1);
  const bool xl = xl_env && (s.K_sh % 64) == 0;  // (s.K % 64 == 0: every fp8 slot)
  if (f.kernel == F8G_RING2) {
    launch_ring2<f8w_t, NMAT>(s, grid, f.ring, st);
  } else if (f.kernel == F8G_HYB) {
#define HYB(RWV, KKV, XLV) KL((ffn_gemm_hyb_kernel<f8w_t, NMAT, RWV, KKV, XLV>), dim3((grid.x + 4 * RWV - 1) / (4 * RWV), grid.y), dim3(256), 0, st, s)
    constexpr int RW = NMAT == 2 ? 1 : 2;
    if (kk == 2) { if (xl) HYB(RW, 2, true); else HYB(RW, 2, false); }
    else { if (xl) HYB(RW, 4, true); else HYB(RW, 4, false); }
#undef HYB
  } else {
    static const int rgb_plain = env_int("MOEINF_FFN_GEMM_RGB", 0);
    static const int rgb_gated = env_int("MOEINF_FFN_GEMM_RGB2", 4);
    const bool wide = f.width == 8;
    auto go = [&](auto kern, int rgb, int nwv) { KL(kern, dim3((grid.x + rgb - 1) / rgb, grid.y), dim3(nwv * 64), 0, st, s); };
#define GO(RG, NW) do { if (xl) go(ffn_gemm_lds_kernel<f8w_t, NMAT, RG, NW, true>, RG, NW); else go(ffn_gemm_lds_kernel<f8w_t, NMAT, RG, NW, false>, RG, NW); } while (0)
    // (as bf16: 128-row blocks for the plain stage only when there are >= 2 blocks per CU to hide the DMA latency)
    const bool big = NMAT == 2 ? rgb_gated == 8 : (rgb_plain ? rgb_plain == 8 : (((grid.x + 7) / 8) * grid.y >= 512 && s.K >= 4096));
    if (big) { if (wide) GO(8, 8); else GO(8, 4); }
    else     { if (wide) GO(4, 8); else GO(4, 4); }
#undef GO
  }
}

bool launch_ffn_gemm_f8(const FfnStage& s, int nmat, dim3 grid, int max_rows, hipStream_t st) {
  if ((nmat == 2) != (s.epi == EPI_GATED_SILU)) return false;
  static const F8GemmKnobs knobs0;
  F8GemmKnobs knobs = knobs0;
  // ring2 keeps element offsets into the activations in 32 bits (xoff): a stage whose rows do not fit takes the other kernels
  if (s.rows_bound > 0 && s.rows_bound * s.ld_in >= (int64_t(1) << 32)) knobs.ring.enable_bits = 0;
  const int K_sh = (s.R_sh > 0 && s.K_sh > 0) ? s.K_sh : 0;  // a shared expert rides in this launch
  const F8GemmForm f = f8_gemm_form(nmat, s.K, K_sh, (int)grid.x, (int)grid.y, max_rows, ring2_num_cus(), knobs);
  if (f.kernel == F8G_ROWS) return false;
  if (nmat == 2) launch_f8<2>(s, grid, f, st);
  else launch_f8<1>(s, grid, f, st);
  return true;
}

}  // namespace moeinf
