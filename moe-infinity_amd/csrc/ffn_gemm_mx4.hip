// ffn_gemm_mx4.hip — MXFP4-slot forms (T = mx4w_t: bf16 activations, the routed experts' weights MXFP4 code tiles + e8m0 scales up-cast
// in registers) of the grouped-GEMM kernels for experts with many rows: the hybrid and the LDS-staged kernel (ffn_gemm_mx4_kernels.h).
// Which one a stage takes: ffn_form (kernels.h), for an engine with moeinf_set_mxfp4_gemm on.  Called by launch_ffn_stage (kernels.hip).
// Its own translation unit, like ffn_gemm_f8.hip.  Eight kernels, all with full-line activation staging: the hybrid (gated RW 1, plain
// RW 2; KK 4) and the LDS-staged kernel with 4 / 8 waves — gated 4 row groups per workgroup, plain 4 or 8.  (The gated 128-row LDS forms
// are not built: with the MXFP4 and the shared expert's bf16 body in one kernel the compiler reserves a 20-byte private segment for
// them.  ffn_form never asks for them; bf16 and fp8 reach theirs through the sweep knob MOEINF_FFN_GEMM_RGB2 only.)
#include "ffn_gemm_mx4_kernels.h"

namespace moeinf {

template <int NMAT>
static void launch_ffn_gemm_mx4_t(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st) {
  if (f.kernel == FFN_HYB) {  // codes -> registers, activations -> LDS
    constexpr int RW = NMAT == 2 ? 1 : 2;
    KL((ffn_gemm_hyb_kernel<mx4w_t, NMAT, RW, 4, true>), dim3((grid.x + 4 * RW - 1) / (4 * RW), grid.y), dim3(256), 0, st, s);
  } else {  // FFN_LDS
#define GO(RG, NW) KL((ffn_gemm_lds_kernel<mx4w_t, NMAT, RG, NW, true>), dim3((grid.x + RG - 1) / RG, grid.y), dim3(NW * 64), 0, st, s)
    if constexpr (NMAT == 1) {
      if (f.rgb == 8) { if (f.waves == 8) GO(8, 8); else GO(8, 4); return; }
    }
    if (f.waves == 8) GO(4, 8); else GO(4, 4);
#undef GO
  }
}

void launch_ffn_gemm_mx4(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st) {
  if (f.nmat == 2) launch_ffn_gemm_mx4_t<2>(s, grid, f, st);
  else launch_ffn_gemm_mx4_t<1>(s, grid, f, st);
}

}  // namespace moeinf
