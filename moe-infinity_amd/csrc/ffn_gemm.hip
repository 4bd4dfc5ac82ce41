// ffn_gemm.hip — bf16 and fp32 entry point of the grouped-GEMM kernels for experts with many rows (kernels: ffn_gemm_kernels.h;
// which one runs: ffn_form, kernels.h).  Called by launch_ffn_stage (kernels.hip).
#include "ffn_gemm_kernels.h"

namespace moeinf {

void launch_ffn_gemm(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st) {
  if (s.dtype == DT_BF16) { if (f.nmat == 1) launch_ffn_gemm_t<uint16_t, 1>(s, grid, f, st); else launch_ffn_gemm_t<uint16_t, 2>(s, grid, f, st); }
  else { if (f.nmat == 1) launch_ffn_gemm_t<float, 1>(s, grid, f, st); else launch_ffn_gemm_t<float, 2>(s, grid, f, st); }
}

}  // namespace moeinf
