// ffn_gemm_f8.hip — fp8-slot forms (T = f8w_t: bf16 activations, the routed experts' weights fp8 tiles up-cast in registers) of
// the grouped-GEMM kernels for experts with many rows: the hybrid, the LDS-staged and the register-ring kernel (ffn_gemm_f8_kernels.h,
// ffn_ring2_kernel.h).  Which one a stage takes: ffn_form (kernels.h).  Called by launch_ffn_stage (kernels.hip).  Its own
// translation unit, so the bf16 and fp16 units do not grow.
#include "ffn_gemm_f8_kernels.h"
#include "ffn_ring2_kernel.h"

namespace moeinf {

void launch_ffn_gemm_f8(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st) {
  if (f.nmat == 2) { if (f.kernel == FFN_RING2) launch_ring2<f8w_t, 2>(s, grid, f.ring, st); else launch_ffn_gemm_t<f8w_t, 2>(s, grid, f, st); }
  else { if (f.kernel == FFN_RING2) launch_ring2<f8w_t, 1>(s, grid, f.ring, st); else launch_ffn_gemm_t<f8w_t, 1>(s, grid, f, st); }
}

}  // namespace moeinf
