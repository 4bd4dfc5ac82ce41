// ffn_gemm_ring2.hip — bf16 entry point of the register-ring GEMM (kernel: ffn_ring2_kernel.h).  Which form a stage takes:
// ring2_form (kernels.h).  Called by launch_ffn_stage (kernels.hip).
#include "ffn_ring2_kernel.h"

namespace moeinf {

void launch_ffn_gemm_ring2_bf16(const FfnStage& s, dim3 grid, const FfnForm& f, hipStream_t st) {
  if (f.nmat == 2) launch_ring2<uint16_t, 2>(s, grid, f.ring, st);
  else launch_ring2<uint16_t, 1>(s, grid, f.ring, st);
}

}  // namespace moeinf
