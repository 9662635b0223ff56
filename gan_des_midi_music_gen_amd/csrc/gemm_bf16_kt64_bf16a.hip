// gemm_bf16_fast, K tile 64 fetched two tiles ahead, bf16 A operand with an fp32 B operand: 4 instantiations
// (gemm_bf16_kernel.h).  bf16 x bf16 runs the ring instances of gemm_bf16_ring_kt64.hip.
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_kt64_bf16a_f32b(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s) {
  launch_layouts<__bf16, float, 64, 2, false>(g, a_kmaj, b_kmaj, grid, s);
}
