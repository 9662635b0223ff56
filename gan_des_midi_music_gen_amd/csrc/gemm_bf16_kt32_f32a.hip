// gemm_bf16_fast, K tile 32 fetched one tile ahead, f32 A operand: 8 of the 32 instantiations (gemm_bf16_kernel.h).
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_kt32_f32a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s) {
  launch_instances<float, 32, 1>(g, a_kmaj, b_dtype, b_kmaj, grid, s);
}
