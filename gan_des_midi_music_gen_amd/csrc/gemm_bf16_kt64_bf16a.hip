// gemm_bf16_fast, K tile 64 fetched two tiles ahead, bf16 A operand: 8 of the 32 instantiations (gemm_bf16_kernel.h).
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_kt64_bf16a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s) {
  launch_instances<__bf16, 64, 2>(g, a_kmaj, b_dtype, b_kmaj, grid, s);
}
