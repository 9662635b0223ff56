// gemm_bf16_fast, K tile 64 fetched two tiles ahead, f32 A operand: 8 instantiations (gemm_bf16_kernel.h).
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_kt64_f32a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s) {
  if (b_dtype == GDM_BF16) launch_layouts<float, __bf16, 64, 2, false>(g, a_kmaj, b_kmaj, grid, s);
  else launch_layouts<float, float, 64, 2, false>(g, a_kmaj, b_kmaj, grid, s);
}
