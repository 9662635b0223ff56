// gemm_bf16_fast, K tile 32 fetched one tile ahead, bf16 A operand: 8 instantiations (gemm_bf16_kernel.h).  bf16 x bf16
// products of GDM_GEMM_RING_K32 k tiles per workgroup or more run the ring instances of gemm_bf16_ring_kt32.hip.
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_kt32_bf16a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s) {
  if (b_dtype == GDM_BF16) launch_layouts<__bf16, __bf16, 32, 1, false>(g, a_kmaj, b_kmaj, grid, s);
  else launch_layouts<__bf16, float, 32, 1, false>(g, a_kmaj, b_kmaj, grid, s);
}
