// gemm_bf16_fast, K tile 64, bf16 x bf16 operands (fc1 forward's pair), GDM_GEMM_RING_K64 register stages with the
// loads pinned in stage order: 4 instantiations (gemm_bf16_kernel.h).
#include "gemm_bf16_kernel.h"

void gdm_gemm_bf16_ring_kt64(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s) {
  launch_layouts<__bf16, __bf16, 64, GDM_GEMM_RING_K64, true>(g, a_kmaj, b_kmaj, grid, s);
}
