// Shared by gemm.hip (generic strided kernel) and gemm_bf16.hip (vectorised bf16-MFMA kernel).
#pragma once
#include "gdm_common.h"

struct GemmArgs {
  const void* A; int64_t sam, sak;
  const void* B; int64_t sbk, sbn;
  void* C; int c_dtype; int64_t scm, scn;
  int M, N, K;
  const float* bias_n; const float* bias_m; int act; float slope;
  int split_k, k_per_split; float* ws;
};

__device__ __forceinline__ void gemm_epilogue_store(const GemmArgs& g, int m, int n, float v) {
  if (g.bias_n) v += g.bias_n[n];
  if (g.bias_m) v += g.bias_m[m];
  v = apply_act(v, g.act, g.slope);
  store_from_f32(g.C, g.c_dtype, (int64_t)m * g.scm + (int64_t)n * g.scn, v);
}

// The path of one product, decided by gemm_plan() in gemm.hip and nowhere else: gdm_gemm launches from it and
// gdm_gemm_plan reports it (kernel: GDM_GEMM_KERNEL_*, reduce: GDM_GEMM_REDUCE_* of include/gdm.h).
struct GemmPlan {
  int kernel;
  bool a_kmaj, b_kmaj;        // operand layouts of the fast kernels (false on the generic path)
  int split_k, k_per_split;   // the clamped split and the slab width in k
  int reduce;
  size_t ws_bytes;
};

// gemm_bf16.hip.  fast_ok: true if the vectorised kernel can take this problem (layouts contiguous along k or along
// m/n, 16-byte aligned rows, row-major C), with the layout of each operand; fast_deep: the K-tile-64 variant for this
// grid and slab width; fast_launch launches the instance the plan names (the split-K reduce is left to the caller).
bool gdm_gemm_bf16_fast_ok(const GemmArgs& g, int a_dtype, int b_dtype, bool* a_kmaj, bool* b_kmaj);
bool gdm_gemm_bf16_fast_deep(int M, int N, int split_k, int k_per_split);
int gdm_gemm_bf16_fast_launch(const GemmArgs& g, int a_dtype, int b_dtype, const GemmPlan& p, hipStream_t s);
// gemm_bf16_kt{32,64}_{bf16,f32}a.hip: the kernel instantiations of one variant (K tile) and A dtype at the variant's
// own prefetch depth; gemm_bf16_ring_kt{32,64}.hip: the bf16 x bf16 instantiations with a deeper register ring
void gdm_gemm_bf16_kt32_bf16a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s);
void gdm_gemm_bf16_kt32_f32a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s);
void gdm_gemm_bf16_kt64_bf16a_f32b(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s);
void gdm_gemm_bf16_kt64_f32a(const GemmArgs& g, bool a_kmaj, int b_dtype, bool b_kmaj, dim3 grid, hipStream_t s);
void gdm_gemm_bf16_ring_kt32(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s);
void gdm_gemm_bf16_ring_kt64(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s);
// register stages of the ring instances = tiles fetched ahead.  2 and 2 are the fastest of the depths measured on
// fc1's three products (K tile 64: 2, 3, 4; K tile 32: 1, 2, 4 -- DESIGN.md section 5); experiment builds override.
#ifndef GDM_GEMM_RING_K64
#define GDM_GEMM_RING_K64 2
#endif
#ifndef GDM_GEMM_RING_K32
#define GDM_GEMM_RING_K32 2
#endif
constexpr int GDM_GEMM_FAST_KT = 64;   // split-K slabs are multiples of the widest K tile
