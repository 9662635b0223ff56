// Vectorised bf16-MFMA GEMM for the weight-/activation-streaming products of the hot path (M <= a few hundred, K or N
// in the tens of thousands): model 1's fc1 forward / dW / dX (GAN_DES/SIMNN.py:126,140 and their autograd mm's), the
// generators' ConvTranspose2d-as-GEMM products and model 2's conv GEMMs.
//
//   128x128 output tile per 256-thread workgroup (4 waves as 2x2, each 64x64 = 4x4 v_mfma_f32_16x16x32_bf16 tiles).
//   These products are bandwidth-bound, so what decides their speed is bytes in flight.  Operand tiles are fetched
//   ahead into registers with 16-byte buffer loads (out-of-range chunks read zeros: no branch around a load, counted
//   waits) and the LDS images are XOR-swizzled so that fragment reads and stores are bank-conflict-free.  Two variants:
//   K tile 64 fetched TWO tiles ahead with double-buffered LDS (one barrier per tile) for skinny long-K products that
//   put few workgroups on a CU, and K tile 32 fetched one tile ahead (16 KB LDS) for products with many short ones.
//   With two bf16 operands (fc1's three products) the loads are pinned in stage order, so that the wait in front of a
//   stage's LDS stores leaves the younger stage in flight, and K tile 32 fetches two tiles ahead as well.
//
// Operand layouts (chosen on the host from the strides; anything else falls back to the generic kernel in gemm.hip):
//   K-major  (k stride 1):   LDS image [row][KT k]   fragment = one ds_read_b128
//                            16-byte piece p of row r sits at piece p ^ kswz(r)
//   R-major  (row stride 1): LDS image [k][128 rows] fragment = two ds_read_b64_tr_b16 (hardware transpose: the
//                            contraction index is the slow axis in memory)
//                            16-element block b of k-row k sits at block b ^ ((k & 3) | ((k >> 1) & 4))
// fp32 operands are converted to bf16 on the way into LDS.  The MFMA is issued with the operands swapped (D^T), so a
// lane ends up with 4 CONSECUTIVE n of one output row: row-major C is written 16 B (fp32) / 8 B (bf16) per lane.
//
// The kernel template lives in gemm_bf16_kernel.h; its instantiations are compiled in gemm_bf16_kt{32,64}_{bf16,f32}a.hip
// and gemm_bf16_ring_kt{32,64}.hip.
#include "gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128;

// rows = extent of the non-contracted axis.  16-byte chunks must be inside or outside the matrix as a whole, and the
// operand must be addressable through one 32-bit buffer descriptor.
inline bool operand_ok(const void* p, int dtype, int64_t s_row, int64_t s_k, int rows, int K, bool* kmaj) {
  const int64_t esz = dtype == GDM_BF16 ? 2 : 4, epc = 16 / esz;
  if (((uintptr_t)p & 15) != 0) return false;
  if (s_k == 1 && s_row >= 1 && (s_row * esz) % 16 == 0 && K % epc == 0) {
    *kmaj = true;
    return ((int64_t)(rows - 1) * s_row + K) * esz < ((int64_t)1 << 31);
  }
  if (s_row == 1 && s_k >= 1 && (s_k * esz) % 16 == 0 && rows % epc == 0) {
    *kmaj = false;
    return ((int64_t)(K - 1) * s_k + rows) * esz < ((int64_t)1 << 31);
  }
  return false;
}

}  // namespace

bool gdm_gemm_bf16_fast_ok(const GemmArgs& g, int a_dtype, int b_dtype, bool* a_kmaj, bool* b_kmaj) {
  if (!operand_ok(g.A, a_dtype, g.sam, g.sak, g.M, g.K, a_kmaj)) return false;
  if (!operand_ok(g.B, b_dtype, g.sbn, g.sbk, g.N, g.K, b_kmaj)) return false;
  if (g.scn != 1) return false;
  const int64_t csz = g.c_dtype == GDM_BF16 ? 2 : 4;
  if (g.N % 4 == 0) {   // vector epilogue: rows of C and the bias must allow 4-element accesses
    if ((g.scm * csz) % (4 * csz) != 0 || ((uintptr_t)g.C & (4 * csz - 1)) != 0) return false;
    if (g.bias_n && ((uintptr_t)g.bias_n & 15) != 0) return false;
  }
  // tiny problems gain nothing from 128x128 tiles
  if ((int64_t)g.M * g.N < 64 * 64) return false;
  return true;
}

bool gdm_gemm_bf16_fast_deep(int M, int N, int split_k, int k_per_split) {
  const int MT = (M + BM - 1) / BM, NTl = (N + BN - 1) / BN;
  const int outer = NTl * split_k;
  // split-K products (few workgroups per CU, long K loops): bytes in flight per workgroup decide -> deep variant
  bool deep = split_k > 1 && (int64_t)outer * MT <= 512 && k_per_split >= 256;
  static const int force = GDM_TUNABLE("GDM_GEMM_VARIANT", -1);
  if (force >= 0) deep = force == 1;
  return deep;
}

int gdm_gemm_bf16_fast_launch(const GemmArgs& g, int a_dtype, int b_dtype, const GemmPlan& p, hipStream_t s) {
  const int MT = (g.M + BM - 1) / BM, NTl = (g.N + BN - 1) / BN;
  const int outer = NTl * g.split_k;
  dim3 grid((unsigned)(((outer + 7) / 8) * 8 * MT));
  // K tile 32, one tile ahead, 16 KB LDS (many workgroups per CU); or K tile 64, two tiles ahead, 64 KB LDS
  const bool deep = p.kernel == GDM_GEMM_KERNEL_FAST_K64;
  const bool both_bf16 = a_dtype == GDM_BF16 && b_dtype == GDM_BF16;
  // k tiles of one workgroup: slice z of the interleaved split takes tiles z, z + split_k, ...
  const int kt = deep ? 64 : 32;
  const int tiles = ((g.K + kt - 1) / kt + g.split_k - 1) / g.split_k;
  if (both_bf16 && deep) {
    // loads pinned in stage order (the deep variant's slabs are four tiles or more: k_per_split >= 256)
    gdm_gemm_bf16_ring_kt64(g, p.a_kmaj, p.b_kmaj, grid, s);
  } else if (both_bf16 && tiles >= GDM_GEMM_RING_K32) {
    // the register ring; a loop shorter than the ring would only multiply its zero tiles
    gdm_gemm_bf16_ring_kt32(g, p.a_kmaj, p.b_kmaj, grid, s);
  } else if (a_dtype == GDM_BF16 && deep) {
    gdm_gemm_bf16_kt64_bf16a_f32b(g, p.a_kmaj, p.b_kmaj, grid, s);
  } else {
    auto* launch = a_dtype == GDM_BF16 ? gdm_gemm_bf16_kt32_bf16a : (deep ? gdm_gemm_bf16_kt64_f32a : gdm_gemm_bf16_kt32_f32a);
    launch(g, p.a_kmaj, b_dtype, p.b_kmaj, grid, s);
  }
  GDM_LAUNCH_OK("gdm_gemm(bf16 fast path)");
  return GDM_OK;
}
