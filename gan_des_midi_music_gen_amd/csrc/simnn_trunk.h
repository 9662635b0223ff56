// Convolution trunk of model 1's discriminator (GAN_DES/SIMNN.py:123-125, 136-139) for gfx950: what every trunk file needs.
//
//   x (B,H,W) fp32 --conv1 k2 p1 +ReLU +pool2--> p1 (B,H1,W1,16) channels-last
//                  --conv2 k3 p1 +ReLU +pool2--> p2 (B,32,H2,W2) channel-major (= the reference's flatten order)
//
// conv1 (K = 4) is an HBM-bound stencil: one lane per pooled pixel, all 16 channels in registers.
// conv2 (K = 144) is an implicit GEMM on MFMA with M = output channels, N = 16 consecutive pixels of a row,
// the input halo band staged once in LDS as [row][col][channel]; ReLU, the 2x2 max-pool and its argmax code are
// applied to the accumulator tile (row pair in two accumulators, column pair by a lane swap) before anything is
// written, so the full-resolution conv outputs never touch HBM.  Backward kernels rebuild the sparse full-resolution
// gradient (one non-zero per pooling window) in LDS from the pooled gradient + the 1-byte code.
//
// T = float : exact-fp32 mode, v_mfma_f32_16x16x4_f32, LDS pixel records padded to avoid bank conflicts
// T = __bf16: bf16 storage + v_mfma_f32_16x16x32_bf16, fp32 accumulation
//
// One .hip per kernel family, each with its kernels and its C-ABI entry points:
//   simnn_conv1.hip (forward, backward-weight, backward-data)   simnn_slab_sum.hip (the fixed-order slab sum)
//   simnn_conv2_fwd.hip (pack + forward)   simnn_conv2_bwd_data.hip (plain + fused)   simnn_conv2_bwd_weight.hip
//   simnn_adam.hip (the discriminator's one-launch optimizer step)
#pragma once
#include "buffer_ops.h"

// Diagnostic build only (-DGDM_STAMPS, tools/stamps.py): per-workgroup cycle totals of the phases of a persistent
// kernel's tile loop, taken with s_memtime by every wave and written by wave 0 to a buffer nothing else reads.
// Device globals do not cross translation units: every trunk file has its own buffer, and a file that stamps exports
// its reader with GDM_STAMP_READER(family) as gdm_debug_read_stamps_<family>.
#ifdef GDM_STAMPS
namespace {
__device__ unsigned long long gdm_stamp_buf[1024 * 8];
struct Stamps {
  uint64_t last, ph[8];
  __device__ __forceinline__ void start() {
    for (int k = 0; k < 8; ++k) ph[k] = 0;
    __builtin_amdgcn_sched_barrier(0);
    last = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void mark(int k) {
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t now = __builtin_amdgcn_s_memtime();
    ph[k] += now - last;
    last = now;
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void flush() {
    if (threadIdx.x == 0)
      for (int k = 0; k < 8; ++k) gdm_stamp_buf[(blockIdx.x & 1023) * 8 + k] = ph[k];
  }
};
}  // namespace
#define STAMP_DECL Stamps stamps_; stamps_.start()
#define STAMP(k) stamps_.mark(k)
#define STAMP_FLUSH stamps_.flush()
#define STAMP_ARG , Stamps& stamps_
#define STAMP_PASS , stamps_
#define GDM_STAMP_READER(family)                                                                           \
  extern "C" int gdm_debug_read_stamps_##family(unsigned long long* host_out, int n) {                     \
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(gdm_stamp_buf), sizeof(unsigned long long) * n);  \
  }
#else
#define STAMP_DECL
#define STAMP(k)
#define STAMP_FLUSH
#define STAMP_ARG
#define STAMP_PASS
#define GDM_STAMP_READER(family)
#endif

#define DISPATCH_T(dtype, CALL)                  \
  if ((dtype) == GDM_BF16) { using T = __bf16; CALL; } else { using T = float; CALL; }

constexpr int COLS = 64;   // conv-output columns handled per workgroup (column super-tile)
constexpr int ROWS = 4;    // conv-output rows per tile / step
constexpr int XROWS = 2 * ROWS + 1;                          // input-window rows behind ROWS rows of the p1 geometry

// index (in 16-bit fields) of code1's field for pooled pixel pw of row `row` (= image * H1 + pooled row), group g
__device__ __forceinline__ uint32_t code1_field(uint32_t row, int Q1, int pw, int g) {
  return ((row * (uint32_t)Q1 + (uint32_t)(pw >> 2)) * 4u + (uint32_t)g) * 4u + (uint32_t)(pw & 3);
}

template <typename T> struct Px;  // LDS pixel-record strides (elements) for 16- and 32-channel records
template <> struct Px<float> { static constexpr int S16 = 17, S32 = 33; };
template <> struct Px<__bf16> { static constexpr int S16 = 16, S32 = 32; };

#ifndef GDM_IN_LOAD_AUX
#define GDM_IN_LOAD_AUX 0            // cache policy of the x / code1 loads: non-temporal (2) was measured 3 % SLOWER (x is
                                     // read again by the backward of the same iteration: it wants to stay in the Infinity Cache)
#endif
// Cache policy of the big write-once activation streams (conv1: p1 + code1, conv2: p2 + code2; 84 + 75 MB per 256 samples):
// non-temporal.  They are consumed by a LATER kernel, and on this 8-XCD part a kernel boundary writes the XCD's dirty L2
// lines back before the dependent kernel starts; streaming them out as they are produced took 0.5-0.9 % off the
// iteration in same-box A/B (the kernels themselves run as before).  -DGDM_ACT_STORE_AUX=0 restores the default policy.
#ifndef GDM_ACT_STORE_AUX
#define GDM_ACT_STORE_AUX 2
#endif
#ifndef GDM_ACT_STORE_AUX2
#define GDM_ACT_STORE_AUX2 GDM_ACT_STORE_AUX
#endif

// =====================================================================================================================
// conv2 block.  Tile = ROWS (4) conv rows x COLS (128) conv columns of one image per 256-thread workgroup; wave w owns
// columns [32w, 32w+32).  Activations/gradients around it are channels-last:
//   p1, dp1 (B,H1,W1,16)   p2, dp2 (B,H2,W2,32)   code2 (B,H2,W2,16) uint8: one byte per channel PAIR (2j, 2j+1) =
//   8 * (c_even + 5 * c_odd) with c = 0..3 argmax position, 4 = ReLU-dead -- i.e. the byte offset of the pair's entry
//   in the backward kernels' 8-byte selector tables (simnn_conv2_bwd.h), so that rebuilding the sparse full-resolution
//   gradient costs one v_bfe, two table reads and four v_perm per two channels and four positions
// Weights are consumed from a pre-packed image (gdm_simnn_conv2_pack, rebuilt after every optimizer step):
//   forward  image Wf[32][KPF]: k = tap*16 + ci                       (zero padded to the MFMA k granularity)
//   backward image Wb[16][KPB]: k = tap'*32 + o with tap' = 8 - tap   (the flipped kernel of the data gradient)
// =====================================================================================================================
template <typename T> struct C2 {
  static constexpr int KPF = sizeof(T) == 2 ? 168 : 146;
  static constexpr int KPB = sizeof(T) == 2 ? 296 : 290;
  static constexpr int WF_ELEMS = 32 * KPF, WB_ELEMS = 16 * KPB;
  static constexpr int S16 = Px<T>::S16, S32 = Px<T>::S32;
  static constexpr int WP = COLS + 2;
  // records per parity plane of a band row in conv2 forward's even/odd-split image: WP / 2 = 33, padded to 34 -- with 33
  // the four pixels of an 8-lane ds_write_b128 group (columns c, c+1, c+2, c+3 -> planes 0, 1, 0, 1) put two of them on the
  // same 32 store banks (33 * 32 B = 32 mod 128): every band store was 2-way conflicted; 34 * 32 B = 64 mod 128 separates them
  static constexpr int HP = WP / 2 + 1;
  static constexpr int IN_ELEMS = (ROWS + 2) * 2 * HP * S16;     // p1 halo band (split image: 2 planes per row)
};

// Element i of conv2's packed forward (BWD = false) or backward (BWD = true) weight image, read from the (32,16,3,3)
// weights at w (global memory in conv2_pack_kernel, the LDS copy of the freshly updated weights in simnn_adam_kernel).
template <typename T, bool BWD>
__device__ __forceinline__ float conv2_packed_value(const float* w, int i) {
  if constexpr (!BWD) {
    const int o = i / C2<T>::KPF, k = i % C2<T>::KPF;
    return k < 144 ? w[(o * 16 + (k & 15)) * 9 + (k >> 4)] : 0.f;
  } else {
    const int ci = i / C2<T>::KPB, k = i % C2<T>::KPB;
    return k < 288 ? w[((k & 31) * 16 + ci) * 9 + (8 - (k >> 5))] : 0.f;
  }
}

// A packed weight image (ELEMS elements of T) on its way from global memory to LDS, as a begin / finish pair: begin
// issues all of its 16-byte loads into registers -- a compile-time number of buffer loads outside any branch, lanes past
// the end read zeros that are never stored --, finish stores them.  A kernel calls begin FIRST, then issues its first
// activation prefetches, does its LDS-only set-up and calls finish just before its first barrier: memory operations
// retire in order, so finish waits for the image alone (vmcnt(N), N = the activation loads issued behind it) and the
// kernel's start costs one memory round trip.  As a loop of load -> wait -> ds_write in front of the first prefetch it
// cost three dependent round trips and a fourth for the prefetch.
template <typename T, int ELEMS> struct LdsImage {
  static_assert(ELEMS * sizeof(T) % 16 == 0, "whole 16-byte chunks");
  static constexpr int CHUNKS = ELEMS * (int)sizeof(T) / 16, ITERS = (CHUNKS + 255) / 256;
  f32x4 v[ITERS];
};
template <typename T, int ELEMS>
__device__ __forceinline__ void lds_image_begin(LdsImage<T, ELEMS>& im, const T* __restrict__ src) {
  const rsrc_t r = make_rsrc(src, (uint32_t)(ELEMS * sizeof(T)));
#pragma unroll
  for (int k = 0; k < LdsImage<T, ELEMS>::ITERS; ++k) {
    const int i = threadIdx.x + 256 * k;
    im.v[k] = buf_load16(r, i < LdsImage<T, ELEMS>::CHUNKS ? (uint32_t)i * 16u : BUF_OOB);
  }
}
template <typename T, int ELEMS>
__device__ __forceinline__ void lds_image_finish(const LdsImage<T, ELEMS>& im, T* __restrict__ dst) {
#pragma unroll
  for (int k = 0; k < LdsImage<T, ELEMS>::ITERS; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < LdsImage<T, ELEMS>::CHUNKS) ((f32x4*)dst)[i] = im.v[k];
  }
}

// ---------------------------------------------------------------------------------------------------- work plans
// Workgroup caps of the trunk's kernels (all persistent: a workgroup walks its items).  An experiment build may
// override the ones that name an environment variable (tools/ sweeps).
namespace cap {
// fused conv2 backward-data, 2 resident workgroups per CU (measured at 2B = 512: 384 -> 132 us, 512 -> 118, 640 -> 121,
// 768 -> 121)
inline int c2_bwd_fused() { static const int v = GDM_TUNABLE("GDM_BD_CAP", 512); return v; }
constexpr int c2_bwd_data = 768;
// conv2 backward-weight, measured at 2B = 512 (1024 strips): 768 workgroups (3 per CU) 73 us, 1024 (4 per CU) 84 us,
// 512 78 us; finer items (more segments per strip) only add pseudo steps
inline int c2_bwd_weight() { static const int v = GDM_TUNABLE("GDM_BW_CAP", 768); return v; }
inline int c2_fwd() { static const int v = GDM_TUNABLE("GDM_C2F_CAP", 768); return v; }    // 3 workgroups per CU
// conv1 forward: 6 workgroups per CU (2048: +0.6 % per iteration)
inline int c1_fwd() { static const int v = GDM_TUNABLE("GDM_C1_CAP", 1536); return v; }
constexpr int c1_slabs = 1024;       // conv1 backward-weight workgroups = slabs
constexpr int c1_bwd_data = 8192;
}  // namespace cap

// Work decomposition of the conv2 backward kernels (the C++ twin of tests/trunk_ref.py's _seg_plan): items = (image,
// row segment, `cols`-column tile).  Whole-height strips when `target` of them fill the chip; small batches are cut
// into row segments (each pays one pseudo step).  A pure function of the shapes: the slab count of the fused variant
// must be reproducible by _finish.  nseg_forced > 0 (experiments) fixes the segments per strip.
struct SegPlan { int n_ctiles, nseg, seg_len, n_items, blocks; };
inline SegPlan seg_plan(int B, int H1, int W1, int target, int cols, int cap, int nseg_forced = 0) {
  SegPlan p;
  const int nrq = (H1 + ROWS - 1) / ROWS;
  p.n_ctiles = (W1 + cols - 1) / cols;
  const int64_t strips = (int64_t)B * p.n_ctiles;
  int nseg = nseg_forced > 0 ? nseg_forced : (int)((target + strips - 1) / strips);
  const int max_seg = nrq / 2 > 1 ? nrq / 2 : 1;            // at least two steps per segment
  nseg = nseg < 1 ? 1 : (nseg > max_seg ? max_seg : nseg);
  p.seg_len = (nrq + nseg - 1) / nseg;
  p.nseg = (nrq + p.seg_len - 1) / p.seg_len;
  p.n_items = (int)(strips * p.nseg);
  p.blocks = p.n_items < cap ? p.n_items : cap;
  return p;
}

// the conv2 kernels address their tensors through 32-bit buffer offsets (see make_rsrc): largest tensor < 2 GiB
inline bool fits_buffer_addressing(int B, int H1, int W1) { return (int64_t)B * H1 * W1 * 16 * 4 < (int64_t)1 << 31; }

// simnn_slab_sum.hip: fixed-order sum of `nslabs` slabs of `width` floats into their sink, using `scratch`
// (>= 64 * width floats).  sink 1 = conv1 gradients (dw[64], db[16], optional accumulate), 2 = conv2 gradients.
void gdm_launch_slab_sum(int sink, const float* slabs, int nslabs, int width, float* scratch, float* dw, float* db,
                         int accumulate, hipStream_t s);
