// conv1 of model 1's discriminator trunk (simnn_trunk.h): forward, backward-weight and backward-data.
#include "simnn_trunk.h"

namespace {

// =====================================================================================================================
// conv1 forward: Conv2d(1,16,k2,s1,p1) + ReLU + MaxPool2d(2)
// code1 = one 16-bit field per (pooled pixel, 4-channel group g): nibble k (bits 4k..4k+3) belongs to channel 4g+k:
//   bits [1:0] = argmax position (dy*2+dx, first max in scan order like aten::max_pool2d_with_indices),
//   bit 2 = channel is live (pooled value > 0, i.e. ReLU passes gradient), bit 3 = 0.
// Fields are stored "quad-major": [image][pooled row][quad = pw / 4][group g][pw % 4], Q1 = ceil(W1 / 4) quads per row
// (8 bytes per pixel).  The forward's lane (pixel, group) writes one field, as before; in the fused backward a lane owns
// ONE channel and FOUR neighbouring pixels (the transposed MFMA result), and the four fields of its channel group are
// then 8 contiguous bytes -- one load, no cross-lane transpose on either side.  Pixels >= W1 of a row's last quad
// hold 0 (dead).
//
// The 2x2 stencil is a [16 channels x 4 taps] x [4 taps x pixels] product: one exact-fp32 v_mfma_f32_16x16x4_f32 per
// pooling position and 16 pooled pixels, bias as the accumulator's initial value.  A wave takes units of 16 pooled
// pixels of one pooled row; in the result lane (lr, lg) holds channels 4lg..4lg+3 of pixel lr for all four positions,
// so max-pool, argmax and ReLU are in-lane and the lane stores 8/16 bytes of p1 and one 16-bit code field.  (As a VALU
// stencil this layer cost ~10 instructions per output value and was issue-bound at 40 % of its memory roofline.)
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                        int bsplit, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int B, int H, int W, int H1,
                                                        int W1, int n_rows, T* __restrict__ p1,
                                                        uint16_t* __restrict__ code1) {
  const int t = threadIdx.x, l = t & 63, lr = l & 15, lg = l >> 4;
  const int Q1 = (W1 + 3) >> 2;
  // the wave index is uniform: keep everything derived from it in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (t >> 6)), n_waves = gridDim.x * 4;
  const int upr = (W1 + 15) >> 4;                            // units per pooled row
  // the batch is the concatenation of two input tensors (images 0 .. bsplit-1 | bsplit .. B-1: real | generated)
  const rsrc_t xr0 = make_rsrc(x0, (uint32_t)bsplit * H * W * 4);
  const rsrc_t xr1 = make_rsrc(x1, (uint32_t)(B - bsplit) * H * W * 4);
  const rsrc_t pr = make_rsrc(p1, (uint32_t)B * H1 * W1 * 16 * sizeof(T));
  const rsrc_t cr = make_rsrc(code1, (uint32_t)B * H1 * Q1 * 32);
  // A operand: lane (row = channel lr, k = tap lg); accumulator rows 4lg + r = channels
  const float aw = w[lr * 4 + lg];
  const f32x4 b4 = {bias[4 * lg], bias[4 * lg + 1], bias[4 * lg + 2], bias[4 * lg + 3]};
  // B operand: lane (k = tap lg = kh*2+kw, column = pixel lr) reads x[2ph-1+kh+dy][2pw-1+kw+dx] for position (dy,dx)
  const int r_lo = (lg >> 1) - 1, c_lo = 2 * lr + (lg & 1) - 1;
  uint32_t loff[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) loff[p] = (uint32_t)(((r_lo + (p >> 1)) * W + c_lo + (p & 1)) * 4);   // may wrap: added to base

  // Work is dealt by pooled ROW: wave w takes rows w, w + n_waves, ... of the (b, ph) row space and walks each row's
  // units left to right in CHUNKS of DEPTH units that share one row record: everything that depends on the row (base
  // offsets, row-interior flag, validity) is computed once per row, behind a scalar branch, and a unit costs a handful
  // of scalar instructions.  The CU's ONE scalar unit is what this kernel queues for: with per-unit position
  // arithmetic with carries (~100 SALU per unit) it was slower than its VALU work; with four independently advancing
  // slots (~45 SALU per unit, a row change every other step of each slot) a phase-stamp build still showed 36 % of a
  // wave's time in "bookkeeping + next loads" (`tools/stamps.py c1`).
  struct Row { int ph, b; uint32_t xrow, pixrow, crow; bool interior, valid, second; };
  const int dph = n_waves % H1, db = n_waves / H1;
  auto set_row = [&](Row& q) {
    const int b = min(q.b, B - 1);                           // past the end: re-read the last image (stores are dropped)
    q.second = b >= bsplit;
    q.xrow = (uint32_t)((((q.second ? b - bsplit : b) * H + 2 * q.ph) * W) * 4);
    q.pixrow = (uint32_t)((b * H1 + q.ph) * W1);
    q.crow = (uint32_t)(b * H1 + q.ph);
    q.interior = q.ph > 0 && 2 * q.ph + 1 < H;
    q.valid = q.b < B;
  };
  auto load = [&](const Row& q, int seg, float (&xv)[4]) {
    const rsrc_t xr = q.second ? xr1 : xr0;                  // scalar select
    const uint32_t base = q.xrow + 128u * (uint32_t)seg;
    if (q.interior && seg > 0 && 32 * seg + 32 < W) {        // interior unit (scalar test)
      // the lane's 2x2 patch as two 8-byte loads (4-byte aligned): memory instructions, not bytes, are what the
      // address unit charges for
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const uint64_t two = buf_load8<GDM_IN_LOAD_AUX>(xr, base + loff[2 * dy]);
        xv[2 * dy] = __builtin_bit_cast(float, (uint32_t)two);
        xv[2 * dy + 1] = __builtin_bit_cast(float, (uint32_t)(two >> 32));
      }
      return;
    }
    // edge unit (also: a unit past the end of its row, seg >= upr -- its stores are dropped)
    const int row0 = 2 * q.ph + r_lo, col0 = 32 * seg + c_lo;
    const bool rok[2] = {(unsigned)row0 < (unsigned)H, (unsigned)(row0 + 1) < (unsigned)H};
    const bool cok[2] = {(unsigned)col0 < (unsigned)W, (unsigned)(col0 + 1) < (unsigned)W};
#pragma unroll
    for (int p = 0; p < 4; ++p) xv[p] = buf_load4<GDM_IN_LOAD_AUX>(xr, (rok[p >> 1] && cok[p & 1]) ? base + loff[p] : BUF_OOB);
  };
  STAMP_DECL;
  auto finish = [&](const Row& q, int seg, const float (&xv)[4]) {
    f32x4 acc[4];
#ifdef GDM_STAMPS
    asm volatile("" :: "v"(xv[0]), "v"(xv[1]), "v"(xv[2]), "v"(xv[3]));      // the unit's loads have landed
    STAMP(0);
#endif
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, xv[p], b4, 0, 0, 0);
#ifdef GDM_STAMPS
    asm volatile("" :: "v"(acc[3][3]));                                        // the MFMAs have finished
    STAMP(1);
#endif
    uint32_t field = 0;
    float best[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v0 = acc[0][r], v1 = acc[1][r], v2 = acc[2][r], v3 = acc[3][r];
      const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
      uint32_t pos = 3u;                        // select chain, last write wins = first maximum in scan order
      pos = v2 == m ? 2u : pos;
      pos = v1 == m ? 1u : pos;
      pos = v0 == m ? 0u : pos;
      best[r] = fmaxf(m, 0.f);
      field |= (m > 0.f ? pos | 4u : pos) << (4 * r);
    }
    const int pw = 16 * seg + lr;
    const uint32_t pix = q.pixrow + (uint32_t)pw;
    const bool ok = q.valid && pw < W1;
#ifdef GDM_STAMPS
    asm volatile("" :: "v"(field), "v"(best[0]), "v"(best[3]));
    STAMP(2);
#endif
    if constexpr (sizeof(T) == 2) {
      bf16x4 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = (__bf16)best[r];
      buf_store8<GDM_ACT_STORE_AUX>(pr, ok ? pix * 32u + 8u * lg : BUF_OOB, __builtin_bit_cast(uint64_t, h));
    } else {
      buf_store16(pr, ok ? pix * 64u + 16u * lg : BUF_OOB, (f32x4){best[0], best[1], best[2], best[3]});
    }
    // the whole last quad is written (zeros beyond W1): its consumers load four pixels' fields at once
    buf_store2<GDM_ACT_STORE_AUX2>(cr, (q.valid && pw < 4 * Q1) ? code1_field(q.crow, Q1, pw, lg) * 2u : BUF_OOB,
                                   ok ? field : 0u);
    STAMP(3);
  };
  if (wave >= n_rows) return;
  // DEPTH units in flight per wave: while the units of this chunk are finished, the loads of the next chunk (same row
  // or the wave's next row) are issued into the registers they free.  Every trip issues the same loads and stores
  // (units past the end of a row or of the batch read valid memory and their stores are dropped), so the waits between
  // them are exact counts.  The sched_barriers keep the compiler from sinking the refill loads below the next unit's
  // MFMAs (which would expose their latency again).
#ifndef GDM_C1_DEPTH
#define GDM_C1_DEPTH 4
#endif
  constexpr int DEPTH = GDM_C1_DEPTH;
  Row rc;
  float xv[DEPTH][4];
  rc.ph = wave % H1; rc.b = wave / H1;
  set_row(rc);
  int seg0 = 0;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(rc, d, xv[d]);
  while (rc.valid) {
    Row rn = rc;
    int seg0n = seg0 + DEPTH;
    if (seg0n >= upr) {                         // the wave's next row
      seg0n = 0;
      rn.ph += dph; rn.b += db;
      if (rn.ph >= H1) { rn.ph -= H1; ++rn.b; }
      set_row(rn);
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      finish(rc, seg0 + d, xv[d]);
      load(rn, seg0n + d, xv[d]);
      STAMP(4);
      __builtin_amdgcn_sched_barrier(0);
    }
    rc = rn;
    seg0 = seg0n;
  }
  STAMP_FLUSH;
}

// =====================================================================================================================
// conv1 backward (weights): dW1[c][kh][kw] = sum live * dp1[c] * x[2ph+dy-1+kh][2pw+dx-1+kw], db1[c] = sum live*dp1[c]
// Two-stage fixed-order reduction: per-workgroup slab of 80 floats, then a 1-block final sum.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void conv1_bwd_weight_kernel(const T* __restrict__ dp1,
                                                               const uint16_t* __restrict__ code1,
                                                               const float* __restrict__ x, int B, int H, int W,
                                                               int H1, int W1, float* __restrict__ slabs) {
  __shared__ float red[4][80];
  float acc[80];
#pragma unroll
  for (int i = 0; i < 80; ++i) acc[i] = 0.f;
  const int64_t total = (int64_t)B * H1 * W1;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int pw = (int)(idx % W1);
    const int ph = (int)((idx / W1) % H1);
    const int b = (int)(idx / ((int64_t)W1 * H1));
    const float* xb = x + (int64_t)b * H * W;
    float in[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ih = 2 * ph - 1 + r;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int iw = 2 * pw - 1 + s;
        in[r][s] = (ih >= 0 && ih < H && iw >= 0 && iw < W) ? xb[(int64_t)ih * W + iw] : 0.f;
      }
    }
    uint32_t fields[4];                                                         // code1 format: see conv1_fwd_kernel
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) fields[g4] = code1[code1_field((uint32_t)(b * H1 + ph), (W1 + 3) >> 2, pw, g4)];
    const T* g16 = dp1 + idx * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const uint32_t nib = fields[c >> 2] >> (4 * (c & 3));
      const bool live = (nib >> 2) & 1;
      const float g = live ? to_f32(g16[c]) : 0.f;
      const int pos = (int)(nib & 3);
      const bool dy = pos >> 1, dx = pos & 1;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int kw = 0; kw < 2; ++kw) {
          const float a = dx ? in[kh][kw + 1] : in[kh][kw];
          const float bsel = dx ? in[kh + 1][kw + 1] : in[kh + 1][kw];
          acc[c * 4 + kh * 2 + kw] = fmaf(g, dy ? bsel : a, acc[c * 4 + kh * 2 + kw]);
        }
      acc[64 + c] += g;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 80; ++i) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wv][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 80)
    slabs[(int64_t)blockIdx.x * 80 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// =====================================================================================================================
// conv1 backward (data): dx[i][j] = sum_{c,kh,kw} w[c][kh][kw] * dy[c][i+1-kh][j+1-kw], where dy is the sparse
// full-resolution gradient of the (H+1)x(W+1) conv output: dy[c][oh][ow] = dp1[oh/2][ow/2][c] if channel c of that
// pooled pixel is live and its argmax position is (oh&1, ow&1), else 0 (conv rows/columns beyond 2*H1 / 2*W1 were
// dropped by the floor pooling).  Not on the reference's training path (the discriminator's inputs are data or detached
// bridge outputs, SIMNN.py:283,299-306): this completes the module's autograd (aten::convolution_backward input grad,
// SIMNN.py:136).  One thread per input pixel; the <= 4 pooled pixels it touches are read straight from HBM/L2.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void conv1_bwd_data_kernel(const T* __restrict__ dp1,
                                                             const uint16_t* __restrict__ code1,
                                                             const float* __restrict__ w, int B, int H, int W, int H1,
                                                             int W1, float* __restrict__ dx) {
  __shared__ float ws[64];
  if (threadIdx.x < 64) ws[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const int64_t total = (int64_t)B * H * W;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx % W), i = (int)((idx / W) % H), b = (int)(idx / ((int64_t)W * H));
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        const int oh = i + 1 - kh, ow = j + 1 - kw;          // >= 0 always
        const int ph = oh >> 1, pw = ow >> 1;
        if (ph >= H1 || pw >= W1) continue;
        const int64_t pix = ((int64_t)b * H1 + ph) * W1 + pw;
        uint32_t fields[4];                                                       // code1 format: see conv1_fwd_kernel
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) fields[g4] = code1[code1_field((uint32_t)(b * H1 + ph), (W1 + 3) >> 2, pw, g4)];
        const uint32_t pos_here = (uint32_t)((oh & 1) * 2 + (ow & 1));
        const T* g16 = dp1 + pix * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const uint32_t nib = fields[c >> 2] >> (4 * (c & 3));
          const bool hit = ((nib >> 2) & 1u) && (nib & 3u) == pos_here;
          acc += hit ? ws[c * 4 + kh * 2 + kw] * to_f32(g16[c]) : 0.f;
        }
      }
    dx[idx] = acc;
  }
}

inline int conv1_slabs(int64_t total) {
  int64_t b = (total + 256 * 8 - 1) / (256 * 8);
  return (int)(b < 1 ? 1 : (b > cap::c1_slabs ? cap::c1_slabs : b));
}

}  // namespace

extern "C" int gdm_simnn_conv1_fwd_pair(const float* x0, const float* x1, int bsplit, const float* w, const float* bias,
                                        int B, int H, int W, void* p1, uint64_t* code1, int dtype, void* stream) {
  GDM_REQUIRE(x0 && w && bias && p1 && code1, "gdm_simnn_conv1_fwd: null pointer");
  GDM_REQUIRE(B > 0 && H >= 1 && W >= 1 && gdm_dtype_ok(dtype), "gdm_simnn_conv1_fwd: bad arguments");
  GDM_REQUIRE(bsplit >= 1 && bsplit <= B && (bsplit == B || x1 != nullptr), "gdm_simnn_conv1_fwd: second input pointer missing");
  const int H1 = (H + 1) / 2, W1 = (W + 1) / 2;
  GDM_REQUIRE((int64_t)B * H1 * W1 * 64 < ((int64_t)1 << 31) && (int64_t)B * H * W * 4 < ((int64_t)1 << 31),
              "gdm_simnn_conv1_fwd: batch of %d %dx%d inputs exceeds 2 GiB per tensor", B, H, W);
  const int64_t n_rows = (int64_t)B * H1;                                // a wave walks whole pooled rows
  int64_t blocks = (n_rows + 3) / 4;                                     // 4 waves per workgroup
  if (blocks > cap::c1_fwd()) blocks = cap::c1_fwd();
  if (bsplit == B) x1 = x0;                                              // never read
  DISPATCH_T(dtype, hipLaunchKernelGGL(conv1_fwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                                       x0, x1, bsplit, w, bias, B, H, W, H1, W1, (int)n_rows, (T*)p1, (uint16_t*)code1));
  GDM_LAUNCH_OK("gdm_simnn_conv1_fwd");
  return GDM_OK;
}

extern "C" int gdm_simnn_conv1_fwd(const float* x, const float* w, const float* bias, int B, int H, int W, void* p1,
                                   uint64_t* code1, int dtype, void* stream) {
  return gdm_simnn_conv1_fwd_pair(x, nullptr, B, w, bias, B, H, W, p1, code1, dtype, stream);
}

extern "C" size_t gdm_simnn_conv1_bwd_weight_workspace_bytes(int B, int H, int W) {
  const int64_t total = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2);
  return (size_t)(conv1_slabs(total) + 65) * 80 * sizeof(float);
}

extern "C" int gdm_simnn_conv1_bwd_weight(const void* dp1, const uint64_t* code1, const float* x, int B, int H, int W,
                                          float* dw, float* db, int dtype, int accumulate, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  GDM_REQUIRE(dp1 && code1 && x && dw && db, "gdm_simnn_conv1_bwd_weight: null pointer");
  GDM_REQUIRE(B > 0 && H >= 1 && W >= 1 && gdm_dtype_ok(dtype), "gdm_simnn_conv1_bwd_weight: bad arguments");
  if (!workspace || workspace_bytes < gdm_simnn_conv1_bwd_weight_workspace_bytes(B, H, W)) {
    gdm_set_error("gdm_simnn_conv1_bwd_weight: workspace too small");
    return GDM_EWORKSPACE;
  }
  const int H1 = (H + 1) / 2, W1 = (W + 1) / 2;
  const int nslabs = conv1_slabs((int64_t)B * H1 * W1);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(conv1_bwd_weight_kernel<T>, dim3(nslabs), dim3(256), 0, s, (const T*)dp1,
                                       (const uint16_t*)code1, x, B, H, W, H1, W1, (float*)workspace));
  float* scratch = (float*)workspace + (size_t)nslabs * 80;
  gdm_launch_slab_sum(1, (const float*)workspace, nslabs, 80, scratch, dw, db, accumulate, s);
  GDM_LAUNCH_OK("gdm_simnn_conv1_bwd_weight");
  return GDM_OK;
}

extern "C" int gdm_simnn_conv1_bwd_data(const void* dp1, const uint64_t* code1, const float* w, int B, int H, int W,
                                        float* dx, int dtype, void* stream) {
  GDM_REQUIRE(dp1 && code1 && w && dx, "gdm_simnn_conv1_bwd_data: null pointer");
  GDM_REQUIRE(B > 0 && H >= 1 && W >= 1 && gdm_dtype_ok(dtype), "gdm_simnn_conv1_bwd_data: bad arguments");
  const int H1 = (H + 1) / 2, W1 = (W + 1) / 2;
  const int64_t total = (int64_t)B * H * W;
  int64_t blocks = (total + 255) / 256;
  if (blocks > cap::c1_bwd_data) blocks = cap::c1_bwd_data;
  DISPATCH_T(dtype, hipLaunchKernelGGL(conv1_bwd_data_kernel<T>, dim3((unsigned)blocks), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)dp1, (const uint16_t*)code1, w, B, H, W, H1, W1, dx));
  GDM_LAUNCH_OK("gdm_simnn_conv1_bwd_data");
  return GDM_OK;
}

GDM_STAMP_READER(conv1)
