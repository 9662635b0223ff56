// Both generators of model 2 in eval mode, one launch for any batch: cat(noise, input) -> 4 x [Linear, BatchNorm1d on
// the running statistics, Sigmoid] (MMGAN_MIDI_DES/network_tests.py:58-123; generate_midi, :199-206).  The sibling of
// simnn_gen.hip's gen_eval_kernel for model 2 and of linear_bn.hip's block kernel, whose rounding points it keeps.
//
// In eval mode BatchNorm is a per-column affine map, so batch rows are independent.  A 256-thread workgroup owns a
// tile of GE_R = 16 rows (one MFMA row tile) and one slab of layer 4's columns: it stages cat(noise, input) into LDS
// from the two pointers (the second one with a row stride, 0 = one vector for every row; K tail zero-filled), runs
// layers 1-3 entirely in LDS (fp32 activations, ping-pong between two buffers) and then its slab of layer 4 straight
// from registers to global memory.  Layers 1-3 are recomputed by every slab of a row tile: they are a fifth of the
// arithmetic at N4 = 4096, and the host picks the fewest slabs that give the chip one workgroup per CU, so at large B
// there is one slab and nothing is recomputed.  The slab partition only decides WHICH workgroup computes a column,
// never how: a row's bits depend on neither B, the row's position nor the slab count.
//
// Arithmetic per layer, as linear_bn_act_kernel in eval mode: operands split x = xh + xl, W = wh + wl in bf16
// (activations when their fragment is read from LDS, weights once in the pack), acc += xl wh + xh wl + xh wh on
// v_mfma_f32_16x16x32_bf16 in k order, + bias, (y - running_mean) * (invstd * gamma) + beta, 1 / (1 + expf(-v)), all
// fp32.  Weights are read from the pack in fragment order (a wave's 64 lanes read 1 KiB contiguous per fragment);
// they are L2-resident after the first workgroup (<= 0.9 MiB per generator).
// Nothing is written but `out` and, in the TAPS instance, the taps.  No atomics.
#include "gdm_common.h"

namespace {

constexpr int GE_R = 16;                      // rows per workgroup
constexpr int GE_H1 = 256, GE_H2 = 128, GE_H3 = 64;
constexpr int GE_KMAX = 512;
constexpr int GE_N4MAX = 1 << 20;
constexpr int GE_SA = GE_KMAX + 4, GE_SB = GE_H1 + 4;   // LDS row strides in floats (16-byte aligned rows)
constexpr int GE_NVEC = 5;                    // bias | invstd | gamma | beta | running_mean, each Np floats

struct GeLayout {
  int K[4], N[4], Kp[4], Np[4];
  size_t w[4], v[4], total;                   // byte offsets of the weight image / vector block of each layer
};

__host__ __device__ inline GeLayout ge_layout(int k1, int n4) {
  GeLayout L;
  const int K[4] = {k1, GE_H1, GE_H2, GE_H3}, N[4] = {GE_H1, GE_H2, GE_H3, n4};
  size_t off = 0;
  for (int i = 0; i < 4; ++i) {
    L.K[i] = K[i];
    L.N[i] = N[i];
    L.Kp[i] = (K[i] + 31) / 32 * 32;
    L.Np[i] = (N[i] + 15) / 16 * 16;
    L.w[i] = off;
    off += (size_t)L.Np[i] * L.Kp[i] * 2 * sizeof(__bf16);      // hi and lo images
    L.v[i] = off;
    off += (size_t)L.Np[i] * GE_NVEC * sizeof(float);
  }
  L.total = off;
  return L;
}

inline bool ge_supported(int k1, int h1, int h2, int h3, int n4) {
  return k1 >= 1 && k1 <= GE_KMAX && h1 == GE_H1 && h2 == GE_H2 && h3 == GE_H3 && n4 >= 1 && n4 <= GE_N4MAX;
}

// ---- the pack: one launch per layer ------------------------------------------------------------------------------
// weight image: [column tile ct][k step ks][hi | lo][lane 0..63][8 bf16], lane (lr, lg) holding W[16 ct + lr][32 ks +
// 8 lg + j] -- the B fragment of v_mfma_f32_16x16x32_bf16; rows >= N and columns >= K are zero.
__global__ __launch_bounds__(256) void ge_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                      int N, int K, int Np, int Kp, float eps, __bf16* __restrict__ dw,
                                                      float* __restrict__ dv) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int KS = Kp / 32;
  if (e < (int64_t)Np * Kp) {
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    const int64_t frag = e >> 9;
    const int ct = (int)(frag / KS), ks = (int)(frag % KS);
    const int n = 16 * ct + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + j;
    const float v = (n < N && k < K) ? w[(int64_t)n * K + k] : 0.f;
    const __bf16 h = (__bf16)v;
    dw[(frag * 2 + 0) * 512 + lane * 8 + j] = h;
    dw[(frag * 2 + 1) * 512 + lane * 8 + j] = (__bf16)(v - (float)h);
  }
  if (e < Np) {
    const int n = (int)e;
    const bool in = n < N;
    dv[0 * Np + n] = in ? bias[n] : 0.f;
    dv[1 * Np + n] = in ? 1.0f / sqrtf(rvar[n] + eps) : 0.f;
    dv[2 * Np + n] = in ? gamma[n] : 0.f;
    dv[3 * Np + n] = in ? beta[n] : 0.f;
    dv[4 * Np + n] = in ? rmean[n] : 0.f;
  }
}

// ---- the forward ---------------------------------------------------------------------------------------------------
struct GeJob {
  const float* noise;
  const float* input;
  const char* pack;
  float* out;
  float* tap_y[4];
  float* tap_a[3];
  int B, z, in, input_stride, k1, n4;
  int slabs, slab_ct;        // column slabs of layer 4 per row tile; column tiles (of 16) per slab, a multiple of 4
};
struct GeJobs {
  GeJob j[2];
  int wgs0;                  // workgroups [0, wgs0) belong to job 0
};

__device__ __forceinline__ void ge_split8(const float* p, bf16x8& h, bf16x8& lo) {
  const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (__bf16)v0[e];
    lo[e] = (__bf16)(v0[e] - (float)h[e]);
    h[4 + e] = (__bf16)v1[e];
    lo[4 + e] = (__bf16)(v1[e] - (float)h[4 + e]);
  }
}

__device__ __forceinline__ f32x4 ge_mac(const bf16x8& ah, const bf16x8& al, const bf16x8* __restrict__ frag, int l,
                                        f32x4 acc) {
  const bf16x8 bh = frag[l], bl = frag[64 + l];
  acc = mfma16(al, bh, acc);             // small terms first, as linear_bn_act_kernel
  acc = mfma16(ah, bl, acc);
  return mfma16(ah, bh, acc);
}

// y = acc + bias; out = sigmoid((y - mean) * (invstd * gamma) + beta) for the 4 rows x 1 column this lane holds
__device__ __forceinline__ void ge_bn_sigmoid(const f32x4 acc, const float* __restrict__ vec, int Np, int n, float y[4],
                                              float o[4]) {
  const float b = vec[n], alpha = vec[Np + n] * vec[2 * Np + n], bt = vec[3 * Np + n], mean = vec[4 * Np + n];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    y[r] = acc[r] + b;
    o[r] = apply_act((y[r] - mean) * alpha + bt, GDM_ACT_SIGMOID, 0.f);
  }
}

// One hidden layer on the workgroup's 16 rows: in (LDS fp32, stride S_in, Kp columns) -> outb (LDS fp32, stride S_out,
// N = 64 NT columns).  Wave wv owns column tiles wv, wv + 4, ...
template <int NT, bool TAPS>
__device__ __forceinline__ void ge_hidden(const float* in, int S_in, int Kp, const char* __restrict__ pack, size_t w_off,
                                          size_t v_off, float* outb, int S_out, float* tap_y, float* tap_a, int row0,
                                          int B, bool tap_here) {
  constexpr int N = 64 * NT;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = l & 15, lg = l >> 4;
  const int KS = Kp / 32;
  const bf16x8* __restrict__ wf = (const bf16x8*)(pack + w_off);
  const float* __restrict__ vec = (const float*)(pack + v_off);
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < KS; ++ks) {
    bf16x8 ah, al;
    ge_split8(in + lr * S_in + 32 * ks + 8 * lg, ah, al);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = ge_mac(ah, al, wf + ((size_t)(wv + 4 * t) * KS + ks) * 128, l, acc[t]);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = 16 * (wv + 4 * t) + lr;
    float y[4], o[4];
    ge_bn_sigmoid(acc[t], vec, N, n, y, o);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * lg + r;
      outb[m * S_out + n] = o[r];
      if constexpr (TAPS) {
        if (tap_here && row0 + m < B) {
          if (tap_y) tap_y[(int64_t)(row0 + m) * N + n] = y[r];
          if (tap_a) tap_a[(int64_t)(row0 + m) * N + n] = o[r];
        }
      }
    }
  }
}

template <bool TAPS>
__global__ __launch_bounds__(256) void mmgan_gen_eval_kernel(const GeJobs jobs) {
  const int job = (int)blockIdx.x >= jobs.wgs0 ? 1 : 0;
  const GeJob& jb = jobs.j[job];
  const int wg = (int)blockIdx.x - (job ? jobs.wgs0 : 0);
  const int rt = wg / jb.slabs, slab = wg % jb.slabs;
  const int row0 = rt * GE_R, B = jb.B;
  const GeLayout L = ge_layout(jb.k1, jb.n4);
  __shared__ __attribute__((aligned(16))) float bufA[GE_R * GE_SA];     // x, then a2
  __shared__ __attribute__((aligned(16))) float bufB[GE_R * GE_SB];     // a1, then a3
  const int t = threadIdx.x, l = t & 63, wv = t >> 6, lr = l & 15, lg = l >> 4;

  // cat(noise, input) with the K tail and the rows past B zero-filled
  const int Kp1 = L.Kp[0];
  for (int i = t; i < GE_R * Kp1; i += 256) {
    const int r = i / Kp1, c = i - r * Kp1, row = row0 + r;
    float v = 0.f;
    if (row < B) {
      if (c < jb.z) v = jb.noise[(int64_t)row * jb.z + c];
      else if (c < jb.k1) v = jb.input[(int64_t)row * jb.input_stride + (c - jb.z)];
    }
    bufA[r * GE_SA + c] = v;
  }
  __syncthreads();
  const bool tap_here = slab == 0;
  ge_hidden<4, TAPS>(bufA, GE_SA, Kp1, jb.pack, L.w[0], L.v[0], bufB, GE_SB, jb.tap_y[0], jb.tap_a[0], row0, B, tap_here);
  __syncthreads();
  ge_hidden<2, TAPS>(bufB, GE_SB, GE_H1, jb.pack, L.w[1], L.v[1], bufA, GE_SA, jb.tap_y[1], jb.tap_a[1], row0, B, tap_here);
  __syncthreads();
  ge_hidden<1, TAPS>(bufA, GE_SA, GE_H2, jb.pack, L.w[2], L.v[2], bufB, GE_SB, jb.tap_y[2], jb.tap_a[2], row0, B, tap_here);
  __syncthreads();

  // layer 4: K = 64, two k steps; this workgroup's slab of column tiles, dealt to the waves round robin
  bf16x8 ah[2], al[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) ge_split8(bufB + lr * GE_SB + 32 * ks + 8 * lg, ah[ks], al[ks]);
  const bf16x8* __restrict__ wf = (const bf16x8*)(jb.pack + L.w[3]);
  const float* __restrict__ vec = (const float*)(jb.pack + L.v[3]);
  const int N4 = jb.n4, Np4 = L.Np[3], T4 = Np4 / 16;
  const int ct_end = min((slab + 1) * jb.slab_ct, T4);
  float* __restrict__ out = jb.out;
  for (int ct = slab * jb.slab_ct + wv; ct < ct_end; ct += 4) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) acc = ge_mac(ah[ks], al[ks], wf + ((size_t)ct * 2 + ks) * 128, l, acc);
    const int n = 16 * ct + lr;
    float y[4], o[4];
    ge_bn_sigmoid(acc, vec, Np4, n, y, o);
    if (n < N4) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * lg + r;
        if (row < B) {
          out[(int64_t)row * N4 + n] = o[r];
          if constexpr (TAPS) {
            if (jb.tap_y[3]) jb.tap_y[3][(int64_t)row * N4 + n] = y[r];
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int gdm_mmgan_gen_eval_supported(int k1, int h1, int h2, int h3, int n4) {
  return ge_supported(k1, h1, h2, h3, n4) ? 1 : 0;
}

extern "C" size_t gdm_mmgan_gen_eval_pack_bytes(int k1, int h1, int h2, int h3, int n4) {
  return ge_supported(k1, h1, h2, h3, n4) ? ge_layout(k1, n4).total : 0;
}

extern "C" int gdm_mmgan_gen_eval_pack(const float* const* w, const float* const* bias, const float* const* gamma,
                                       const float* const* beta, const float* const* running_mean,
                                       const float* const* running_var, int k1, int h1, int h2, int h3, int n4, float eps,
                                       void* pack, size_t pack_bytes, void* stream) {
  GDM_REQUIRE(ge_supported(k1, h1, h2, h3, n4),
              "gdm_mmgan_gen_eval_pack: geometry (%d -> %d -> %d -> %d -> %d) is not supported (1 <= K1 <= %d, hidden "
              "widths %d, %d, %d, 1 <= N4 <= %d)", k1, h1, h2, h3, n4, GE_KMAX, GE_H1, GE_H2, GE_H3, GE_N4MAX);
  GDM_REQUIRE(w && bias && gamma && beta && running_mean && running_var && pack, "gdm_mmgan_gen_eval_pack: null pointer");
  for (int i = 0; i < 4; ++i)
    GDM_REQUIRE(w[i] && bias[i] && gamma[i] && beta[i] && running_mean[i] && running_var[i],
                "gdm_mmgan_gen_eval_pack: null pointer in layer %d", i + 1);
  GDM_REQUIRE(eps >= 0.f, "gdm_mmgan_gen_eval_pack: eps < 0");
  const GeLayout L = ge_layout(k1, n4);
  GDM_REQUIRE(pack_bytes == L.total, "gdm_mmgan_gen_eval_pack: pack of %zu bytes, this geometry takes %zu", pack_bytes,
              L.total);
  GDM_REQUIRE(((uintptr_t)pack & 15) == 0, "gdm_mmgan_gen_eval_pack: the pack must be 16-byte aligned");
  for (int i = 0; i < 4; ++i) {
    const int64_t n = (int64_t)L.Np[i] * L.Kp[i];
    hipLaunchKernelGGL(ge_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w[i], bias[i],
                       gamma[i], beta[i], running_mean[i], running_var[i], L.N[i], L.K[i], L.Np[i], L.Kp[i], eps,
                       (__bf16*)((char*)pack + L.w[i]), (float*)((char*)pack + L.v[i]));
    GDM_LAUNCH_OK("gdm_mmgan_gen_eval_pack");
  }
  return GDM_OK;
}

extern "C" int gdm_mmgan_gen_eval(const gdm_mmgan_gen_eval_job* jobs, int n_jobs, int h1, int h2, int h3, void* stream) {
  GDM_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 2, "gdm_mmgan_gen_eval: 1 or 2 jobs per launch");
  GeJobs gj{};
  bool taps = false;
  int64_t wgs = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const gdm_mmgan_gen_eval_job& j = jobs[i];
    GDM_REQUIRE(j.B >= 1, "gdm_mmgan_gen_eval: job %d: batch %d < 1", i, j.B);
    GDM_REQUIRE(j.z >= 0 && j.in >= 0 && j.z <= GE_KMAX && j.in <= GE_KMAX, "gdm_mmgan_gen_eval: job %d: bad z / in", i);
    const int k1 = j.z + j.in;
    GDM_REQUIRE(ge_supported(k1, h1, h2, h3, j.n4),
                "gdm_mmgan_gen_eval: job %d: geometry (%d -> %d -> %d -> %d -> %d) is not supported (1 <= K1 <= %d, "
                "hidden widths %d, %d, %d, 1 <= N4 <= %d)", i, k1, h1, h2, h3, j.n4, GE_KMAX, GE_H1, GE_H2, GE_H3,
                GE_N4MAX);
    GDM_REQUIRE(j.pack && j.out && (j.z == 0 || j.noise) && (j.in == 0 || j.input), "gdm_mmgan_gen_eval: job %d: null pointer",
                i);
    GDM_REQUIRE(j.input_stride == 0 || j.input_stride >= j.in,
                "gdm_mmgan_gen_eval: job %d: input_stride %d is neither 0 (broadcast) nor >= in = %d", i, j.input_stride,
                j.in);
    const GeLayout L = ge_layout(k1, j.n4);
    GDM_REQUIRE(j.pack_bytes == L.total, "gdm_mmgan_gen_eval: job %d: pack of %zu bytes, this geometry takes %zu", i,
                j.pack_bytes, L.total);
    GDM_REQUIRE(((uintptr_t)j.pack & 15) == 0, "gdm_mmgan_gen_eval: job %d: the pack must be 16-byte aligned", i);
    GeJob& d = gj.j[i];
    d.noise = j.noise;
    d.input = j.input;
    d.pack = (const char*)j.pack;
    d.out = j.out;
    for (int q = 0; q < 4; ++q) { d.tap_y[q] = j.tap_y[q]; taps = taps || j.tap_y[q]; }
    for (int q = 0; q < 3; ++q) { d.tap_a[q] = j.tap_a[q]; taps = taps || j.tap_a[q]; }
    d.B = j.B; d.z = j.z; d.in = j.in; d.input_stride = j.input_stride; d.k1 = k1; d.n4 = j.n4;
    // the fewest column slabs that put about one workgroup on every CU (256): slab_ct column tiles each, 4 per wave round
    const int row_tiles = (j.B + GE_R - 1) / GE_R, T4 = L.Np[3] / 16;
    const int max_slabs = (T4 + 3) / 4;
    int slabs = (256 + row_tiles - 1) / row_tiles;
    slabs = slabs < 1 ? 1 : (slabs > max_slabs ? max_slabs : slabs);
    d.slab_ct = ((T4 + slabs - 1) / slabs + 3) / 4 * 4;
    d.slabs = (T4 + d.slab_ct - 1) / d.slab_ct;
    const int64_t n = (int64_t)row_tiles * d.slabs;
    if (i == 0) gj.wgs0 = (int)n;
    wgs += n;
  }
  GDM_REQUIRE(wgs <= 0x7fffffff, "gdm_mmgan_gen_eval: too many workgroups");
  if (n_jobs == 1) gj.wgs0 = (int)wgs;
  if (taps)
    hipLaunchKernelGGL(mmgan_gen_eval_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, gj);
  else
    hipLaunchKernelGGL(mmgan_gen_eval_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, gj);
  GDM_LAUNCH_OK("gdm_mmgan_gen_eval");
  return GDM_OK;
}
