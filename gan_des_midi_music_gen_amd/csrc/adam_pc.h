// Adam with on-the-fly transposition for a parameter whose gradient / operand copy live in the (N, P, C) layout
// (model 1's fc1.weight): the tile body shared by pointwise.hip's stand-alone kernel and simnn_adam.hip's one-launch
// optimizer step.
#pragma once
#include "gdm_common.h"

// derived terms of step `step` in double, like torch computes them on the host: lr / (1 - beta1^t), sqrt(1 - beta2^t)
__device__ __forceinline__ void adam_derived(const float* hyper, int step, float& step_size, float& bc2_sqrt) {
  const double b1 = (double)hyper[2], b2 = (double)hyper[3];
  step_size = (float)((double)hyper[1] / (1.0 - pow(b1, (double)step)));
  bc2_sqrt = (float)sqrt(1.0 - pow(b2, (double)step));
}

// One (128 p x 32 c) tile of row n of an (N, C, P) parameter (gdm_adam_step_dev_pc, gdm_simnn_adam_step), in two parts
// with a workgroup barrier between them (the caller's): the gather of the gradient tile and the first p / m / v loads
// need nothing but addresses, so a caller that still waits for the step's bias-correction terms issues them first.
//
// `flags` (adam_pc_flags, host side): ADAM_PC_VEC = 16-byte accesses to p, m, v (a tile takes them when it is full both
// ways); ADAM_PC_WIDE = C == 32 and the gradient and the operand copy are 16-byte aligned: a tile that is full in p is
// then ONE contiguous run of 128 x 32 elements in both of them, moved with 16-byte accesses (four loads and two (bf16)
// or four (fp32) stores per thread instead of sixteen 4-byte loads and sixteen 2- or 4-byte stores).
//
// LDS image: element (c, p) of the tile is tile[c][p ^ (c & 28)], rows of 132 floats.  Banks (4-byte accesses: dword
// address mod 32, per 32-lane half; row c starts at bank 4 c mod 32):
//   wide gather / fp32 scatter   lane l holds c = 4 (l & 7) + e, p = 4 k + (l >> 3): bank = 16 (l & 1) + 4 e +
//                                4 (k ^ (l & 7)) + (l >> 3) mod 32.  (k ^ u) + 4 (u & 1) mod 8 takes every value once
//                                over u = l & 7 (even u keep the parity of k, odd u flip it), l >> 3 fills the two low
//                                bits: 32 lanes, 32 banks.  Without the XOR the eight u fall on two bank groups: 4-way.
//   bf16 scatter                 lane l holds c = 8 (l & 3) + e, p = 8 k + (l >> 2): bank = 4 e + (p ^ 8 (l & 3) ^
//                                (e & 4)) mod 32 -- bits 3, 4 separate the four l & 3, l >> 2 fills bits 0 .. 2:
//                                conflict-free.
//   the 16-byte row accesses     of the update see the 32 16-byte slots of a row permuted inside aligned groups of
//                                eight; every lane group of ds_read_b128 / ds_write_b128 still covers each bank once.
//   the scalar fallback          (lane = c, p fixed) stays 4-way, as it was without the XOR.
constexpr int ADAM_PC_VEC = 1, ADAM_PC_WIDE = 2;

static inline int adam_pc_flags(const float* p, const float* m, const float* v, const float* g_pc,
                                const void* shadow_pc, int C, int P) {
  const int vec = (P % 4 == 0) && ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const int wide = C == 32 && ((((uintptr_t)g_pc | (uintptr_t)shadow_pc) & 15) == 0);
  return (vec ? ADAM_PC_VEC : 0) | (wide ? ADAM_PC_WIDE : 0);
}

__device__ __forceinline__ f32x4 adam_pc_load4(const float* a) {
#ifndef GDM_ADAM_DEFAULT_POLICY       /* p, m, v are read once and written once per step: non-temporal */
  return __builtin_nontemporal_load((const f32x4*)a);
#else
  return *(const f32x4*)a;
#endif
}
__device__ __forceinline__ f32x4 adam_pc_load_g4(const float* a) {
#ifndef GDM_ADAM_G_DEFAULT_POLICY     /* the gradient is read once per step: non-temporal */
  return __builtin_nontemporal_load((const f32x4*)a);
#else
  return *(const f32x4*)a;
#endif
}
__device__ __forceinline__ void adam_pc_store4(f32x4 x, float* a) {
#ifndef GDM_ADAM_DEFAULT_POLICY       /* p, m, v are written once per step: non-temporal */
  __builtin_nontemporal_store(x, (f32x4*)a);
#else
  *(f32x4*)a = x;
#endif
}

// p, m, v of the tile's first group of rows (c = c0 + ty), in flight across the caller's barrier
struct AdamPcEarly { f32x4 p, m, v; };

__device__ __forceinline__ void adam_pc_gather(float (&tile)[32][132], const float* __restrict__ g_pc,
                                               const float* __restrict__ p, const float* __restrict__ m,
                                               const float* __restrict__ v, int C, int P, int flags, int bx, int by,
                                               int bz, AdamPcEarly& early) {
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int p0 = bx * 128, c0 = by * 32;
  const int64_t base = (int64_t)bz * C * P;
  const bool full = (flags & ADAM_PC_VEC) && p0 + 128 <= P && c0 + 32 <= C;
  const int64_t k0 = base + (int64_t)(c0 + ty) * P + p0 + 4 * tx;
  if ((flags & ADAM_PC_WIDE) && p0 + 128 <= P) {                     // C == 32: the tile is 4096 contiguous floats
    const float* src = g_pc + base + (int64_t)p0 * 32 + 4 * t;
    f32x4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = adam_pc_load_g4(src + 1024 * j);
    if (full) { early.p = adam_pc_load4(p + k0); early.m = adam_pc_load4(m + k0); early.v = adam_pc_load4(v + k0); }
    const int c4 = 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = ((t >> 3) + 32 * j) ^ c4;                      // (c4 + e) & 28 == c4
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[c4 + e][col] = g[j][e];
    }
    return;
  }
  float g[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {                                     // gradient tile, read along c
    const int pp = p0 + ty + 8 * i, c = c0 + tx;
    g[i] = (pp < P && c < C) ? g_pc[base + (int64_t)pp * C + c] : 0.f;
  }
  if (full) { early.p = adam_pc_load4(p + k0); early.m = adam_pc_load4(m + k0); early.v = adam_pc_load4(v + k0); }
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[tx][(ty + 8 * i) ^ (tx & 28)] = g[i];
}

// step_size / bc2_sqrt: the derived bias-correction terms of THIS step.
template <typename TS>
__device__ __forceinline__ void adam_pc_update(float (&tile)[32][132], float* __restrict__ p, float* __restrict__ m,
                                               float* __restrict__ v, int C, int P, TS* __restrict__ shadow_pc,
                                               const float* __restrict__ hyper, int flags, float step_size,
                                               float bc2_sqrt, int bx, int by, int bz, const AdamPcEarly& early) {
  const float w1 = 1.0f - hyper[2], beta2 = hyper[3], omb2 = 1.0f - hyper[3], eps = hyper[4], gscale = hyper[5];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int p0 = bx * 128, c0 = by * 32, n = bz;
  const int64_t base = (int64_t)n * C * P;
  const bool full = (flags & ADAM_PC_VEC) && p0 + 128 <= P && c0 + 32 <= C;      // 16-byte accesses to p, m, v
  if (full) {
    // Software pipeline over the four row groups: the loads of group i + 1 are in flight while group i is updated and
    // stored (group 0's were issued with the gather), so a workgroup makes ONE dependent HBM round trip, not two.  All
    // twelve remaining vectors at once would need 48 more registers than the 64 that 8 workgroups per CU leave.
    f32x4 pv = early.p, mv = early.m, vv = early.v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                    // p, m, v along p: four elements per thread
      const int cl = ty + 8 * i;
      const int64_t k = base + (int64_t)(c0 + cl) * P + p0 + 4 * tx;
      f32x4 pn, mn, vn;
      if (i < 3) {
        const int64_t kn = k + (int64_t)8 * P;
        pn = adam_pc_load4(p + kn); mn = adam_pc_load4(m + kn); vn = adam_pc_load4(v + kn);
      }
      float* trow = &tile[cl][(4 * tx) ^ (cl & 28)];
      const f32x4 gg = *(const f32x4*)trow;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pj = pv[e], mj = mv[e], vj = vv[e];
        adam_element(pj, mj, vj, gg[e], gscale, w1, beta2, omb2, eps, step_size, bc2_sqrt);
        pv[e] = pj; mv[e] = mj; vv[e] = vj;
      }
      adam_pc_store4(pv, p + k); adam_pc_store4(mv, m + k); adam_pc_store4(vv, v + k);
      *(f32x4*)trow = pv;                                            // the elements this thread read: no hazard
      if (i < 3) { pv = pn; mv = mn; vv = vn; }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cl = ty + 8 * i, c = c0 + cl, pp = p0 + 4 * tx;
      const int64_t k = base + (int64_t)c * P + pp;
      float* trow = &tile[cl][(4 * tx) ^ (cl & 28)];
      f32x4 gg = *(const f32x4*)trow, pv, mv, vv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = c < C && pp + e < P;
        pv[e] = ok ? p[k + e] : 0.f; mv[e] = ok ? m[k + e] : 0.f; vv[e] = ok ? v[k + e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pj = pv[e], mj = mv[e], vj = vv[e];
        adam_element(pj, mj, vj, gg[e], gscale, w1, beta2, omb2, eps, step_size, bc2_sqrt);
        pv[e] = pj; mv[e] = mj; vv[e] = vj;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c < C && pp + e < P) { p[k + e] = pv[e]; m[k + e] = mv[e]; v[k + e] = vv[e]; }
      *(f32x4*)trow = pv;
    }
  }
  __syncthreads();
  if ((flags & ADAM_PC_WIDE) && p0 + 128 <= P) {                     // updated weight: one run, 16 bytes a store
    constexpr int E = 16 / (int)sizeof(TS), CG = 32 / E;              // elements per store, stores per pixel
    typedef TS ts_vec __attribute__((ext_vector_type(E)));
    ts_vec* dst = (ts_vec*)(shadow_pc + base + (int64_t)p0 * 32) + t;
    const int ce = E * (t % CG);
#pragma unroll
    for (int j = 0; j < 16 / E; ++j) {                               // 4096 / E stores over 256 threads
      const int pl = t / CG + (256 / CG) * j;
      ts_vec o;
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] = from_f32<TS>(tile[ce + e][pl ^ ((ce + e) & 28)]);
#ifndef GDM_ADAM_COPY_NONTEMPORAL     /* the next iteration's fc1 products read the copy: default policy */
      dst[256 * j] = o;
#else
      __builtin_nontemporal_store(o, dst + 256 * j);
#endif
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {                                     // updated weight, written along c
    const int pl = ty + 8 * i, pp = p0 + pl, c = c0 + tx;
    if (pp < P && c < C) shadow_pc[base + (int64_t)pp * C + c] = from_f32<TS>(tile[tx][pl ^ (tx & 28)]);
  }
}


template <typename TS>
__device__ __forceinline__ void adam_pc_tile(float (&tile)[32][132], float* __restrict__ p, const float* __restrict__ g_pc,
                                             float* __restrict__ m, float* __restrict__ v, int C, int P,
                                             TS* __restrict__ shadow_pc, const float* __restrict__ hyper, int flags,
                                             float step_size, float bc2_sqrt, int bx, int by, int bz) {
  AdamPcEarly early;
  adam_pc_gather(tile, g_pc, p, m, v, C, P, flags, bx, by, bz, early);
  __syncthreads();
  adam_pc_update<TS>(tile, p, m, v, C, P, shadow_pc, hyper, flags, step_size, bc2_sqrt, bx, by, bz, early);
}
