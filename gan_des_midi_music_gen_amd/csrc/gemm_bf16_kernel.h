// The kernel template of the vectorised bf16-MFMA GEMM (gemm_bf16.hip has the description, the operand checks and the
// dispatch).  Its 36 instantiations -- TA x A layout x TB x B layout x 2 variants, and bf16 x bf16 with the K tile 32
// ring as well, each with four epilogue bodies -- are divided over gemm_bf16_kt{32,64}_{bf16,f32}a.hip by variant and A
// dtype and gemm_bf16_ring_kt{32,64}.hip: one translation unit with all of them took as long to compile as everything
// else in the library several times over.
#pragma once
#include <type_traits>
#include "buffer_ops.h"
#include "gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128, NT = 256;

// Lanes of one wave exchange data through LDS without a workgroup barrier (the wave-private epilogue scratch): the
// compiler reasons per thread and would otherwise move the scratch stores under the (per-lane) condition of the loads.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// K-major image swizzle: 16-byte piece p of row r sits at piece p ^ kswz(r).  Found by exhaustive search over the
// ds_read_b128 lane groups ({0-3,12-15,20-27}, ...): conflict-free for 16 consecutive rows at any row offset.
// activation with a compile-time selector (same formulas as apply_act)
template <int ACT> __device__ __forceinline__ float act_const(float v, float slope) {
  if constexpr (ACT == GDM_ACT_RELU) return v > 0.f ? v : 0.f;
  else if constexpr (ACT == GDM_ACT_LEAKY) return v > 0.f ? v : v * slope;
  else if constexpr (ACT == GDM_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
  else return v;
}

template <int KT> __device__ __forceinline__ int kswz(int row) { return KT == 64 ? ((row >> 1) & 7) : ((row >> 1) & 2); }
// R-major image swizzle: 16-element block b of k-row k sits at block b ^ rswz(k) (ds_read_b64_tr_b16 reads k-rows
// {q, 8+q} x 16 rows per 32-lane half: eight distinct blocks).
__device__ __forceinline__ int rswz(int k) { return (k & 3) | ((k >> 1) & 4); }

// One operand tile in flight: 16-byte chunks per lane.
template <typename T, int KT> struct Stage {
  static constexpr int N = 128 * KT * (int)sizeof(T) / 16 / NT;
  f32x4 v[N];
};

// Per-lane constants of an operand's staging pattern (the chunk -> (row, k) map never changes).
template <typename T, int KT> struct Lane {
  uint32_t off[Stage<T, KT>::N];     // byte offset of the chunk inside the tile at k0 = 0
  int kl[Stage<T, KT>::N];           // k of the chunk relative to the tile; -1: row outside the matrix
  int lds[Stage<T, KT>::N];          // element offset in the LDS image
};

template <typename T, int KT, bool KMAJ>
__device__ __forceinline__ void lane_init(Lane<T, KT>& ln, int64_t ld, int rows, int r0) {
  constexpr int EPC = 16 / sizeof(T);               // elements per 16-byte chunk
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < Stage<T, KT>::N; ++i) {
    const int c = t + NT * i;
    int rl, kl;
    if constexpr (KMAJ) {
      constexpr int CPR = KT / EPC;                 // chunks per row
      rl = c / CPR; kl = (c % CPR) * EPC;
      ln.off[i] = (uint32_t)(((int64_t)(r0 + rl) * ld + kl) * (int64_t)sizeof(T));
      ln.lds[i] = rl * KT + 8 * ((kl >> 3) ^ kswz<KT>(rl)) + (kl & 7);
    } else {
      constexpr int CPK = 128 / EPC;                // chunks per k-row
      kl = c / CPK; rl = (c % CPK) * EPC;
      ln.off[i] = (uint32_t)(((int64_t)kl * ld + r0 + rl) * (int64_t)sizeof(T));
      ln.lds[i] = kl * 128 + (rl ^ (16 * rswz(kl)));
    }
    ln.kl[i] = (r0 + rl < rows) ? kl : -1;          // rows % EPC == 0: a chunk is inside or outside as a whole
  }
}

// ---- global -> registers, tile origin k0 (chunks at or past kend, or in rows past the matrix, read zeros)
template <typename T, int KT, bool KMAJ>
__device__ __forceinline__ void stage_load(Stage<T, KT>& st, const Lane<T, KT>& ln, rsrc_t rs, int64_t ld, int k0,
                                           int kend) {
  const uint32_t kbytes = (uint32_t)((KMAJ ? (int64_t)k0 : (int64_t)k0 * ld) * (int64_t)sizeof(T));
#pragma unroll
  for (int i = 0; i < Stage<T, KT>::N; ++i) {
    const bool ok = ln.kl[i] >= 0 && k0 + ln.kl[i] < kend;
    st.v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? kbytes + ln.off[i] : BUF_OOB, 0, 0));
  }
}

// ---- registers -> LDS image (bf16)
template <typename T, int KT>
__device__ __forceinline__ void stage_store(const Stage<T, KT>& st, const Lane<T, KT>& ln, __bf16* __restrict__ img) {
#pragma unroll
  for (int i = 0; i < Stage<T, KT>::N; ++i) {
    if constexpr (sizeof(T) == 2) {
      *(f32x4*)(img + ln.lds[i]) = st.v[i];
    } else {
      bf16x4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = (__bf16)st.v[i][e];
      *(bf16x4*)(img + ln.lds[i]) = h;
    }
  }
}

// fragment of rows [row0, row0+16) for MFMA k-step kk (32 k) of the tile
template <int KT, bool KMAJ>
__device__ __forceinline__ bf16x8 frag_read(const __bf16* __restrict__ img, int row0, int kk, int lr, int lg) {
  if constexpr (KMAJ) {
    const int row = row0 + lr;
    return *(const bf16x8*)&img[row * KT + 8 * ((4 * kk + lg) ^ kswz<KT>(row))];
  } else {
    const int q = lr >> 2, p = lr & 3;
    const int kr = 32 * kk + 8 * lg + q;
    const int n = (row0 + 4 * p) ^ (16 * (q | (4 * (lg & 1))));     // = rswz(kr) = rswz(kr + 4)
    const bf16x4 lo = lds_tr16(&img[kr * 128 + n]);
    const bf16x4 hi = lds_tr16(&img[(kr + 4) * 128 + n]);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

// KT 64: two LDS buffers (64 KB), one barrier per tile, for products with few workgroups per CU (long K, split-K).
// KT 32: one LDS buffer (16 KB), two barriers per tile, for products with many short workgroups.
// RING = register stages = tiles fetched ahead; the LDS layout does not depend on it.  The k loop is unrolled over
// the ring (and the LDS buffers), so every stage has fixed registers and a fixed place: stage s of tile t goes to
// LDS and is reloaded behind the barrier for tile t + RING, and its store waits for ITS loads only -- the RING - 1
// younger stages stay in flight.  That count holds only while the loads are issued in stage order; PIN fences the
// scheduler (sched_barrier) behind each stage's loads, in the prologue and in the loop: without it the scheduler
// issues the prologue's stages out of order, the wait-count pass falls back to vmcnt(0) in the loop (RING 2 then
// fetches ONE tile ahead), and the reload sinks under the tile's MFMAs.  The waits stay the compiler's own.
// (KT, RING, PIN) = (64, 2, false) and (32, 1, false) are the instances with an fp32 operand, as they always were;
// bf16 x bf16 runs (64, 2, true) and (32, 2, true) -- deeper rings measured slower (DESIGN.md sections 5 and 8).
template <typename TA, bool A_KMAJ, typename TB, bool B_KMAJ, int KT, int RING, bool PIN>
__global__ __launch_bounds__(NT) void gemm_bf16_fast(GemmArgs g) {
  constexpr int IMG = 128 * KT;                                         // elements of one operand image
  constexpr int NBUF = KT == 64 ? 2 : 1;                                // LDS buffers
  constexpr int UNROLL = RING % NBUF == 0 ? RING : RING * NBUF;         // tiles per trip: every (stage, buffer) pairing
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * NBUF * IMG];     // [buffer][A | B]
  const int t = threadIdx.x, l = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int lr = l & 15, lg = l >> 4;
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with its own L2), so the MT row tiles
  // that stream the SAME B panel (n tile, k slice) are given ids 8 apart -> they run on one XCD and share its L2.
  const int MT = (g.M + BM - 1) / BM, NTl = (g.N + BN - 1) / BN;
  const int id = blockIdx.x;
  const int grp = id / (8 * MT), within = id % (8 * MT);
  const int outer = grp * 8 + (within & 7), mt = within >> 3;
  if (outer >= NTl * g.split_k) return;
  const int nt = outer % NTl, zs = outer / NTl;
  const int m0 = mt * BM, n0 = nt * BN;
  // split-K slices are INTERLEAVED k tiles (slice z takes tiles z, z + split_k, ...), not contiguous ranges: the
  // workgroups of one output tile run side by side, so together they sweep each operand row contiguously and a DRAM
  // page is used up while it is open (with contiguous slices every workgroup pulls 128-byte pieces from pages of its
  // own, 128 KB apart per row).  The slab sum is the same set of products in a different, still fixed, order.
  const int kstep = KT * g.split_k;
  const int kbeg = zs * KT;
  const int kend = g.K;
  const int64_t lda = A_KMAJ ? g.sam : g.sak;
  const int64_t ldb = B_KMAJ ? g.sbn : g.sbk;
  // whole-operand descriptors (sizes checked < 2 GiB on the host)
  const rsrc_t ra = make_rsrc(g.A, (uint32_t)((A_KMAJ ? (int64_t)(g.M - 1) * lda + g.K : (int64_t)(g.K - 1) * lda + g.M) *
                                             (int64_t)sizeof(TA)));
  const rsrc_t rb = make_rsrc(g.B, (uint32_t)((B_KMAJ ? (int64_t)(g.N - 1) * ldb + g.K : (int64_t)(g.K - 1) * ldb + g.N) *
                                             (int64_t)sizeof(TB)));
  Lane<TA, KT> la;
  Lane<TB, KT> lb;
  lane_init<TA, KT, A_KMAJ>(la, lda, g.M, m0);
  lane_init<TB, KT, B_KMAJ>(lb, ldb, g.N, n0);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto multiply = [&](const __bf16* As, const __bf16* Bs) {
#pragma unroll
    for (int kk = 0; kk < KT / 32; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = frag_read<KT, A_KMAJ>(As, wm * 64 + 16 * i, kk, lr, lg);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = frag_read<KT, B_KMAJ>(Bs, wn * 64 + 16 * j, kk, lr, lg);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(b[j], a[i], acc[i][j]);   // D^T: lane -> (m = lr, n = 4*lg + r)
    }
  };
  Stage<TA, KT> sa[RING];
  Stage<TB, KT> sb[RING];
  auto pin = [] {
    if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll
  for (int r = 0; r < RING; ++r) {
    stage_load<TA, KT, A_KMAJ>(sa[r], la, ra, lda, kbeg + r * kstep, kend);
    stage_load<TB, KT, B_KMAJ>(sb[r], lb, rb, ldb, kbeg + r * kstep, kend);
    pin();
  }
  // tiles are taken UNROLL at a time; the tiles of the last trip at or past kend are zeros and are multiplied in
  for (int k0 = kbeg; k0 < kend; k0 += UNROLL * kstep) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      Stage<TA, KT>& xa = sa[u % RING];
      Stage<TB, KT>& xb = sb[u % RING];
      __bf16* As = smem + 2 * IMG * (u % NBUF);
      __bf16* Bs = As + IMG;
      if constexpr (NBUF == 1) __syncthreads();  // previous tile's fragment reads are done
      stage_store<TA, KT>(xa, la, As);           // waits for THIS stage's loads only: the other stages' were issued later
      stage_store<TB, KT>(xb, lb, Bs);
      __syncthreads();                           // (two buffers: the other one is what laggards still read)
      stage_load<TA, KT, A_KMAJ>(xa, la, ra, lda, k0 + (u + RING) * kstep, kend);   // always issued (zeros past kend)
      stage_load<TB, KT, B_KMAJ>(xb, lb, rb, ldb, k0 + (u + RING) * kstep, kend);
      pin();
      multiply(As, Bs);
    }
  }

  // ---- epilogue.  The activation is a compile-time constant of the (four) epilogue bodies: a run-time switch per
  //      element costs more instructions than the whole K loop of a short product.
  auto epilogue = [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    const bool vec_ok = (g.N % 4 == 0);
    if (g.split_k > 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + 16 * i + lr;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wn * 64 + 16 * j + 4 * lg;
          if (n >= g.N) continue;
          float* dst = g.ws + ((int64_t)zs * g.M + m) * g.N + n;
#ifndef GDM_GEMM_DEFAULT_STORES
          // (outputs and split-K slabs are consumed by a later kernel: non-temporal, like the activation streams of
          //  simnn_trunk.h (GDM_ACT_STORE_AUX) -- 0.7 % per iteration in same-box A/B)
          if (vec_ok) __builtin_nontemporal_store(acc[i][j], (f32x4*)dst);
#else
          if (vec_ok) *(f32x4*)dst = acc[i][j];
#endif
          else
            for (int r = 0; r < 4 && n + r < g.N; ++r) dst[r] = acc[i][j][r];
        }
      }
      return;
    }
    if (vec_ok && m0 + BM <= g.M && n0 + BN <= g.N &&
        (g.c_dtype != GDM_BF16 || (g.scm % 8 == 0 && ((uintptr_t)g.C & 15) == 0))) {
      // Interior tile: turn the accumulator layout (a lane owns 4 consecutive n of ONE row: 16 rows x 64 bytes per
      // store) into row-contiguous stores through a wave-private 16 x 64 fp32 LDS scratch (XOR-swizzled by the row):
      // one store instruction writes 4 rows x 256 bytes (fp32 C) or 8 rows x 128 bytes (bf16 C).
      __syncthreads();                                   // every wave is done reading the operand images
      float* scr = (float*)smem + w * (16 * 64);
      const bool is_bf16 = g.c_dtype == GDM_BF16;
      // this lane's (row, column) inside a 16 x 64 pass, and its bias vectors
      const int prow = is_bf16 ? (l >> 3) : (l >> 4), pcol = is_bf16 ? 8 * (l & 7) : 4 * (l & 15);
      const int nn = n0 + wn * 64 + pcol;
      f32x4 bn0 = {0.f, 0.f, 0.f, 0.f}, bn1 = bn0;
      if (g.bias_n) {
        bn0 = *(const f32x4*)(g.bias_n + nn);
        if (is_bf16) bn1 = *(const f32x4*)(g.bias_n + nn + 4);
      }
      const bool has_bias = g.bias_n || g.bias_m;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wave_lds_sync();                     // the previous pass's scratch reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)&scr[lr * 64 + 4 * ((4 * j + lg) ^ lr)] = acc[i][j];
        wave_lds_sync();
        if (is_bf16) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int row = 8 * h + prow, c8 = l & 7;
            f32x4 v0 = *(const f32x4*)&scr[row * 64 + 4 * ((2 * c8) ^ row)];
            f32x4 v1 = *(const f32x4*)&scr[row * 64 + 4 * ((2 * c8 + 1) ^ row)];
            const int m = m0 + wm * 64 + 16 * i + row;
            if (has_bias) {
              const float bm = g.bias_m ? g.bias_m[m] : 0.f;
              v0 += bn0 + (f32x4){bm, bm, bm, bm};
              v1 += bn1 + (f32x4){bm, bm, bm, bm};
            }
            bf16x8 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              hv[r] = (__bf16)act_const<ACT>(v0[r], g.slope);
              hv[4 + r] = (__bf16)act_const<ACT>(v1[r], g.slope);
            }
#ifndef GDM_GEMM_DEFAULT_STORES
            __builtin_nontemporal_store(hv, (bf16x8*)((__bf16*)g.C + (int64_t)m * g.scm + nn));
#else
            *(bf16x8*)((__bf16*)g.C + (int64_t)m * g.scm + nn) = hv;
#endif
          }
        } else {
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const int row = 4 * h + prow, pc = l & 15;
            f32x4 v = *(const f32x4*)&scr[row * 64 + 4 * (pc ^ row)];
            const int m = m0 + wm * 64 + 16 * i + row;
            if (has_bias) {
              const float bm = g.bias_m ? g.bias_m[m] : 0.f;
              v += bn0 + (f32x4){bm, bm, bm, bm};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = act_const<ACT>(v[r], g.slope);
#ifndef GDM_GEMM_DEFAULT_STORES
            __builtin_nontemporal_store(v, (f32x4*)((float*)g.C + (int64_t)m * g.scm + nn));
#else
            *(f32x4*)((float*)g.C + (int64_t)m * g.scm + nn) = v;
#endif
          }
        }
      }
      return;
    }
    // edge tiles / odd N
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + 16 * i + lr;
      if (m >= g.M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + 4 * lg;
        if (n >= g.N) continue;
        f32x4 v = acc[i][j];
        for (int r = 0; r < 4 && n + r < g.N; ++r) {
          float y = v[r];
          if (g.bias_n) y += g.bias_n[n + r];
          if (g.bias_m) y += g.bias_m[m];
          store_from_f32(g.C, g.c_dtype, (int64_t)m * g.scm + n + r, act_const<ACT>(y, g.slope));
        }
      }
    }
  };
  switch (g.act) {
    case GDM_ACT_RELU: epilogue(std::integral_constant<int, GDM_ACT_RELU>{}); break;
    case GDM_ACT_LEAKY: epilogue(std::integral_constant<int, GDM_ACT_LEAKY>{}); break;
    case GDM_ACT_SIGMOID: epilogue(std::integral_constant<int, GDM_ACT_SIGMOID>{}); break;
    default: epilogue(std::integral_constant<int, GDM_ACT_NONE>{}); break;
  }
}

// the four layout instantiations of one variant (KT, RING, PIN) and operand type pair
template <typename TA, typename TB, int KT, int RING, bool PIN>
void launch_layouts(const GemmArgs& g, bool a_kmaj, bool b_kmaj, dim3 grid, hipStream_t s) {
  if (a_kmaj) {
    if (b_kmaj) hipLaunchKernelGGL((gemm_bf16_fast<TA, true, TB, true, KT, RING, PIN>), grid, dim3(NT), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16_fast<TA, true, TB, false, KT, RING, PIN>), grid, dim3(NT), 0, s, g);
  } else {
    if (b_kmaj) hipLaunchKernelGGL((gemm_bf16_fast<TA, false, TB, true, KT, RING, PIN>), grid, dim3(NT), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16_fast<TA, false, TB, false, KT, RING, PIN>), grid, dim3(NT), 0, s, g);
  }
}

}  // namespace
