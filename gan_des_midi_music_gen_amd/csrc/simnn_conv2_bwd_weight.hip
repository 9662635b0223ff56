// conv2 backward-weight of model 1's discriminator trunk (simnn_trunk.h).
#include "simnn_conv2_bwd.h"

namespace {

// -------------------------------------------------------------------------------------- conv2 backward (weights)
// dW2[o][ci][kh][kw] = sum_{b,r,c} dc2[r][c][o] * p1[r-1+kh][c-1+kw][ci];  db2[o] = sum dc2
// GEMM with M = 32 (o), N = 9 taps x 16 ci, K = pixels.  Like the data-gradient kernel, a persistent workgroup walks
// strips (image, 64-column tile) top to bottom in steps of 4 conv rows; wave w contracts row w of the step.  p1 lives
// in an 8-row LDS ring (a step needs rows 4rq-1 .. 4rq+4, only 4rq+1 .. 4rq+4 are new), dc2 rows are rebuilt per step
// from the two pooled rows they come from; the next step's rows are fetched into registers during the MFMAs.  bf16
// reads both operands with the transposing ds_read_b64_tr_b16 (the contraction index is the pixel, the LDS images are
// channel-contiguous); both images are swizzled by the column's bit 3 -- a half-wave's tr16 read touches columns
// {c..c+3} and {c+8..c+11}, which without it fall on the same banks (with it: none left, checked exhaustively).
// Accumulators (2 x 9 tiles per wave) live in registers across all steps, then waves are summed through LDS in fixed
// order and the workgroup writes one slab.

constexpr int BW_RING = 8;                    // p1 rows in the LDS ring
constexpr int BW_WPX = 72;                    // p1 columns per ring row (band columns 0..65, padded to a multiple of 8)
template <typename T> struct BW {
  static constexpr int P_ELEMS = BW_RING * BW_WPX * C2<T>::S16;
  static constexpr int DC_ELEMS = ROWS * COLS * C2<T>::S32;
  static constexpr int P1IT = 3;              // 16-byte chunks of the 4 new rows: 2 x 256 (columns c0..c0+63) + halo
  // column swizzles (bf16 only): band column c of the p1 ring, 16-byte channel group og of dc2 column c
  static __device__ __forceinline__ int pcol(int c) { return sizeof(T) == 2 ? (c ^ (4 * ((c >> 3) & 1))) : c; }
  static __device__ __forceinline__ int dcpiece(int og, int c) { return sizeof(T) == 2 ? (og ^ (2 * ((c >> 3) & 1))) : og; }
};

template <typename T>
__global__ __launch_bounds__(256) void conv2_bwd_weight_kernel(const T* __restrict__ dp2,
                                                               const uint8_t* __restrict__ code2,
                                                               const T* __restrict__ p1, int B, int H1, int W1,
                                                               int H2, int W2, int n_ctiles, int nseg, int seg_len,
                                                               int n_items, float* __restrict__ slabs) {
  constexpr int S16 = C2<T>::S16, S32 = C2<T>::S32, WPX = BW_WPX;
  constexpr int PIECES = 2, EPP = 8;          // a p1 pixel record is staged as two 8-channel halves (16 B bf16, 32 B fp32)
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  T* dc_s = (T*)dyn_smem;
  T* p_s = dc_s + BW<T>::DC_ELEMS;
  const unsigned char* tab_s = (const unsigned char*)(p_s + BW<T>::P_ELEMS);     // bf16: code2 selector tables
  const int t = threadIdx.x, l = t & 63, wv = t >> 6, lr = l & 15, lg = l >> 4;
  const int nrq = (H1 + ROWS - 1) / ROWS, G = gridDim.x;
  f32x4 acc[2][9];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < 9; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bsum[e] = 0.f;

  const rsrc_t dp2r = make_rsrc(dp2, (uint32_t)B * H2 * W2 * 32 * sizeof(T));
  const rsrc_t code2r = make_rsrc(code2, (uint32_t)B * H2 * W2 * 16);
  const rsrc_t p1r = make_rsrc(p1, (uint32_t)B * H1 * W1 * 16 * sizeof(T));

  // ---- per-lane staging constants
  // dc2: lane = (pooled pixel item = t >> 2 of the 2 x 32 pooled block, 8-channel group og)
  const int og = t & 3, dprow = (t >> 2) >> 5, dpcol = (t >> 2) & 31;
  const uint32_t dc_goff = (uint32_t)(dprow * W2 + dpcol) * 32 + 8 * og;
  // p1: chunk k -> (new row 0..3, band column 0..65, piece); chunks 0..511 cover band columns 1..64, 512..527 the halo
  int pr_row[BW<T>::P1IT], pr_col[BW<T>::P1IT], pr_lds[BW<T>::P1IT];
  uint32_t pr_goff[BW<T>::P1IT];
#pragma unroll
  for (int k = 0; k < BW<T>::P1IT; ++k) {
    const int i = t + 256 * k;
    int row, col, piece;
    if (k < 2) {                                  // 4 rows x 64 columns x 2 halves = 512 chunks
      piece = i % PIECES; col = 1 + (i / PIECES) % 64; row = i / (PIECES * 64);
    } else {
      const int j = i - 512;                      // halo columns 0 and 65
      piece = j % PIECES; col = ((j / PIECES) & 1) ? 65 : 0; row = j / (2 * PIECES);
    }
    const bool has = row < 4;
    pr_row[k] = has ? row : 99;
    pr_col[k] = col;
    pr_goff[k] = (uint32_t)((row * W1 + col) * 16 + piece * EPP) * (uint32_t)sizeof(T);
    pr_lds[k] = BW<T>::pcol(col) * S16 + piece * EPP;       // + slot * WPX * S16
  }

  struct Regs {
    f32x4 g[sizeof(T) == 2 ? 1 : 2];
    uint32_t cd;
    f32x4 p[(sizeof(T) == 2 ? 1 : 2) * BW<T>::P1IT];
  } rg;
  auto issue = [&](int b, int c0, int rq, bool with_dc) {
    {   // dc2: pooled rows 2rq, 2rq+1, pooled columns c0/2 .. c0/2+31
      const int pr = 2 * rq + dprow, pc = (c0 >> 1) + dpcol;
      const bool ok = with_dc && pr >= 0 && pr < H2 && pc < W2;
      const uint32_t gi = (uint32_t)b * H2 * W2 * 32 + (uint32_t)(2 * rq * W2 + (c0 >> 1)) * 32 + dc_goff;
      rg.cd = __builtin_bit_cast(uint32_t, buf_load4(code2r, ok ? gi >> 1 : BUF_OOB));
      rg.g[0] = buf_load16(dp2r, ok ? gi * (uint32_t)sizeof(T) : BUF_OOB);
      if constexpr (sizeof(T) == 4) rg.g[1] = buf_load16(dp2r, ok ? gi * 4u + 16u : BUF_OOB);
    }
    // p1: rows 4rq+1 .. 4rq+4, band columns 0..65 = image columns c0-1 .. c0+64
    const int r0 = ROWS * rq + 1, cc0 = c0 - 1;
    const uint32_t base = (uint32_t)((b * H1 + r0) * W1 + cc0) * 16 * (uint32_t)sizeof(T);
#pragma unroll
    for (int k = 0; k < BW<T>::P1IT; ++k) {
      const bool ok = (unsigned)(r0 + pr_row[k]) < (unsigned)H1 && (unsigned)(cc0 + pr_col[k]) < (unsigned)W1;
      rg.p[k] = buf_load16(p1r, ok ? base + pr_goff[k] : BUF_OOB);
      if constexpr (sizeof(T) == 4) {
        // fp32: a half record is 32 bytes -> second 16 bytes
        rg.p[BW<T>::P1IT + k] = buf_load16(p1r, ok ? base + pr_goff[k] + 16u : BUF_OOB);
      }
    }
  };

  auto place = [&](int s_, int& b_, int& c0_, int& rq_first, int& rq_end) {
    const int ct = s_ % n_ctiles, sg = (s_ / n_ctiles) % nseg;
    b_ = s_ / (n_ctiles * nseg);
    c0_ = ct * COLS;
    rq_first = sg * seg_len;
    rq_end = min(rq_first + seg_len, nrq);
  };
  int s = blockIdx.x, b, c0, rq_first, rq_end;            // host guarantees gridDim.x <= n_items
  place(s, b, c0, rq_first, rq_end);
  int rq = rq_first - 1;                                   // pseudo step: brings in p1 rows 4 rq_first - 1 and 4 rq_first
  STAMP_DECL;
  issue(b, c0, rq, false);
  STAMP(4);
  // (LDS-only set-up behind the first loads; first barrier: in the loop)
  if constexpr (sizeof(T) == 2) code2_tables_init((uint32_t*)(p_s + BW<T>::P_ELEMS));

  // per-lane fragment addresses that never change: swizzled p1 band columns for (segment, kw, lo/hi)
  int pcol_off[2][3][2];
  const int q = lr >> 2, p4 = lr & 3;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int sg2 = 0; sg2 < 2; ++sg2)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
          pcol_off[sg2][kw][hi] = BW<T>::pcol(32 * sg2 + 8 * lg + kw + q + 4 * hi) * S16 + 4 * p4;
  }

  while (s < n_items) {
#ifdef GDM_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(5);
#endif
    // ---- registers -> LDS: dc2 rows of this step, p1 ring rows 4rq+1 .. 4rq+4
    if (rq >= rq_first) {
      const uint32_t cd = rg.cd;
      if constexpr (sizeof(T) == 2) {
        const u32x4 gv = __builtin_bit_cast(u32x4, rg.g[0]);
        uint32_t ex[4][4];                                   // [channel pair][position]
        const int odd = dpcol & 1;                           // odd pooled column: columns swapped (see Code2 tables)
        const unsigned char* tab_l = tab_s + (odd ? C2T_SWAP : 0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t off8 = (cd >> (8 * w)) & 0xffu;
          code2_expand_pair(tab_l, off8, gv[w], ex[w]);
          // bias gradient: channels whose pooled value was live
          const uint32_t g = __builtin_amdgcn_perm(0u, gv[w], *(const uint32_t*)(tab_s + C2T_C + off8));
          bsum[2 * w] += __builtin_bit_cast(float, g << 16);
          bsum[2 * w + 1] += __builtin_bit_cast(float, g & 0xffff0000u);
        }
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int col = 2 * dpcol + (dx ^ odd);
          T* dst = dc_s + (2 * dprow * COLS + col) * S32 + 8 * BW<T>::dcpiece(og, col);
#pragma unroll
          for (int dy = 0; dy < 2; ++dy)
            *(u32x4*)(dst + dy * COLS * S32) = (u32x4){ex[0][2 * dy + dx], ex[1][2 * dy + dx], ex[2][2 * dy + dx],
                                                       ex[3][2 * dy + dx]};
        }
      } else {
        float g[8];
        uint32_t c[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          g[e] = rg.g[0][e]; g[4 + e] = rg.g[1][e];
          code2_pair_codes((cd >> (8 * e)) & 0xffu, c[2 * e], c[2 * e + 1]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum[e] += c[e] < 4 ? g[e] : 0.f;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
          T* dst = dc_s + ((2 * dprow + (pos >> 1)) * COLS + 2 * dpcol + (pos & 1)) * S32 + 8 * og;
#pragma unroll
          for (int e = 0; e < 8; ++e) dst[e] = (int)c[e] == pos ? g[e] : 0.f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < BW<T>::P1IT; ++k) {
      if (pr_row[k] > 3) continue;
      const int slot = (ROWS * rq + 1 + pr_row[k]) & (BW_RING - 1);
      T* dst = p_s + slot * WPX * S16 + pr_lds[k];
      if constexpr (sizeof(T) == 2) {
        *(f32x4*)dst = rg.p[k];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { dst[e] = rg.p[k][e]; dst[4 + e] = rg.p[BW<T>::P1IT + k][e]; }
      }
    }
    STAMP(6);
    __syncthreads();
    STAMP(0);
    // ---- next step's loads (always issued: the very last step re-reads its own rows)
    int sn = s, bn = b, c0n = c0, rqn = rq + 1, rq_first_n = rq_first, rq_end_n = rq_end;
    if (rqn == rq_end) {
      sn = s + G;
      if (sn < n_items) {
        place(sn, bn, c0n, rq_first_n, rq_end_n);
        rqn = rq_first_n - 1;
      } else {
        rqn = rq;
      }
    }
    issue(bn, c0n, rqn, rqn >= rq_first_n);
    STAMP(1);

    if (rq >= rq_first) {
      // wave wv contracts row wv of the step (64 pixels = 2 bf16 k-steps / 16 fp32 k-steps)
      const int d = wv;
      if constexpr (sizeof(T) == 2) {
        int prow[3];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) prow[kh] = ((ROWS * rq + d - 1 + kh) & (BW_RING - 1)) * WPX * S16;
#pragma unroll
        for (int sgm = 0; sgm < COLS / 32; ++sgm) {
          const int cb = 32 * sgm + 8 * lg;   // this lane group's 8 pixels: cols cb .. cb+7 of row d
          bf16x8 a[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int pc8 = 16 * (i ^ (lg & 1)) + 4 * p4;     // swizzled 8-byte piece (columns cb+q, cb+4+q share bit 3)
            const bf16x4 lo = lds_tr16(&dc_s[(d * COLS + cb + q) * S32 + pc8]);
            const bf16x4 hi = lds_tr16(&dc_s[(d * COLS + cb + 4 + q) * S32 + pc8]);
            a[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
          bf16x8 bb[2];
          auto bfrag = [&](int tap) {
            const int kh = tap / 3, kw = tap % 3;
            const bf16x4 lo = lds_tr16(&p_s[prow[kh] + pcol_off[sgm][kw][0]]);
            const bf16x4 hi = lds_tr16(&p_s[prow[kh] + pcol_off[sgm][kw][1]]);
            return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          };
          bb[0] = bfrag(0);
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {      // the next tap's fragment is read before this tap's MFMAs issue
            if (tap + 1 < 9) bb[(tap + 1) & 1] = bfrag(tap + 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][tap] = mfma16(a[i], bb[tap & 1], acc[i][tap]);
          }
        }
      } else {
#pragma unroll 2
        for (int ks = 0; ks < COLS / 4; ++ks) {
          const int cpix = 4 * ks + lg;
          float a[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) a[i] = dc_s[(d * COLS + cpix) * S32 + 16 * i + lr];
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;
            const int slot = (ROWS * rq + d - 1 + kh) & (BW_RING - 1);
            const float bb = p_s[(slot * WPX + cpix + kw) * S16 + lr];
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][tap] = mfma16(a[i], bb, acc[i][tap]);
          }
        }
      }
    }
    STAMP(2);
    __syncthreads();   // this step's readers are done: the LDS images may be rebuilt
    STAMP(3);
    s = sn; b = bn; c0 = c0n; rq = rqn; rq_first = rq_first_n; rq_end = rq_end_n;
  }
  STAMP_FLUSH;
  // ---- cross-wave reduction in fixed order and slab write.  slab layout: [o 32][tap 9][ci 16] then 32 bias sums.
  // All four waves work at once, three taps at a time (the staging must fit the LDS of the step loop): every wave
  // stores its accumulators of the chunk as whole f32x4 [wave][i, tap][lane]; after one barrier each thread reads the
  // four waves' values of six slab elements -- all 24 reads issued before the first add -- and stores
  // ((w0 + w1) + w2) + w3 straight into the slab, 48-float runs per output channel.  (Waves taking turns at a
  // read-modify-write of one LDS image, then a copy to the slab, gave the same sums with every LDS access waited for
  // by itself and three waves idle: ~7 us per launch that nothing hides, the workgroups all end together.)
  __syncthreads();
  constexpr int TPC = 3, STAGE_W = 2 * TPC * 64 * 4;      // taps per chunk; floats per wave of the staging image
  f32x4* stage = (f32x4*)dyn_smem;
  const float* stage_f = (const float*)dyn_smem;
  float* bias_s = (float*)dyn_smem + 4 * STAGE_W;          // 2048 floats behind the staging image (host: sm covers both)
  float* slab = slabs + (int64_t)blockIdx.x * (4608 + 32);
  int red_src[6], red_dst[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int j = t + 256 * k, o = j / (16 * TPC), rem = j % (16 * TPC);     // rem = tap of the chunk * 16 + ci
    // accumulator element of (o, ci): tile i = o / 16, lane (lg = (o / 4) % 4, lr = ci), component r = o % 4
    red_src[k] = ((((o >> 4) * TPC + (rem >> 4)) * 64 + ((o >> 2) & 3) * 16 + (rem & 15)) << 2) + (o & 3);
    red_dst[k] = o * 144 + rem;
  }
#pragma unroll
  for (int c = 0; c < 9 / TPC; ++c) {
    if (c > 0) __syncthreads();                            // the previous chunk has been read
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int tl = 0; tl < TPC; ++tl) stage[(wv * 2 * TPC + i * TPC + tl) * 64 + l] = acc[i][TPC * c + tl];
    if (c == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bias_s[t * 8 + e] = bsum[e];
    }
    __syncthreads();
    float v[6][4];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int w = 0; w < 4; ++w) v[k][w] = stage_f[red_src[k] + w * STAGE_W];
#pragma unroll
    for (int k = 0; k < 6; ++k) slab[red_dst[k] + 16 * TPC * c] = ((v[k][0] + v[k][1]) + v[k][2]) + v[k][3];
  }
  if (t < 32) {                                            // bias sums: thread 4k + og holds channels 8 og .. 8 og + 7
    const int og = t >> 3, e = t & 7;
    float bv[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) bv[k] = bias_s[(4 * k + og) * 8 + e];
    __builtin_amdgcn_sched_barrier(0);                     // all reads in flight before the first (ordered) add
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 64; ++k) s += bv[k];
    slab[4608 + t] = s;
  }
}

// same items as the data gradient, small batches cut finer
inline SegPlan bwd_weight_plan(int B, int H1, int W1) {
  static const int nseg_exp = GDM_TUNABLE("GDM_BW_NSEG", 0);
  return seg_plan(B, H1, W1, 1024, COLS, cap::c2_bwd_weight(), nseg_exp);
}

template <typename T>
void launch_bwd_weight(const void* dp2, const uint8_t* code2, const void* p1, int B, int H1, int W1, const SegPlan& pl,
                       float* slabs, hipStream_t s) {
  const size_t red_bytes = (size_t)(4 * 6 * 256 + 2048) * sizeof(float);   // epilogue: staging image + bias sums
  size_t sm = (size_t)(BW<T>::DC_ELEMS + BW<T>::P_ELEMS) * sizeof(T) + (sizeof(T) == 2 ? C2T_BYTES : 0);
  if (sm < red_bytes) sm = red_bytes;
  allow_lds(conv2_bwd_weight_kernel<T>, sm);
  hipLaunchKernelGGL(conv2_bwd_weight_kernel<T>, dim3(pl.blocks), dim3(256), sm, s, (const T*)dp2, code2, (const T*)p1, B,
                     H1, W1, H1 / 2, W1 / 2, pl.n_ctiles, pl.nseg, pl.seg_len, pl.n_items, slabs);
}

}  // namespace

extern "C" size_t gdm_simnn_conv2_bwd_weight_workspace_bytes(int B, int H1, int W1) {
  return (size_t)(bwd_weight_plan(B, H1, W1).blocks + 65) * (4608 + 32) * sizeof(float);
}

extern "C" int gdm_simnn_conv2_bwd_weight(const void* dp2, const uint8_t* code2, const void* p1, int B, int H1, int W1,
                                          float* dw, float* db, int dtype, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  GDM_REQUIRE(dp2 && code2 && p1 && dw && db, "gdm_simnn_conv2_bwd_weight: null pointer");
  GDM_REQUIRE(B > 0 && H1 >= 2 && W1 >= 2 && gdm_dtype_ok(dtype), "gdm_simnn_conv2_bwd_weight: bad arguments");
  GDM_REQUIRE(fits_buffer_addressing(B, H1, W1), "gdm_simnn_conv2_bwd_weight: batch of %d %dx%d maps exceeds 2 GiB per tensor", B, H1, W1);
  if (!workspace || workspace_bytes < gdm_simnn_conv2_bwd_weight_workspace_bytes(B, H1, W1)) {
    gdm_set_error("gdm_simnn_conv2_bwd_weight: workspace too small");
    return GDM_EWORKSPACE;
  }
  const SegPlan pl = bwd_weight_plan(B, H1, W1);
  const int nblocks = pl.blocks;
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_T(dtype, launch_bwd_weight<T>(dp2, code2, p1, B, H1, W1, pl, (float*)workspace, s));
  float* scratch = (float*)workspace + (size_t)nblocks * (4608 + 32);
  gdm_launch_slab_sum(2, (const float*)workspace, nblocks, 4608 + 32, scratch, dw, db, 0, s);
  GDM_LAUNCH_OK("gdm_simnn_conv2_bwd_weight");
  return GDM_OK;
}

GDM_STAMP_READER(conv2_bwd_weight)
