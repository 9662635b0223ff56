// conv2 of model 1's discriminator trunk (simnn_trunk.h): the weight pack and the forward kernel.
#include "simnn_trunk.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void conv2_pack_kernel(const float* __restrict__ w, T* __restrict__ wf,
                                                         T* __restrict__ wb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < C2<T>::WF_ELEMS) wf[i] = from_f32<T>(conv2_packed_value<T, false>(w, i));
  if (i < C2<T>::WB_ELEMS) wb[i] = from_f32<T>(conv2_packed_value<T, true>(w, i));
}

// p1 halo band (rows r_first .. r_first+NR-1, cols c_first .. c_first+WP-1) -> LDS [row][col][S16], zero outside.
// Two phases so that every global load of the tile is in flight before the first LDS store.
template <typename T, int NR> struct P1Stage {
  static constexpr int PIECES = (sizeof(T) == 2) ? 2 : 4;          // 16-byte pieces per pixel record
  static constexpr int ITERS = (NR * C2<T>::WP * PIECES + 255) / 256;
  f32x4 v[ITERS];
};

template <typename T, int NR>
__device__ __forceinline__ void p1_band_load(P1Stage<T, NR>& st, rsrc_t p1r, uint32_t img_off, int H1, int W1,
                                             int r_first, int c_first) {
  constexpr int WP = C2<T>::WP, PIECES = P1Stage<T, NR>::PIECES;
#pragma unroll
  for (int k = 0; k < P1Stage<T, NR>::ITERS; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int piece = i % PIECES, pix = i / PIECES;
    const int cl = pix % WP, rl = pix / WP;
    const int r = r_first + rl, c = c_first + cl;
    const bool ok = i < NR * WP * PIECES && r >= 0 && r < H1 && c >= 0 && c < W1;
    const uint32_t off = img_off + (uint32_t)(r * W1 + c) * (16 * sizeof(T)) + piece * 16;   // bytes
    st.v[k] = buf_load16(p1r, ok ? off : BUF_OOB);
  }
}

// SPLIT: records of a band row are stored even columns first, then odd columns ([row][parity][WP/2][S16]), so that a
// reader whose lanes walk every second column (conv2 forward: a lane owns one pooled column) still steps one record
// per lane -- the conflict-free pattern of the plain layout.
template <typename T, int NR, bool SPLIT = false>
__device__ __forceinline__ void p1_band_store(const P1Stage<T, NR>& st, T* __restrict__ in_s) {
  constexpr int S16 = C2<T>::S16, WP = C2<T>::WP, PIECES = P1Stage<T, NR>::PIECES, EPP = 16 / PIECES;
#pragma unroll
  for (int k = 0; k < P1Stage<T, NR>::ITERS; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i >= NR * WP * PIECES) continue;
    const int piece = i % PIECES, pix = i / PIECES;
    int rec = pix;
    if constexpr (SPLIT) {
      const int cl = pix % WP, rl = pix / WP;
      rec = (rl * 2 + (cl & 1)) * C2<T>::HP + (cl >> 1);
    }
    T* dst = in_s + rec * S16 + piece * EPP;
    if constexpr (sizeof(T) == 2) *(f32x4*)dst = st.v[k];
    else { dst[0] = st.v[k][0]; dst[1] = st.v[k][1]; dst[2] = st.v[k][2]; dst[3] = st.v[k][3]; }
  }
}

// ---------------------------------------------------------------------------------------------------- conv2 forward
// One tile (4 conv rows x 64 columns of image b) from the LDS band in_s: MFMA implicit GEMM + bias/ReLU/pool epilogue.
// Wave (rp, half) computes conv rows 2rp, 2rp+1 x 32 columns x 32 channels.  The mapping is chosen so that the 2x2
// pooling window never leaves a lane: column tile j holds the band columns 32*half + 2*lr + j (lane lr = pooled column),
// so {acc[i][d][j]} over (d, j) ARE the window; and accumulator row 4*lg + r of channel tile i is channel 8*lg + 4*i + r,
// so a lane ends up with 8 consecutive channels of one pooled pixel = one 16-byte store (+ one 8-byte code store).
// The bias is the accumulator's initial value.
template <typename T>
__device__ __forceinline__ void conv2_fwd_tile(const T* __restrict__ in_s, const T* __restrict__ w_s,
                                               const float (&bo)[2][4], int b, int rq, int c0, int H2, int W2,
                                               rsrc_t p2r, rsrc_t code2r STAMP_ARG) {
  constexpr int S16 = C2<T>::S16, KP = C2<T>::KPF, HP = C2<T>::HP;
  const int t = threadIdx.x, l = t & 63, wv = t >> 6, lr = l & 15, lg = l >> 4;
  const int rp = wv >> 1, half = wv & 1;            // wave -> (pooled row of the tile, 32-column half)
  f32x4 acc[2][2][2];                               // [channel tile][row of the pair][column parity]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][d][j] = (f32x4){bo[i][0], bo[i][1], bo[i][2], bo[i][3]};
  const int arow = 8 * (lr >> 2) + (lr & 3);        // + 4*i: the channel this lane's A row stands for
  const int pcol = 16 * half + lr;                  // pooled column within the tile
  if constexpr (sizeof(T) == 2) {
    // fragments of k-step ks+1 are read from LDS before the 8 MFMAs of k-step ks are issued (register double buffer),
    // so that the LDS latency sits under the matrix pipe instead of in front of every MFMA pair
    bf16x8 a[2][2], bb[2][2][2];
    auto frags = [&](int ks, bf16x8 (&aa)[2], bf16x8 (&bx)[2][2]) {
      int tap = 2 * ks + (lg >> 1);
      tap = tap > 8 ? 8 : tap;               // k >= 144: weights are zero, read any valid record
      const int kh = tap / 3, kw = tap % 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) aa[i] = *(const bf16x8*)&w_s[(arow + 4 * i) * KP + 32 * ks + 8 * lg];
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int q = j + kw;               // band column 2*pcol + q
          bx[d][j] = *(const bf16x8*)&in_s[(((2 * rp + d + kh) * 2 + (q & 1)) * HP + pcol + (q >> 1)) * S16 +
                                           8 * (lg & 1)];
        }
    };
    frags(0, a[0], bb[0]);
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      if (ks + 1 < 5) frags(ks + 1, a[(ks + 1) & 1], bb[(ks + 1) & 1]);
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i][d][j] = mfma16(a[ks & 1][i], bb[ks & 1][d][j], acc[i][d][j]);
    }
  } else {
    // exact-fp32 mode: four k-steps (one tap) at a time -- the eight weight reads and sixteen activation reads of a tap are
    // issued together, ahead of its 32 MFMAs (two dependent LDS reads in front of every MFMA pair left the fp32 matrix
    // pipe waiting)
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap % 3;
      float a[4][2], bb[4][2][2];
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const int ks = 4 * tap + k4, ci = 4 * k4 + lg;
#pragma unroll
        for (int i = 0; i < 2; ++i) a[k4][i] = w_s[(arow + 4 * i) * KP + 4 * ks + lg];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int q = j + kw;
            bb[k4][d][j] = in_s[(((2 * rp + d + kh) * 2 + (q & 1)) * HP + pcol + (q >> 1)) * S16 + ci];
          }
      }
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][d][j] = mfma16(a[k4][i], bb[k4][d][j], acc[i][d][j]);
    }
  }
  STAMP(2);
  // ---- epilogue, all in-lane: first maximum of the window in scan order (as aten::max_pool2d_with_indices), ReLU,
  //      code = window position, or 4 when the pooled value is not positive (ReLU passes no gradient)
  float best[8];
  uint32_t codes = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v0 = acc[i][0][0][r], v1 = acc[i][0][1][r], v2 = acc[i][1][0][r], v3 = acc[i][1][1][r];
      const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
      uint32_t pos = 3u;                      // select chain, last write wins = first maximum (no branches)
      pos = v2 == m ? 2u : pos;
      pos = v1 == m ? 1u : pos;
      pos = v0 == m ? 0u : pos;
      best[4 * i + r] = fmaxf(m, 0.f);
      const uint32_t c = m > 0.f ? pos : 4u;
      // pair byte 8 * (c_even + 5 * c_odd) of channels 2j, 2j+1 (j = (4i + r) / 2) = byte j of the word (<= 192)
      codes += ((r & 1) ? c * 40u : c * 8u) << (8 * ((4 * i + r) >> 1));
    }
  const int ph = (ROWS / 2) * rq + rp, pw = (c0 >> 1) + pcol;
  const bool ok = ph < H2 && pw < W2;
  const uint32_t gi = (uint32_t)((b * H2 + ph) * W2 + pw) * 32 + 8 * lg;
  if constexpr (sizeof(T) == 2) {
    bf16x8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (__bf16)best[e];
    buf_store16<GDM_ACT_STORE_AUX>(p2r, ok ? gi * 2u : BUF_OOB, __builtin_bit_cast(f32x4, h));
  } else {
    buf_store16(p2r, ok ? gi * 4u : BUF_OOB, (f32x4){best[0], best[1], best[2], best[3]});
    buf_store16(p2r, ok ? gi * 4u + 16u : BUF_OOB, (f32x4){best[4], best[5], best[6], best[7]});
  }
  __builtin_amdgcn_raw_buffer_store_b32(codes, code2r, ok ? gi >> 1 : BUF_OOB, 0, GDM_ACT_STORE_AUX);
}

// Persistent over tiles; the weight image and the biases are fetched once per workgroup; input bands are prefetched
// TWO tiles ahead in two register sets (a tile's MFMA + epilogue is ~4x shorter than an HBM round trip under load, so
// one tile of look-ahead leaves the workgroup waiting for memory most of the time).
template <typename T>
__global__ __launch_bounds__(256) void conv2_fwd_kernel(const T* __restrict__ p1, const T* __restrict__ wf,
                                                        const float* __restrict__ bias, int H1, int W1, int H2,
                                                        int W2, int n_ctiles, int n_tiles, T* __restrict__ p2,
                                                        uint8_t* __restrict__ code2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  T* in_s = (T*)dyn_smem;
  T* w_s = in_s + C2<T>::IN_ELEMS;
  const int lg = (threadIdx.x & 63) >> 4;
  const int nrq = (2 * H2 + ROWS - 1) / ROWS, G = gridDim.x;
  // Every path through the loop issues the SAME number of global loads (tile indices past the end are clamped to the
  // last tile instead of skipping the loads): the hardware counts memory operations in order, so only then can the
  // compiler wait for "all but the other register set's loads" (vmcnt(N)) instead of draining the queue (vmcnt(0)).
  STAMP_DECL;
  const int B = n_tiles / (n_ctiles * nrq);
  const rsrc_t p1r = make_rsrc(p1, (uint32_t)B * H1 * W1 * 16 * sizeof(T));
  const rsrc_t p2r = make_rsrc(p2, (uint32_t)B * H2 * W2 * 32 * sizeof(T));
  const rsrc_t code2r = make_rsrc(code2, (uint32_t)B * H2 * W2 * 16);
  auto issue = [&](P1Stage<T, ROWS + 2>& st, int u) {
    u = min(u, n_tiles - 1);
    const int ct = u % n_ctiles, rq = (u / n_ctiles) % nrq, b = u / (n_ctiles * nrq);
    p1_band_load(st, p1r, (uint32_t)b * H1 * W1 * 16 * sizeof(T), H1, W1, ROWS * rq - 1, ct * COLS - 1);
  };
  auto run = [&](P1Stage<T, ROWS + 2>& st, int u, const float (&bo)[2][4]) {
    const int ct = u % n_ctiles, rq = (u / n_ctiles) % nrq, b = u / (n_ctiles * nrq);
    p1_band_store<T, ROWS + 2, true>(st, in_s);
    STAMP(6);
    __syncthreads();
    STAMP(0);
    issue(st, u + 2 * G);                                   // this register set is free again: two tiles ahead
    STAMP(1);
    conv2_fwd_tile<T>(in_s, w_s, bo, b, rq, ct * COLS, H2, W2, p2r, code2r STAMP_PASS);
    STAMP(3);
    __syncthreads();                                        // the band may be overwritten
    STAMP(4);
  };
  float bo[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) bo[i][r] = bias[8 * lg + 4 * i + r];     // channel map of conv2_fwd_tile
  // kernel start = ONE memory round trip: the weight image's loads go out first, the first two bands right behind them;
  // the image is stored (lds_image_finish waits for it alone) in front of the first run()'s barrier
  LdsImage<T, C2<T>::WF_ELEMS> wimg;
  lds_image_begin(wimg, wf);
  P1Stage<T, ROWS + 2> sa, sb;
  // Workgroups are dealt round-robin over the 8 XCDs (each with its own L2): give every XCD a CONTIGUOUS run of tile
  // ids per round, so that the tiles that share halo rows / columns (vertical neighbours are n_ctiles ids apart) are
  // fetched through the same L2.  With tile id = workgroup id every neighbour lived on another XCD and the 1.55x halo
  // over-read of the 6 x 66 band went to HBM in full (157 MB fetched for 101 MB of p1).
  int u = blockIdx.x;                                       // host guarantees gridDim.x <= n_tiles
  if ((G & 7) == 0) u = (u & 7) * (G >> 3) + (u >> 3);
  issue(sa, u);
  issue(sb, u + G);
  lds_image_finish(wimg, w_s);
  STAMP(5);
  for (; u + G < n_tiles; u += 2 * G) {
    run(sa, u, bo);
    run(sb, u + G, bo);
  }
  if (u < n_tiles) run(sa, u, bo);
  STAMP_FLUSH;
}

template <typename T>
void launch_fwd(const void* p1, const void* pack, const float* bias, int H1, int W1, int H2, int W2, int n_ctiles,
                int n_tiles, void* p2, uint8_t* code2, hipStream_t s) {
  const int cap = cap::c2_fwd();
  const size_t sm = (size_t)(C2<T>::IN_ELEMS + C2<T>::WF_ELEMS) * sizeof(T);
  if constexpr (sizeof(T) == 4) allow_lds(conv2_fwd_kernel<T>, sm);     // (bf16 stays under the default limit)
  hipLaunchKernelGGL(conv2_fwd_kernel<T>, dim3((unsigned)(n_tiles < cap ? n_tiles : cap)), dim3(256), sm, s,
                     (const T*)p1, (const T*)pack, bias, H1, W1, H2, W2, n_ctiles, n_tiles, (T*)p2, code2);
}

}  // namespace

extern "C" size_t gdm_simnn_conv2_pack_bytes(int dtype) {
  return dtype == GDM_BF16 ? (size_t)(C2<__bf16>::WF_ELEMS + C2<__bf16>::WB_ELEMS) * 2
                           : (size_t)(C2<float>::WF_ELEMS + C2<float>::WB_ELEMS) * 4;
}

extern "C" int gdm_simnn_conv2_pack(const float* w, int dtype, void* pack, void* stream) {
  GDM_REQUIRE(w && pack && gdm_dtype_ok(dtype), "gdm_simnn_conv2_pack: bad arguments");
  GDM_REQUIRE(((uintptr_t)pack & 15) == 0, "gdm_simnn_conv2_pack: pack buffer must be 16-byte aligned");
  DISPATCH_T(dtype, hipLaunchKernelGGL(conv2_pack_kernel<T>, dim3((C2<T>::WF_ELEMS + 255) / 256), dim3(256), 0,
                                       (hipStream_t)stream, w, (T*)pack, (T*)pack + C2<T>::WF_ELEMS));
  GDM_LAUNCH_OK("gdm_simnn_conv2_pack");
  return GDM_OK;
}

extern "C" int gdm_simnn_conv2_fwd(const void* p1, const void* pack, const float* bias, int B, int H1, int W1, void* p2,
                                   uint8_t* code2, int dtype, void* stream) {
  GDM_REQUIRE(p1 && pack && bias && p2 && code2, "gdm_simnn_conv2_fwd: null pointer");
  GDM_REQUIRE(B > 0 && H1 >= 2 && W1 >= 2 && gdm_dtype_ok(dtype), "gdm_simnn_conv2_fwd: bad arguments");
  GDM_REQUIRE(fits_buffer_addressing(B, H1, W1), "gdm_simnn_conv2_fwd: batch of %d %dx%d maps exceeds 2 GiB per tensor", B, H1, W1);
  const int H2 = H1 / 2, W2 = W1 / 2;
  const int n_ctiles = (2 * W2 + COLS - 1) / COLS;
  const int n_tiles = B * ((2 * H2 + ROWS - 1) / ROWS) * n_ctiles;
  DISPATCH_T(dtype, launch_fwd<T>(p1, pack, bias, H1, W1, H2, W2, n_ctiles, n_tiles, p2, code2, (hipStream_t)stream));
  GDM_LAUNCH_OK("gdm_simnn_conv2_fwd");
  return GDM_OK;
}

GDM_STAMP_READER(conv2_fwd)
