// conv2 backward-data of model 1's discriminator trunk (simnn_trunk.h), plain and fused with conv1's weight gradient.
#include "simnn_conv2_bwd.h"

namespace {

// ---------------------------------------------------------------------------------- conv2 backward (data [+ conv1 dW])
// dp1[ih][iw][ci] = sum_{ah,aw,o} dc2[ih-1+ah][iw-1+aw][o] * Wb[ci][(ah*3+aw)*32 + o]        (K = 288)
// where dc2 is the sparse full-resolution gradient  dc2[r][c][o] = (code2[r/2][c/2][o] == 2(r&1)+(c&1)) ? dp2[..] : 0.
//
// A persistent 256-thread workgroup walks STRIPS (image b, 64-column tile ct) top to bottom in steps of 4 output
// rows; wave w owns the 16 columns of column tile w (4 rows = 4 accumulators).  dc2 lives in an 8-row LDS ring: step rq needs conv rows
// 4rq-1 .. 4rq+4 and only the two pooled rows 2rq+1, 2rq+2 (conv rows 4rq+2 .. 4rq+5) are new, so every dp2/code2
// element of the strip is fetched and expanded once (a stand-alone 4-row tile with halo re-expands 2.1x as much).  A
// strip starts with the pseudo step rq = -1 (pooled rows -1 [zeros] and 0, no output).  The pooled rows of the next
// step are fetched into registers right after this step's expansion (software prefetch across steps and strips);
// every staging access is a buffer load/store whose out-of-image lanes read zeros / are dropped, so the step body has
// no branch around memory operations.  The bf16 ring keeps a pixel's four 16-byte channel groups XOR-swizzled by its
// column (group ^ ((col >> 1) & 2)): the B-fragment ds_read_b128 of 16 neighbouring pixels (64-byte records, lane
// groups {0-3,12-15,20-27}, ...) is then bank-conflict-free for every column offset (searched exhaustively).
//
// FUSE: instead of (or besides) writing dp1, route it through conv1's ReLU/pool code and contract it with the input
// window held in LDS:  dW1[c][kh][kw] += live * dp1[c] * x[2ih+dy-1+kh][2iw+dx-1+kw],  db1[c] += live * dp1[c];
// the workgroup's 80 partial sums go to one slab (summed in fixed order by slab_sum_kernel).
// (the selector tables for code2's pair bytes: simnn_conv2_bwd.h)

constexpr int BD_COLS = 64;
constexpr int BD_RING = 8;                     // conv rows in the LDS ring
constexpr int BD_WPX = BD_COLS + 4;            // stored columns: band column cl = -1 .. 66 lives at index cl + 1
constexpr int BD_NPC = BD_COLS / 2 + 2;        // pooled columns touching the band (c0/2 - 1 .. c0/2 + 32)
constexpr int BD_ITEMS = 2 * BD_NPC;           // pooled pixels expanded per step
constexpr int BD_DCIT = (BD_ITEMS * 4 + 255) / 256;
#ifndef GDM_BD_XW
#define GDM_BD_XW 256
#endif
constexpr int BD_XW = GDM_BD_XW;               // x-window row stride in LDS (>= BD_XCOLS = 136, multiple of 4)
constexpr int BD_XCOLS = 2 * BD_COLS + 8;      // x-window columns 2c0-4 .. 2c0+131 (16-byte aligned start)
// bf16 FUSE ("MF") epilogue: conv1's weight gradient is one more MFMA product (see conv2_bwd_data_kernel).  The input
// window lives in LDS as four bf16 planes [hi|lo part][kw] of XROWS rows: plane(kw)[row][m] = x[row][m + 3 + kw], so
// that the 8 window values a lane needs for its 4 pixels x 2 pooling columns are ONE aligned 16-byte read.  Row stride
// 288 B and plane stride = 64 (mod 256) B put the 16 (plane, kh, lane group) combinations of a read on 16 distinct
// 16-byte slots of the 256-byte bank row.
constexpr int XP_ROW = 144;                     // bf16 elements per plane row (128 used)
constexpr int XP_PLANE = XROWS * XP_ROW + 16;   // elements (2624 B)
constexpr int XP_ONES = 8 * XP_ROW;             // a block of 1.0: the B operand column that sums the bias gradient
constexpr int XP_ELEMS = 4 * XP_PLANE + XP_ONES;
template <typename T> struct BD {
  static constexpr int DC_ELEMS = BD_RING * BD_WPX * C2<T>::S32;
  static constexpr size_t TAB = sizeof(T) == 2 ? C2T_BYTES : 0;      // code2 selector tables (bf16)
  static constexpr size_t lds_bytes(bool fuse) {
    if (!fuse) return (size_t)(DC_ELEMS + C2<T>::WB_ELEMS) * sizeof(T) + TAB;
    const size_t xbytes = sizeof(T) == 2 ? (size_t)XP_ELEMS * 2 + 64 : (size_t)(XROWS * BD_XW) * 4;
    return (size_t)(DC_ELEMS + C2<T>::WB_ELEMS) * sizeof(T) + TAB + xbytes + (size_t)(4 * 80) * 4;
  }
};

// Everything a workgroup fetches from HBM for one step, held in registers between "issue" and "consume".
template <typename T, bool FUSE, bool XVEC> struct BdStepRegs {
  static constexpr int XIT = FUSE ? (XVEC ? (XROWS * (BD_XCOLS / 4) + 255) / 256 : (XROWS * BD_XCOLS + 255) / 256) : 1;
  static constexpr bool MF = FUSE && sizeof(T) == 2;
  f32x4 g[BD_DCIT][sizeof(T) == 2 ? 1 : 2];
  uint32_t cd[BD_DCIT];                       // four pair bytes = the item's 8 channels
  f32x4 xv4[XVEC ? XIT : 1];
  float xv[XVEC ? (MF ? XIT : 1) : XIT];     // XVEC && MF: the window value left of each vector (column bc - 1)
  uint64_t codes[FUSE ? 4 : 1];
};

struct BdRsrc {
  rsrc_t dp2, code2, dp1, code1;
};

// Per-thread constants of the staging pattern (they depend on the lane only, never on the step): computed once so
// that issuing a step's loads costs a handful of VALU per load.
template <bool FUSE, bool XVEC> struct BdLane {
  static constexpr int XIT = FUSE ? (XVEC ? (XROWS * (BD_XCOLS / 4) + 255) / 256 : (XROWS * BD_XCOLS + 255) / 256) : 1;
  uint32_t dc_off[BD_DCIT];      // (prow * W2 + pcol) * 32 + 8 og
  int dc_prow[BD_DCIT], dc_pcol[BD_DCIT];   // prow = 99 marks a lane without an item
  uint32_t x_off[XIT];           // (br * W + bc) * 4
  int x_br[XIT], x_bc[XIT];      // br = 99 marks a lane without an element
};

template <typename T, bool FUSE, bool XVEC>
__device__ __forceinline__ void bd_issue(BdStepRegs<T, FUSE, XVEC>& rg, const BdLane<FUSE, XVEC>& ln, int b, int c0,
                                         int rq, const BdRsrc& rs, int H1, int W1, int H2, int W2,
                                         const float* __restrict__ x0, const float* __restrict__ x1, int bsplit, int H,
                                         int W) {
  constexpr bool MF = FUSE && sizeof(T) == 2;
  const int t = threadIdx.x, lr = t & 15, lg = (t >> 4) & 3, wv = t >> 6;
  const int pr0 = 2 * rq + 1, pc0 = (c0 >> 1) - 1;
  const uint32_t base = (uint32_t)b * H2 * W2 * 32 + (uint32_t)(pr0 * W2 + pc0) * 32;   // may wrap: only used when valid
#pragma unroll
  for (int k = 0; k < BD_DCIT; ++k) {
    const bool ok = (unsigned)(pr0 + ln.dc_prow[k]) < (unsigned)H2 && (unsigned)(pc0 + ln.dc_pcol[k]) < (unsigned)W2;
    const uint32_t gi = base + ln.dc_off[k];
    rg.cd[k] = __builtin_bit_cast(uint32_t, buf_load4(rs.code2, ok ? gi >> 1 : BUF_OOB));
    rg.g[k][0] = buf_load16(rs.dp2, ok ? gi * (uint32_t)sizeof(T) : BUF_OOB);
    if constexpr (sizeof(T) == 4) rg.g[k][1] = buf_load16(rs.dp2, ok ? gi * 4u + 16u : BUF_OOB);
  }
  if constexpr (FUSE) {
    // the input image of sample b lives in one of two tensors (real | generated): one descriptor per step
    const float* xb = (b < bsplit) ? x0 + (int64_t)b * H * W : x1 + (int64_t)(b - bsplit) * H * W;
    const rsrc_t xr_ = make_rsrc(xb, (uint32_t)H * W * 4);
    const int xr0 = 2 * ROWS * rq - 1, xc0 = 2 * c0 - 4;
    const uint32_t xbase = (uint32_t)(xr0 * W + xc0) * 4u;
#pragma unroll
    for (int k = 0; k < BdLane<FUSE, XVEC>::XIT; ++k) {
      // XVEC: W % 4 == 0, a 4-column vector is inside or outside the image as a whole.  Row and column validity are
      // merged ARITHMETICALLY (OR of the out-of-range bit): with `row_ok && col_ok` shared by two loads the compiler
      // turned the row test into a branch around them and put s_waitcnt vmcnt(0) in front of the second version of each
      // load -- every step then waited for everything in flight, the look-ahead was gone.
      const uint32_t rbad = (unsigned)(xr0 + ln.x_br[k]) < (unsigned)H ? 0u : BUF_OOB;
      const uint32_t off = ((unsigned)(xc0 + ln.x_bc[k]) < (unsigned)W ? xbase + ln.x_off[k] : BUF_OOB) | rbad;
      if constexpr (XVEC) {
        rg.xv4[k] = buf_load16<GDM_IN_LOAD_AUX>(xr_, off);
        if constexpr (MF) {
          // the kw = 0 plane is the kw = 1 plane shifted by one column: each vector also needs its left neighbour
          const uint32_t offm = ((unsigned)(xc0 + ln.x_bc[k] - 1) < (unsigned)W ? xbase + ln.x_off[k] - 4u : BUF_OOB) | rbad;
          rg.xv[k] = buf_load4<GDM_IN_LOAD_AUX>(xr_, offm);
        }
      } else {
        rg.xv[k] = buf_load4<GDM_IN_LOAD_AUX>(xr_, off);
      }
    }
    const int Q1 = (W1 + 3) >> 2;
    if constexpr (MF) {
      // lane (channel lr, pixel quad lg of this wave's 16 columns): the four pixels' fields of channel group lr / 4
      const int quad = (c0 >> 2) + 4 * wv + lg;
      const uint32_t cbase = (((uint32_t)(b * H1 + ROWS * rq) * Q1 + quad) * 4u + (uint32_t)(lr >> 2)) * 8u;
#pragma unroll
      for (int ir = 0; ir < 4; ++ir) {
        const bool ok = (unsigned)(ROWS * rq + ir) < (unsigned)H1 && quad < Q1;
        rg.codes[ir] = buf_load8<GDM_IN_LOAD_AUX>(rs.code1, ok ? cbase + (uint32_t)(ir * Q1) * 32u : BUF_OOB);
      }
    } else {
      // lane (pixel lr, channel group lg): one 16-bit field per row, rows 4rq .. 4rq+3
      const int iw = c0 + 16 * wv + lr;
#pragma unroll
      for (int ir = 0; ir < 4; ++ir) {
        const bool ok = (unsigned)(ROWS * rq + ir) < (unsigned)H1 && iw < W1;
        const uint32_t fi = code1_field((uint32_t)(b * H1 + ROWS * rq + ir), Q1, iw, lg) * 2u;
        rg.codes[ir] = (uint64_t)__builtin_amdgcn_raw_buffer_load_b16(rs.code1, ok ? fi : BUF_OOB, 0, GDM_IN_LOAD_AUX);
      }
    }
  }
}

// Registers of step rq -> ring rows 4rq+2 .. 4rq+5.  Lane = (pooled pixel, 8-channel group): four 16-byte records.
// (OOB items loaded zeros: pair byte 0 = "both channels at position 0" of a zero gradient -> zeros everywhere.)
// slot0 = ring row of the step's first new conv row (even), RING = rows in the ring.
template <typename T, bool FUSE, bool XVEC, int RING = BD_RING>
__device__ __forceinline__ void bd_expand(const BdStepRegs<T, FUSE, XVEC>& rg, const BdLane<FUSE, XVEC>& ln, int slot0,
                                          T* __restrict__ dc_s, const unsigned char* __restrict__ tab) {
  constexpr int S32 = C2<T>::S32;
  const int og = threadIdx.x & 3;
#pragma unroll
  for (int k = 0; k < BD_DCIT; ++k) {
    const int prow = ln.dc_prow[k], pcol = ln.dc_pcol[k];
    if (prow > 1) continue;
    int slot = slot0 + 2 * prow;                                         // even: slot + 1 never wraps
    if (slot >= RING) slot -= RING;
    const uint32_t cd = rg.cd[k];
    if constexpr (sizeof(T) == 2) {
      const u32x4 gv = __builtin_bit_cast(u32x4, rg.g[k][0]);
      uint32_t ex[4][4];                                                  // [channel pair][position]
      const int odd = pcol & 1;                                           // odd pooled column: columns swapped (tables A'/B')
      const unsigned char* tab_l = tab + (odd ? C2T_SWAP : 0);
#pragma unroll
      for (int w = 0; w < 4; ++w) code2_expand_pair(tab_l, (cd >> (8 * w)) & 0xffu, gv[w], ex[w]);
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int sc = 2 * pcol + (dx ^ odd);                                 // stored column
        const int piece = og ^ ((sc >> 1) & 2);                               // swizzled 16-byte slot of the record
        T* dst = dc_s + (slot * BD_WPX + sc) * S32 + 8 * piece;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
          *(u32x4*)(dst + dy * BD_WPX * S32) = (u32x4){ex[0][2 * dy + dx], ex[1][2 * dy + dx], ex[2][2 * dy + dx],
                                                       ex[3][2 * dy + dx]};
      }
    } else {
      float g[8];
      uint32_t c[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g[e] = rg.g[k][0][e]; g[4 + e] = rg.g[k][1][e];
        code2_pair_codes((cd >> (8 * e)) & 0xffu, c[2 * e], c[2 * e + 1]);
      }
#pragma unroll
      for (int pos = 0; pos < 4; ++pos) {
        T* dst = dc_s + ((slot + (pos >> 1)) * BD_WPX + 2 * pcol + (pos & 1)) * S32 + 8 * og;
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = (int)c[e] == pos ? g[e] : 0.f;
      }
    }
  }
}

// bf16 FUSE ("MF"): the data-gradient MFMA is issued with its operands SWAPPED (A = gradient fragments: rows = pixels,
// B = weights: columns = input channels), so a lane of the result holds ONE channel (lr) and FOUR neighbouring pixels
// (4 lg + r) of each of the step's four rows.  That is the A-operand layout of one more MFMA product,
//     S[c][n] += sum_k A[c][k] * X[k][n],      k = (pixel 4lg + r, pooling column dx)  for a fixed (row ir, pooling row dy)
//     A[c][k] = dp1[c][pixel] if channel c of that pixel is live and its argmax is (dy, dx), else 0
//     X[k][n] = x[2 ih + dy - 1 + kh][2 iw + dx - 1 + kw]  for n = tap (kh, kw) -- 8 CONSECUTIVE window values,
// i.e. conv1's weight gradient as the weight gradient of the full-resolution convolution (K = full-resolution pixels,
// one non-zero per pooling window): 8 MFMAs per wave and step.  A is built from the accumulators with one cvt_pk, one
// 8-byte LDS table read (argmax code -> two v_perm selectors) and two v_perm per value; X is one aligned 16-byte read
// from the bf16 planes (columns 0-3 of the result: high parts of x, 4-7: low parts -- x stays exact to 2^-17 --,
// column 8: a block of ones = the bias gradient).  The round-1/2 epilogue (position-dependent 2x2 gathers from an fp32
// window + 20 FMAs per value: 58 of the kernel's 117 us, 37 % of its LDS cycles bank conflicts) is kept for fp32 only.
// DP1: the data gradient itself is written out (always without FUSE; with FUSE only for the module's input-gradient
// path -- the training step never needs it, and as a run-time test the 16 stores stayed in the step body).
template <typename T, bool FUSE, bool XVEC, bool DP1>
__global__ __launch_bounds__(256) void conv2_bwd_data_kernel(const T* __restrict__ dp2,
                                                             const uint8_t* __restrict__ code2,
                                                             const T* __restrict__ wb, int B, int H1, int W1, int H2,
                                                             int W2, int n_ctiles, int nseg, int seg_len,
                                                             int n_strips, T* __restrict__ dp1,
                                                             const uint16_t* __restrict__ code1,
                                                             const float* __restrict__ x0,
                                                             const float* __restrict__ x1, int bsplit, int H, int W,
                                                             float* __restrict__ slabs) {
  constexpr int S32 = C2<T>::S32, KP = C2<T>::KPB, XW = BD_XW;
  constexpr bool MF = FUSE && sizeof(T) == 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  T* dc_s = (T*)dyn_smem;
  T* w_s = dc_s + BD<T>::DC_ELEMS;
  unsigned char* tab_s = (unsigned char*)(w_s + C2<T>::WB_ELEMS);     // bf16: code2 selector tables
  float* x_s = (float*)(tab_s + BD<T>::TAB);              // FUSE, fp32: [XROWS][XW]
  __bf16* xp_s = (__bf16*)(tab_s + BD<T>::TAB);           // MF: four planes + ones block, then the selector table
  uint32_t* tbl_s = (uint32_t*)(xp_s + XP_ELEMS);         // MF: 8 x {selector for dy = 0, selector for dy = 1}
  float* red = MF ? (float*)(tbl_s + 16) : x_s + XROWS * XW;   // FUSE: [4][80]
  const int t = threadIdx.x, l = t & 63, wv = t >> 6, lr = l & 15, lg = l >> 4;
  const int nrq = (H1 + ROWS - 1) / ROWS, G = gridDim.x;

  float a1[MF ? 1 : 4][4], bs[4];
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f};                         // MF: S[c = 4lg + r][n = lr]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bs[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) a1[MF ? 0 : r][q] = 0.f;
  }
  STAMP_DECL;
  BdRsrc rs;
  rs.dp2 = make_rsrc(dp2, (uint32_t)B * H2 * W2 * 32 * sizeof(T));
  rs.code2 = make_rsrc(code2, (uint32_t)B * H2 * W2 * 16);
  rs.dp1 = make_rsrc(dp1, DP1 ? (uint32_t)B * H1 * W1 * 16 * sizeof(T) : 0u);
  rs.code1 = make_rsrc(code1, FUSE ? (uint32_t)B * H1 * ((W1 + 3) >> 2) * 32 : 0u);
  // kernel start = ONE memory round trip: the weight image's loads go out first, the first two steps' loads right
  // behind them; the LDS-only set-up follows, and the image is stored (lds_image_finish waits for it alone) in front
  // of the first barrier
  LdsImage<T, C2<T>::WB_ELEMS> wimg;
  lds_image_begin(wimg, wb);
  BdLane<FUSE, XVEC> ln;
#pragma unroll
  for (int k = 0; k < BD_DCIT; ++k) {
    const int i = t + 256 * k, item = i >> 2, og = i & 3;
    const bool has = item < BD_ITEMS;
    ln.dc_prow[k] = has ? item / BD_NPC : 99;
    ln.dc_pcol[k] = item % BD_NPC;
    ln.dc_off[k] = (uint32_t)((item / BD_NPC) * W2 + item % BD_NPC) * 32 + 8 * og;
  }
  if constexpr (FUSE) {
#pragma unroll
    for (int k = 0; k < BdLane<FUSE, XVEC>::XIT; ++k) {
      const int i = t + 256 * k;
      constexpr int PER_ROW = XVEC ? BD_XCOLS / 4 : BD_XCOLS;
      const int br = i / PER_ROW, bc = (i % PER_ROW) * (XVEC ? 4 : 1);
      ln.x_br[k] = br < XROWS ? br : 99;
      ln.x_bc[k] = bc;
      ln.x_off[k] = (uint32_t)(br * W + bc) * 4u;
    }
  }

  // work item s = (image b, row segment seg, column tile ct); a segment is seg_len steps and starts with a pseudo step
  auto place = [&](int s_, int& b_, int& c0_, int& rq_first, int& rq_end) {
    const int ct = s_ % n_ctiles, sg = (s_ / n_ctiles) % nseg;
    b_ = s_ / (n_ctiles * nseg);
    c0_ = ct * BD_COLS;
    rq_first = sg * seg_len;
    rq_end = min(rq_first + seg_len, nrq);
  };
  // Step positions.  The loads of a step are issued TWO steps ahead into one of two register sets: with one step of
  // look-ahead a step could not be shorter than one HBM round trip under load (~2 us) -- halving the step's VALU work
  // (round 3: 418 -> 270 instructions per wave) did not move the kernel by a microsecond until the look-ahead doubled.
  struct Pos { int s, b, c0, rq, rq_first, rq_end; };
  auto advance = [&](const Pos& q) {
    Pos n = q;
    if (q.s >= n_strips) return n;                          // past the end: keep re-reading the last rows
    n.rq = q.rq + 1;
    if (n.rq == q.rq_end) {
      n.s = q.s + G;
      if (n.s < n_strips) {
        place(n.s, n.b, n.c0, n.rq_first, n.rq_end);
        n.rq = n.rq_first - 1;
      } else {
        n.rq = q.rq;                                        // nothing left: its loads re-read cache-hot rows
      }
    }
    return n;
  };
  // (fp32: one register set, one step of look-ahead -- a second set does not fit 256 VGPRs beside the 72 weight registers)
  constexpr bool AHEAD2 = sizeof(T) == 2;
  BdStepRegs<T, FUSE, XVEC> rg_a, rg_b;
  Pos p0, p1;
  p0.s = blockIdx.x;                                        // host guarantees gridDim.x <= n_strips
  place(p0.s, p0.b, p0.c0, p0.rq_first, p0.rq_end);
  p0.rq = p0.rq_first - 1;
  p1 = advance(p0);
  bd_issue<T, FUSE, XVEC>(rg_a, ln, p0.b, p0.c0, p0.rq, rs, H1, W1, H2, W2, x0, x1, bsplit, H, W);
  if constexpr (AHEAD2) bd_issue<T, FUSE, XVEC>(rg_b, ln, p1.b, p1.c0, p1.rq, rs, H1, W1, H2, W2, x0, x1, bsplit, H, W);
  if constexpr (sizeof(T) == 2) code2_tables_init((uint32_t*)tab_s);
  if constexpr (MF) {
    // argmax code (bits 1:0 position, bit 2 live) -> v_perm selectors that place the bf16 gradient (bytes 0,1 of the
    // source) in the low (dx = 0) or high (dx = 1) half of the A dword of pooling row dy, or nowhere (0x0c = 0x00)
    if (t < 8) {
      const uint32_t none = 0x0c0c0c0cu, lo = 0x0c0c0100u, hi = 0x01000c0cu;
      const bool live = t >= 4;
      const int pos = t & 3;
      tbl_s[2 * t] = (live && (pos >> 1) == 0) ? ((pos & 1) ? hi : lo) : none;
      tbl_s[2 * t + 1] = (live && (pos >> 1) == 1) ? ((pos & 1) ? hi : lo) : none;
    }
    for (int i = t; i < XP_ONES / 2; i += 256) ((uint32_t*)(xp_s + 4 * XP_PLANE))[i] = 0x3f803f80u;   // bf16 1.0 pairs
    // plane cells no step ever writes (row padding, columns the window does not reach) must hold finite values:
    // they are read by lanes whose result columns are discarded
    for (int i = t; i < 4 * XP_PLANE / 2; i += 256) ((uint32_t*)xp_s)[i] = 0u;
  }
  lds_image_finish(wimg, w_s);
  __syncthreads();                                          // weight image complete

  // Wave w computes the 4 output rows of column tile w (16 columns).  A dc2 row fragment (one per tap column aw) feeds
  // the up to three output rows it touches, and the weight fragments of all nine taps stay in registers for the whole
  // kernel (bf16): 18 LDS fragment reads per 36 MFMAs.
  bf16x8 afr[sizeof(T) == 2 ? 9 : 1];
  float afw[sizeof(T) == 4 ? 72 : 1];
  int cb[3];
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int k = 0; k < 72; ++k) afw[k] = w_s[lr * KP + 4 * k + lg];
  }
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int ks = 0; ks < 9; ++ks) afr[ks] = *(const bf16x8*)&w_s[lr * KP + 32 * ks + 8 * lg];
#pragma unroll
    for (int aw = 0; aw < 3; ++aw) {
      const int sc = 16 * wv + lr + aw + 1;
      cb[aw] = sc * S32 + 8 * (lg ^ ((sc >> 1) & 2));
    }
  }
  // MF: per-lane constants of the epilogue
  //   xb_off: element offset of this lane's X fragment for (ir, dy) = (0, 0); result column n = lr: n < 4 high plane of
  //           tap (kh, kw) = (n >> 1, n & 1), 4..7 the low plane, >= 8 the block of ones (only column 8 is used)
  //   sh0/sh1: rotation that brings the lane's channel nibble of pixel r (even / odd: low / high half word) to bits 5:3
  const int xb_off = lr < 8 ? (2 * (lr >> 2) + (lr & 1)) * XP_PLANE + ((lr >> 1) & 1) * XP_ROW + 32 * wv + 8 * lg
                            : 4 * XP_PLANE;
  const uint32_t sh0 = 29u + 4u * (lr & 3), sh1 = sh0 + 16u;
  STAMP(6);
  auto step = [&](BdStepRegs<T, FUSE, XVEC>& rg, const Pos& cur, const Pos& nxt) {
    const int b = cur.b, c0 = cur.c0, rq = cur.rq, rq_first = cur.rq_first;
    // ---- consume the prefetched registers into the LDS images of this step
    STAMP(3);
#ifdef GDM_STAMPS
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");     // (stamp builds: this set's 12 loads have landed; the other set's 12 fly)
    STAMP(6);
#endif
    bd_expand<T, FUSE, XVEC>(rg, ln, (ROWS * rq + 2) & (BD_RING - 1), dc_s, tab_s);
    uint64_t codes[FUSE ? 4 : 1];
    if constexpr (FUSE) {
      if constexpr (MF) {
        // fp32 window values -> bf16 high / low parts in the two column-shifted planes
        auto split = [](float v0, float v1, uint32_t& hi, uint32_t& lo) {
          const bf16x2 h = {(__bf16)v0, (__bf16)v1};
          hi = __builtin_bit_cast(uint32_t, h);
          const float r0 = v0 - __builtin_bit_cast(float, hi << 16), r1 = v1 - __builtin_bit_cast(float, hi & 0xffff0000u);
          const bf16x2 lw = {(__bf16)r0, (__bf16)r1};
          lo = __builtin_bit_cast(uint32_t, lw);
        };
#pragma unroll
        for (int k = 0; k < BdLane<FUSE, XVEC>::XIT; ++k) {
          if constexpr (XVEC) {
            // vector = window columns bc .. bc+3 -> plane kw=1 cells m = bc-4 .. bc-1; with the left neighbour in
            // front (bc-1 .. bc+2) the same cells of plane kw=0
            if (ln.x_br[k] < XROWS && ln.x_bc[k] >= 4) {
              const f32x4 v = rg.xv4[k];
              const float vm = rg.xv[k];
              __bf16* cell = xp_s + ln.x_br[k] * XP_ROW + ln.x_bc[k] - 4;
              uint32_t h00, h01, l00, l01, h10, h11, l10, l11;
              split(vm, v[0], h00, l00);
              split(v[1], v[2], h01, l01);
              split(v[0], v[1], h10, l10);
              split(v[2], v[3], h11, l11);
              *(u32x2*)(cell) = (u32x2){h00, h01};
              *(u32x2*)(cell + XP_PLANE) = (u32x2){h10, h11};
              *(u32x2*)(cell + 2 * XP_PLANE) = (u32x2){l00, l01};
              *(u32x2*)(cell + 3 * XP_PLANE) = (u32x2){l10, l11};
            }
          } else {
            // one window value: cell m = bc - 3 of plane kw=0 and m = bc - 4 of plane kw=1
            if (ln.x_br[k] < XROWS && ln.x_bc[k] >= 3) {
              const float v = rg.xv[k];
              const __bf16 h = (__bf16)v, lw = (__bf16)(v - (float)h);
              __bf16* cell = xp_s + ln.x_br[k] * XP_ROW + ln.x_bc[k] - 3;
              cell[0] = h;
              cell[2 * XP_PLANE] = lw;
              if (ln.x_bc[k] >= 4) {
                cell[XP_PLANE - 1] = h;
                cell[3 * XP_PLANE - 1] = lw;
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < BdLane<FUSE, XVEC>::XIT; ++k) {
          if (ln.x_br[k] < XROWS) {
            if constexpr (XVEC) *(f32x4*)&x_s[ln.x_br[k] * XW + ln.x_bc[k]] = rg.xv4[k];
            else x_s[ln.x_br[k] * XW + ln.x_bc[k]] = rg.xv[k];
          }
        }
      }
#pragma unroll
      for (int ir = 0; ir < 4; ++ir) codes[ir] = rg.codes[ir];
    }
    STAMP(7);
    __syncthreads();
    STAMP(0);
    // this register set is free again: the loads of the step after next fly during this step and the next one; issued on
    // EVERY step (past the end they re-read cache-hot rows), so the step body has no branch around memory operations
    bd_issue<T, FUSE, XVEC>(rg, ln, nxt.b, nxt.c0, nxt.rq, rs, H1, W1, H2, W2, x0, x1, bsplit, H, W);
    STAMP(1);

    if (rq >= rq_first) {
      f32x4 acc[4];                                         // [output row of the step]
#pragma unroll
      for (int ir = 0; ir < 4; ++ir) acc[ir] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (sizeof(T) == 2) {
        // band row rr (conv row 4rq-1+rr) contributes to output row ir = rr - ah with tap row ah; the fragments of
        // row rr+1 are read before the MFMAs of row rr issue.  Per accumulator the taps arrive in ascending order.
        bf16x8 bb[2][3];
        auto row_frags = [&](int rr, bf16x8 (&bx)[3]) {
          const int ro = ((ROWS * rq - 1 + rr) & (BD_RING - 1)) * BD_WPX * S32;
#pragma unroll
          for (int aw = 0; aw < 3; ++aw) bx[aw] = *(const bf16x8*)&dc_s[ro + cb[aw]];
        };
        row_frags(0, bb[0]);
#pragma unroll
        for (int rr = 0; rr < ROWS + 2; ++rr) {
          if (rr + 1 < ROWS + 2) row_frags(rr + 1, bb[(rr + 1) & 1]);
#pragma unroll
          for (int ah = 2; ah >= 0; --ah) {
            const int ir = rr - ah;
            if (ir < 0 || ir >= ROWS) continue;
#pragma unroll
            for (int aw = 0; aw < 3; ++aw) {
              // MF: operands swapped -> result row = pixel 4lg + r, column = input channel lr (same sums, transposed)
              if constexpr (MF) acc[ir] = mfma16(bb[rr & 1][aw], afr[3 * ah + aw], acc[ir]);
              else acc[ir] = mfma16(afr[3 * ah + aw], bb[rr & 1][aw], acc[ir]);
            }
          }
        }
      } else {
        // exact-fp32 mode: the weight fragments of all nine taps live in registers (72 per lane, loaded once per
        // kernel), so a v_mfma_f32_16x16x4_f32 costs one LDS read (the gradient value, shared by up to three output
        // rows) instead of two; the eight reads of a (row, tap column) are issued together ahead of their MFMAs
#pragma unroll
        for (int rr = 0; rr < ROWS + 2; ++rr) {
          const int ro = ((ROWS * rq - 1 + rr) & (BD_RING - 1)) * BD_WPX;
#pragma unroll
          for (int aw = 0; aw < 3; ++aw) {
            float bb[8];
#pragma unroll
            for (int o4 = 0; o4 < 8; ++o4) bb[o4] = dc_s[(ro + 16 * wv + lr + aw + 1) * S32 + 4 * o4 + lg];
#pragma unroll
            for (int o4 = 0; o4 < 8; ++o4)
#pragma unroll
              for (int ah = 2; ah >= 0; --ah) {
                const int ir = rr - ah;
                if (ir < 0 || ir >= ROWS) continue;
                acc[ir] = mfma16(afw[(3 * ah + aw) * 8 + o4], bb[o4], acc[ir]);
              }
          }
        }
      }
      STAMP(2);
      if constexpr (MF) {
        // C layout (swapped): col (lr) = input channel ci, row (4*lg + r) = pixel of the wave's 16 columns
        if constexpr (DP1) {
#pragma unroll
          for (int ir = 0; ir < 4; ++ir) {
            const int ih = ROWS * rq + ir;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int iw = c0 + 16 * wv + 4 * lg + r;
              const bool ok = ih < H1 && iw < W1;
              const uint32_t di = (uint32_t)((b * H1 + ih) * W1 + iw) * 16 + lr;
              const __bf16 v = (__bf16)acc[ir][r];
              buf_store2(rs.dp1, ok ? di * 2u : BUF_OOB, (uint32_t)__builtin_bit_cast(unsigned short, v));
            }
          }
        }
        const unsigned char* xp_b = (const unsigned char*)xp_s + 2 * xb_off;
        const unsigned char* tb = (const unsigned char*)tbl_s;
        u32x2 sel[2][4];
        auto selectors = [&](int ir, u32x2 (&so)[4]) {
          const uint32_t clo = (uint32_t)codes[ir], chi = (uint32_t)(codes[ir] >> 32);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t word = r < 2 ? clo : chi;
            // rotate right by (nibble offset - 3) mod 32 (the instruction takes the shift modulo 32)
            const uint32_t idx8 = __builtin_amdgcn_alignbit(word, word, (r & 1) ? sh1 : sh0) & 0x38u;
            so[r] = *(const u32x2*)(tb + idx8);
          }
        };
        selectors(0, sel[0]);
#pragma unroll
        for (int ir = 0; ir < 4; ++ir) {
          if (ir + 1 < 4) selectors(ir + 1, sel[(ir + 1) & 1]);      // table reads of the next row fly under this one
          const bf16x8 xf0 = *(const bf16x8*)(xp_b + (2 * ir) * (XP_ROW * 2));
          const bf16x8 xf1 = *(const bf16x8*)(xp_b + (2 * ir + 1) * (XP_ROW * 2));
          u32x4 a0, a1v;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gv = acc[ir][r];
            const bf16x2 gp = {(__bf16)gv, (__bf16)gv};
            const uint32_t gg = __builtin_bit_cast(uint32_t, gp);
            a0[r] = __builtin_amdgcn_perm(0u, gg, sel[ir & 1][r][0]);
            a1v[r] = __builtin_amdgcn_perm(0u, gg, sel[ir & 1][r][1]);
          }
          s1 = mfma16(__builtin_bit_cast(bf16x8, a0), xf0, s1);
          s1 = mfma16(__builtin_bit_cast(bf16x8, a1v), xf1, s1);
        }
      } else {
        // C layout: col (lr) = pixel, row (4*lg + r) = input channel ci
        const int iw = c0 + 16 * wv + lr;
        if constexpr (DP1) {
#pragma unroll
          for (int ir = 0; ir < 4; ++ir) {
            const int ih = ROWS * rq + ir;
            const bool ok = ih < H1 && iw < W1;
            const uint32_t di = (uint32_t)((b * H1 + ih) * W1 + iw) * 16 + 4 * lg;
            if constexpr (sizeof(T) == 2) {
              bf16x4 v;
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = (__bf16)acc[ir][r];
              buf_store8(rs.dp1, ok ? di * 2u : BUF_OOB, __builtin_bit_cast(uint64_t, v));
            } else {
              buf_store16(rs.dp1, ok ? di * 4u : BUF_OOB, acc[ir]);
            }
          }
        }
        if constexpr (FUSE) {
          // x window of pixel (row ir, column cl = 16 wv + lr) starts at x_s[2 ir][2 cl + 3]; position (dy, dx) moves it
          // by dy rows and dx columns: offset = dx + 256 dy = (pos * 129) & 0x101.  The 16 gathers of row ir+1 are issued
          // before the FMAs of row ir (register double buffer).
          const float* xcol = x_s + 2 * (16 * wv + lr) + 3;
          float xw[2][4][4];
          auto gather = [&](int ir, float (&xo)[4][4]) {
            const uint32_t pf = (uint32_t)codes[ir];                          // nibbles of channels 4lg..4lg+3
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t pos = (pf >> (4 * r)) & 3u;
              const float* xp = xcol + 2 * ir * XW + (XW == 256 ? ((pos * 129u) & 0x101u) : (pos & 1u) + XW * (pos >> 1));
              xo[r][0] = xp[0]; xo[r][1] = xp[1]; xo[r][2] = xp[XW]; xo[r][3] = xp[XW + 1];
            }
          };
          gather(0, xw[0]);
#pragma unroll
          for (int ir = 0; ir < 4; ++ir) {
            if (ir + 1 < 4) gather(ir + 1, xw[(ir + 1) & 1]);
            const uint32_t lv = (uint32_t)codes[ir];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t live = (uint32_t)((int32_t)(lv << (29 - 4 * r)) >> 31);        // bit 4r+2 -> 0 or ~0
              const float av = acc[ir][r];     // (bit_cast straight from a vector element reads element 0)
              const float g = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, av) & live);
#pragma unroll
              for (int q = 0; q < 4; ++q) a1[r][q] = fmaf(g, xw[ir & 1][r][q], a1[r][q]);
              bs[r] += g;
            }
          }
        }
      }
      STAMP(4);
    }
    __syncthreads();     // every wave is done with this step's LDS images
    STAMP(5);
  };
  while (p0.s < n_strips) {
    if constexpr (AHEAD2) {
      const Pos p2 = advance(p1);
      step(rg_a, p0, p2);
      const Pos p3 = advance(p2);
      if (p1.s < n_strips) step(rg_b, p1, p3);
      p0 = p2;
      p1 = p3;
    } else {
      step(rg_a, p0, p1);
      p0 = p1;
      p1 = advance(p1);
    }
  }
  STAMP_FLUSH;
  if constexpr (MF) {
    // S[c = 4lg + r][n = lr]: taps = columns 0..3 (+ their low-part twins 4..7), bias gradient = column 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = s1[r];
      const float tw = __shfl_down(v, 4, 64);          // lane lr + 4 of the same lane group (lr < 4: no wrap)
      if (lr < 4) red[wv * 80 + (4 * lg + r) * 4 + lr] = v + tw;
      if (lr == 8) red[wv * 80 + 64 + 4 * lg + r] = v;
    }
    __syncthreads();
    if (t < 80) slabs[(int64_t)blockIdx.x * 80 + t] = ((red[t] + red[80 + t]) + red[160 + t]) + red[240 + t];
  } else if constexpr (FUSE) {
    // one reduction per workgroup (not per tile): over the 16 lanes that share a channel group, then over the waves
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = a1[r][q];
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
        if (lr == 0) red[wv * 80 + (4 * lg + r) * 4 + q] = v;
      }
      float v = bs[r];
      v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
      if (lr == 0) red[wv * 80 + 64 + 4 * lg + r] = v;
    }
    __syncthreads();
    if (t < 80) slabs[(int64_t)blockIdx.x * 80 + t] = ((red[t] + red[80 + t]) + red[160 + t]) + red[240 + t];
  }
}

// 64-column items; 512 strips fill the chip at 2 resident workgroups per CU
inline SegPlan bwd_data_plan(int B, int H1, int W1, bool fuse) {
  return seg_plan(B, H1, W1, 512, BD_COLS, fuse ? cap::c2_bwd_fused() : cap::c2_bwd_data);
}

template <typename T, bool FUSE>
int launch_bwd_data(const void* dp2, const uint8_t* code2, const void* pack, int B, int H1, int W1, void* dp1,
                    const uint64_t* code1, const float* x0, const float* x1, int bsplit, int H, int W, float* slabs,
                    hipStream_t s) {
  const int H2 = H1 / 2, W2 = W1 / 2;
  const SegPlan pl = bwd_data_plan(B, H1, W1, FUSE);
  const size_t sm = BD<T>::lds_bytes(FUSE);
  // 16-byte x-window loads need rows that start on 16-byte boundaries
  const bool xvec = FUSE && W % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0;
#define GDM_BD_LAUNCH(XV, D1)                                                                                          \
  allow_lds(conv2_bwd_data_kernel<T, FUSE, XV, D1>, sm);                                                               \
  hipLaunchKernelGGL((conv2_bwd_data_kernel<T, FUSE, XV, D1>), dim3(pl.blocks), dim3(256), sm, s, (const T*)dp2, code2, \
                     (const T*)pack + C2<T>::WF_ELEMS, B, H1, W1, H2, W2, pl.n_ctiles, pl.nseg, pl.seg_len, pl.n_items, \
                     (T*)dp1, (const uint16_t*)code1, x0, x1, bsplit, H, W, slabs)
  if constexpr (FUSE) {
    if (dp1 != nullptr) {
      if (xvec) { GDM_BD_LAUNCH(true, true); } else { GDM_BD_LAUNCH(false, true); }
    } else {
      if (xvec) { GDM_BD_LAUNCH(true, false); } else { GDM_BD_LAUNCH(false, false); }
    }
  } else {
    GDM_BD_LAUNCH(false, true);
  }
#undef GDM_BD_LAUNCH
  GDM_LAUNCH_OK("gdm_simnn_conv2_bwd_data");
  return GDM_OK;
}
}  // namespace

extern "C" int gdm_simnn_conv2_bwd_data(const void* dp2, const uint8_t* code2, const void* pack, int B, int H1, int W1,
                                        void* dp1, int dtype, void* stream) {
  GDM_REQUIRE(dp2 && code2 && pack && dp1, "gdm_simnn_conv2_bwd_data: null pointer");
  GDM_REQUIRE(B > 0 && H1 >= 2 && W1 >= 2 && gdm_dtype_ok(dtype), "gdm_simnn_conv2_bwd_data: bad arguments");
  GDM_REQUIRE(fits_buffer_addressing(B, H1, W1), "gdm_simnn_conv2_bwd_data: batch of %d %dx%d maps exceeds 2 GiB per tensor", B, H1, W1);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_T(dtype, return (launch_bwd_data<T, false>(dp2, code2, pack, B, H1, W1, dp1, nullptr, nullptr, nullptr, 0, 0,
                                                      0, nullptr, s)));
}

extern "C" size_t gdm_simnn_conv2_bwd_fused_workspace_bytes(int B, int H1, int W1) {
  return (size_t)(bwd_data_plan(B, H1, W1, true).blocks + 65) * 80 * sizeof(float);
}

extern "C" int gdm_simnn_conv2_bwd_fused(const void* dp2, const uint8_t* code2, const void* pack, int B, int H1, int W1,
                                         const uint64_t* code1, const float* x0, const float* x1, int bsplit, int H,
                                         int W, void* dp1_or_null, int dtype, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  GDM_REQUIRE(dp2 && code2 && pack && code1 && x0, "gdm_simnn_conv2_bwd_fused: null pointer");
  GDM_REQUIRE(B > 0 && gdm_dtype_ok(dtype), "gdm_simnn_conv2_bwd_fused: bad arguments");
  GDM_REQUIRE(H1 == (H + 1) / 2 && W1 == (W + 1) / 2 && H1 >= 2 && W1 >= 2,
              "gdm_simnn_conv2_bwd_fused: (H1,W1)=(%d,%d) does not belong to a %dx%d input", H1, W1, H, W);
  GDM_REQUIRE(bsplit >= 0 && bsplit <= B && (bsplit == B || x1 != nullptr),
              "gdm_simnn_conv2_bwd_fused: second input pointer missing");
  GDM_REQUIRE(fits_buffer_addressing(B, H1, W1), "gdm_simnn_conv2_bwd_fused: batch of %d %dx%d maps exceeds 2 GiB per tensor",
              B, H1, W1);
  if (!workspace || workspace_bytes < gdm_simnn_conv2_bwd_fused_workspace_bytes(B, H1, W1)) {
    gdm_set_error("gdm_simnn_conv2_bwd_fused: workspace too small");
    return GDM_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* slabs = (float*)workspace;
  DISPATCH_T(dtype, return (launch_bwd_data<T, true>(dp2, code2, pack, B, H1, W1, dp1_or_null, code1, x0, x1, bsplit, H,
                                                     W, slabs, s)));
}

extern "C" int gdm_simnn_conv2_bwd_fused_finish(int B, int H1, int W1, float* dw1, float* db1, void* workspace,
                                                size_t workspace_bytes, void* stream) {
  GDM_REQUIRE(dw1 && db1 && B > 0 && H1 >= 2 && W1 >= 2, "gdm_simnn_conv2_bwd_fused_finish: bad arguments");
  if (!workspace || workspace_bytes < gdm_simnn_conv2_bwd_fused_workspace_bytes(B, H1, W1)) {
    gdm_set_error("gdm_simnn_conv2_bwd_fused_finish: workspace too small");
    return GDM_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = bwd_data_plan(B, H1, W1, true).blocks;
  float* slabs = (float*)workspace;
  float* scratch = slabs + (size_t)nblocks * 80;
  gdm_launch_slab_sum(1, slabs, nblocks, 80, scratch, dw1, db1, 0, s);
  GDM_LAUNCH_OK("gdm_simnn_conv2_bwd_fused_finish");
  return GDM_OK;
}

GDM_STAMP_READER(conv2_bwd_data)
