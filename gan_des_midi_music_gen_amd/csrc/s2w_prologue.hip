// The matrix prologue of the stand-alone demo (SIMULATOR/simulation_to_wav.py:25-71): a (size, size) float64 matrix ->
// what simulation_v3.Sim is constructed from.  It differs from matrix_to_wav's prologue (des_prologue.hip) in every
// constant, works in float64 on matrices of up to 256 x 256, draws nothing, and sums a row with Python's built-in
// sum() over ALL `size` entries -- after the source columns and the diagonal have been zeroed, the five parameter
// columns included, which a given matrix may fill.
//
// One workgroup of 256 threads per sample, one launch for the batch.  A 256 x 256 float64 sample is 512 KB and does not
// fit in LDS, so the sample is walked in strips of 16 columns: all threads load a (dim x 16) strip with the masks
// applied (128-byte row segments), then thread i continues ROW i's chain over the strip's 16 entries from LDS -- the
// sum stays the strictly sequential left-to-right float64 sum, dim chains run side by side, and the row stride of 17
// doubles keeps the lanes on different banks.  A second pass divides (IEEE) and writes the (dim, dim) routing matrix
// with coalesced loads and stores.  Nothing is contracted: no product feeds an add here, and contraction is off.
//
// Comparisons are made on bit patterns (the library is built with -fno-honor-nans): `x > 0.75` is false for a NaN, as
// in numpy, and a row sum is refused when it is zero of either sign, infinite or NaN.  No value read from the matrix
// forms an address.
#pragma clang fp contract(off)
#include "gdm_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxS = GDM_S2W_MAX_SIZE;
constexpr int kStrip = 16;
static_assert(kMaxS <= kThreads, "one thread per row and per column");

__device__ __forceinline__ uint64_t bits_of(double v) { return (uint64_t)__double_as_longlong(v); }

// x > 0.75 as numpy decides it: positive, above 0.75's pattern, not a NaN (+inf passes)
__device__ __forceinline__ bool above_threshold(double v) {
  const uint64_t u = bits_of(v);
  return (u >> 63) == 0 && u > 0x3FE8000000000000ULL && u <= 0x7FF0000000000000ULL;
}

__device__ __forceinline__ bool zero_or_nonfinite(double v) {
  const uint64_t u = bits_of(v) & 0x7FFFFFFFFFFFFFFFULL;
  return u == 0 || u >= 0x7FF0000000000000ULL;
}

// int(x * 127): truncation; v_cvt_i32_f64 saturates and turns a NaN into 0 where Python would raise
__device__ __forceinline__ int trunc127(double v) { return __double2int_rz(v * 127.0); }

__global__ __launch_bounds__(kThreads) void s2w_prologue_kernel(
    const double* __restrict__ m, int S, const int32_t* __restrict__ instrument_override, uint8_t* __restrict__ src,
    int32_t* __restrict__ instruments, int32_t* __restrict__ note_levels, double* __restrict__ loc,
    double* __restrict__ scale, int32_t* __restrict__ queue_cap, double* __restrict__ adj, int32_t* __restrict__ status) {
  __shared__ double tile[kMaxS][kStrip + 1];
  __shared__ double row_sum[kMaxS];
  __shared__ uint8_t col_src[kMaxS];
  __shared__ int bad;
  const int b = blockIdx.x, t = threadIdx.x, dim = S - 5;
  const double* mb = m + (int64_t)b * S * S;
  if (t == 0) bad = 0;
  col_src[t] = t < S ? (above_threshold(mb[(int64_t)dim * S + t]) ? 1 : 0) : 0;   // np.where(matrix[dim] > 0.75): all S
  __syncthreads();

  // ---- the row sums: `for i in sources: matrix[:, i] = 0`, the diagonal zeroed, then sum(matrix[i]) over S entries
  double acc = 0.0;                                   // Python's sum() starts from 0: 0 + (-0.0) is +0.0 here as well
  for (int c0 = 0; c0 < S; c0 += kStrip) {
    const int width = min(kStrip, S - c0);
    for (int k = t; k < dim * kStrip; k += kThreads) {
      const int r = k / kStrip, c = k % kStrip, col = c0 + c;
      double v = 0.0;
      if (c < width && !col_src[col] && col != r) v = mb[(int64_t)r * S + col];
      tile[r][c] = v;
    }
    __syncthreads();
    if (t < dim)
      for (int c = 0; c < width; ++c) acc = acc + tile[t][c];
    __syncthreads();
  }
  if (t < dim) {
    row_sum[t] = acc;
    if (zero_or_nonfinite(acc)) atomicOr(&bad, 1);
  }
  __syncthreads();
  const bool refused = bad != 0;

  // ---- per node: sources, instruments, note levels, the two distribution parameters, the queue capacity
  if (t < dim) {
    const int64_t o = (int64_t)b * dim + t;
    const bool is_src = col_src[t] != 0;
    const int over = instrument_override ? instrument_override[b] : INT_MIN;
    src[o] = is_src ? 1 : 0;
    instruments[o] = over != INT_MIN ? over : trunc127(mb[(int64_t)(dim + 1) * S + t]);
    note_levels[o] = trunc127(mb[(int64_t)(dim + 2) * S + t]);
    const double r3 = mb[(int64_t)(dim + 3) * S + t], r4 = mb[(int64_t)(dim + 4) * S + t];
    loc[o] = is_src ? 10.0 * r3 : 3.0 * r3;
    scale[o] = refused ? -1.0 : (is_src ? 5.0 * r4 : 2.0 * r4);     // -1: gdm_des_run_batch ends the sample with an error
    queue_cap[o] = 127;
  }
  if (t == 0) status[b] = refused ? 1 : 0;

  // ---- matrix[i] / sum(matrix[i]), diagonal +1 (source) / -1 (server), the first dim columns
  double* out = adj + (int64_t)b * dim * dim;
  for (int k = t; k < dim * dim; k += kThreads) {
    const int i = k / dim, x = k % dim;
    double v;
    if (x == i) v = col_src[i] ? 1.0 : -1.0;
    else if (refused) v = 0.0;                        // a refused sample: zeros, never a NaN whose bits are not defined
    else v = (col_src[x] ? 0.0 : mb[(int64_t)i * S + x]) / row_sum[i];
    out[k] = v;
  }
}

}  // namespace

extern "C" int gdm_s2w_prologue(const double* m, int B, int S, const int32_t* instrument_override_or_null, uint8_t* src,
                                int32_t* instruments, int32_t* note_levels, double* loc, double* scale,
                                int32_t* queue_cap, double* adj, int32_t* status, void* stream) {
  GDM_REQUIRE(m && src && instruments && note_levels && loc && scale && queue_cap && adj && status,
              "gdm_s2w_prologue: null pointer");
  GDM_REQUIRE(S >= GDM_S2W_MIN_SIZE && S <= GDM_S2W_MAX_SIZE, "gdm_s2w_prologue: size = %d (%d .. %d: 1 .. %d nodes)", S,
              GDM_S2W_MIN_SIZE, GDM_S2W_MAX_SIZE, GDM_S2W_MAX_SIZE - 5);
  GDM_REQUIRE(B >= 1, "gdm_s2w_prologue: B = %d (at least 1)", B);
  GDM_REQUIRE(((uintptr_t)m & 7) == 0 && ((uintptr_t)loc & 7) == 0 && ((uintptr_t)scale & 7) == 0 &&
                  ((uintptr_t)adj & 7) == 0 && ((uintptr_t)instruments & 3) == 0 && ((uintptr_t)note_levels & 3) == 0 &&
                  ((uintptr_t)queue_cap & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
                  ((uintptr_t)instrument_override_or_null & 3) == 0,
              "gdm_s2w_prologue: m / loc / scale / adj / instruments / note_levels / queue_cap / status / "
              "instrument_override must be aligned to their elements");
  hipLaunchKernelGGL(s2w_prologue_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, m, S,
                     instrument_override_or_null, src, instruments, note_levels, loc, scale, queue_cap, adj, status);
  GDM_LAUNCH_OK("gdm_s2w_prologue");
  return GDM_OK;
}
