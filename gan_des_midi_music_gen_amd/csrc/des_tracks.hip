// 'Music' logs of B simulations -> queue tracks: per sample a matrix of "arrivals minus departures so far" with one
// column per tracked server and one row per logged event, what the reference's MMGAN_MIDI_DES/simlog_to_vid.ipynb
// (process_adjsim_log, its first cell) builds from logs/simulation.log before it animates it as a bar chart.
//
// The rule, per sample, over the first max_lines records of its log ('processing' records count towards max_lines and
// change nothing):
//   an 'arrival' at node n adds 1 to n's counter, a 'departure' subtracts 1; after each of the two, if the sum of all
//   counters is > 0, one row with the counters of the tracked servers (in the caller's column order) is appended;
//   row 0 is a row of zeros.
// A reneged arrival is never subtracted (the log has no record for it), so a full queue drifts upward: that is the
// notebook's number, kept.  One difference: the notebook's regular expression drops a line whose clock prints in
// exponent notation; here every record counts (the clock is not read at all).
// An arrival or departure at a node without a column (col_of_node < 0, the notebook's KeyError) sets status
// GDM_DES_TRACKS_ENODE and gives the sample zero rows; offsets outside the record arrays GDM_DES_TRACKS_EPTR.
//
// Two launches, because the number of rows is data: gdm_des_log_tracks_count (rows per sample and their exclusive scan)
// and, after the caller has read row_ptr[B] and allocated, gdm_des_log_tracks (the rows).  Both map one workgroup to a
// sample and walk its log in chunks of kThreads records: a block scan of the +-1 deltas gives the total after each
// record and with it the keep flag, a second scan of the flags the row.  The fill kernel then turns round: thread j
// owns COLUMN j (j + kThreads, ...), walks the chunk's (column, delta, row) tuples from LDS -- every lane reads the same
// word, a broadcast -- and carries its counter across chunks, so a kept row is written as S consecutive int32 by
// consecutive lanes.  No atomics; ordinary vector stores.
// Bounds: a record index stays inside [rec_ptr[b], rec_ptr[b + 1]) which is checked against n_records; node is checked
// against dim before it indexes col_of_node, a column against S, a row against the sample's row count and the
// sample's rows against n_rows_cap before anything is stored.
#include <vector>
#include "gdm_common.h"
#include "des_tracks.h"

static_assert(DES_TRACKS_ENODE == GDM_DES_TRACKS_ENODE, "status codes");

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / GDM_WAVE;
constexpr int kMaxDim = GDM_DES_TRACKS_MAX_DIM;

// inclusive scan of one value per thread over the workgroup (wave scans by shuffle, the wave totals through LDS);
// total = the sum over the workgroup.  Ends with a barrier: s_wave may be used again at once.
template <class T>
__device__ __forceinline__ T block_scan(T v, T* s_wave, T& total) {
  const int lane = threadIdx.x & (GDM_WAVE - 1), w = threadIdx.x / GDM_WAVE;
#pragma unroll
  for (int off = 1; off < GDM_WAVE; off <<= 1) {
    const T x = __shfl_up(v, off, GDM_WAVE);
    if (lane >= off) v += x;
  }
  if (lane == GDM_WAVE - 1) s_wave[w] = v;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const T x = s_wave[i];
    if (i < w) before += x;
    all += x;
  }
  __syncthreads();
  total = all;
  return v + before;
}

// the records of sample b the rule reads: [lo, lo + n); false: the offsets do not lie inside the record arrays
__device__ __forceinline__ bool sample_range(const int64_t* __restrict__ rec_ptr, int b, int64_t n_records,
                                             int64_t max_lines, int64_t& lo, int64_t& n) {
  lo = rec_ptr[b];
  const int64_t hi = rec_ptr[b + 1];
  if (lo < 0 || hi < lo || hi > n_records) return false;
  n = hi - lo < max_lines ? hi - lo : max_lines;
  return true;
}

// record i of the log: its delta (+1 arrival, -1 departure, 0 anything else) and its column; false: an arrival or a
// departure at a node without a column
__device__ __forceinline__ bool record_delta(const int32_t* __restrict__ node, const int32_t* __restrict__ kind,
                                             const int32_t* __restrict__ cols, int dim, int S, int64_t i, int& delta,
                                             int& col) {
  const int32_t kd = kind[i];
  delta = kd == 0 ? 1 : (kd == 1 ? -1 : 0);
  col = -1;
  if (delta == 0) return true;
  const int32_t nd = node[i];
  if (nd < 0 || nd >= dim) return false;
  col = cols[nd];
  return col >= 0 && col < S;
}

__global__ __launch_bounds__(kThreads) void des_tracks_count_kernel(
    const int32_t* __restrict__ node, const int32_t* __restrict__ kind, const int64_t* __restrict__ rec_ptr,
    int64_t n_records, int dim, const int32_t* __restrict__ col_of_node, int64_t max_lines,
    int64_t* __restrict__ n_rows, int32_t* __restrict__ status) {
  __shared__ int s_wave[kWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  int64_t lo, n;
  if (!sample_range(rec_ptr, b, n_records, max_lines, lo, n)) {        // uniform over the workgroup
    if (t == 0) {
      n_rows[b] = 0;
      status[b] = GDM_DES_TRACKS_EPTR;
    }
    return;
  }
  const int32_t* cols = col_of_node + (int64_t)b * dim;
  int total = 0, bad = 0;
  int64_t rows = 1;                                       // row 0
  for (int64_t base = 0; base < n; base += kThreads) {
    int delta = 0, col = -1;
    if (base + t < n && !record_delta(node, kind, cols, dim, INT32_MAX, lo + base + t, delta, col)) bad = 1;
    int chunk_sum, chunk_keep;
    const int after = total + block_scan(delta, s_wave, chunk_sum);
    const int keep = delta != 0 && after > 0;
    block_scan(keep, s_wave, chunk_keep);
    total += chunk_sum;
    rows += chunk_keep;
  }
  bad = __syncthreads_or(bad);
  if (t == 0) {
    n_rows[b] = bad ? 0 : rows;
    status[b] = bad ? GDM_DES_TRACKS_ENODE : 0;
  }
}

// n_rows -> row_ptr (exclusive scan, one workgroup)
__global__ __launch_bounds__(kThreads) void des_tracks_scan_kernel(int B, const int64_t* __restrict__ n_rows,
                                                                   int64_t* __restrict__ row_ptr) {
  __shared__ int64_t s_wave[kWaves];
  const int t = threadIdx.x;
  int64_t carry = 0;
  for (int base = 0; base < B; base += kThreads) {
    int64_t v = 0, sum;
    if (base + t < B) {
      v = n_rows[base + t];
      v = v < 0 ? 0 : v;
    }
    const int64_t incl = block_scan(v, s_wave, sum);
    if (base + t < B) row_ptr[base + t + 1] = carry + incl;
    carry += sum;
  }
  if (t == 0) row_ptr[0] = 0;
}

__global__ __launch_bounds__(kThreads) void des_tracks_fill_kernel(
    const int32_t* __restrict__ node, const int32_t* __restrict__ kind, const int64_t* __restrict__ rec_ptr,
    int64_t n_records, int dim, const int32_t* __restrict__ col_of_node, int S, int64_t max_lines,
    const int64_t* __restrict__ row_ptr, int64_t n_rows_cap, int32_t* __restrict__ tracks) {
  __shared__ int s_wave[kWaves];
  __shared__ int s_col[kThreads], s_delta[kThreads], s_row[kThreads];
  __shared__ int s_cnt[kMaxDim];                          // column j's counter between chunks: thread j % kThreads' own
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t row0 = row_ptr[b], n_own = row_ptr[b + 1] - row0;
  int64_t lo, n;
  // a sample without rows (an error sample), or rows that do not lie inside `tracks`: nothing is written (uniform)
  if (n_own <= 0 || row0 < 0 || row0 + n_own > n_rows_cap || n_own > max_lines + 1 ||
      !sample_range(rec_ptr, b, n_records, max_lines, lo, n))
    return;
  const int32_t* cols = col_of_node + (int64_t)b * dim;
  int32_t* out = tracks + row0 * S;
  for (int j = t; j < S; j += kThreads) {
    s_cnt[j] = 0;
    out[j] = 0;                                           // row 0
  }
  int total = 0, rows = 1;
  for (int64_t base = 0; base < n; base += kThreads) {
    int delta = 0, col = -1;
    if (base + t < n && !record_delta(node, kind, cols, dim, S, lo + base + t, delta, col)) delta = 0;
    int chunk_sum, chunk_keep;
    const int after = total + block_scan(delta, s_wave, chunk_sum);
    const int keep = delta != 0 && after > 0;
    const int row = rows + block_scan(keep, s_wave, chunk_keep) - 1;
    s_col[t] = delta != 0 ? col : -1;
    s_delta[t] = delta;
    s_row[t] = keep ? row : -1;
    __syncthreads();
    const int m = n - base < kThreads ? (int)(n - base) : kThreads;
    for (int j = t; j < S; j += kThreads) {
      int c = s_cnt[j];
      for (int k = 0; k < m; ++k) {
        if (s_col[k] == j) c += s_delta[k];
        const int r = s_row[k];
        if (r >= 0 && r < n_own) out[(int64_t)r * S + j] = c;
      }
      s_cnt[j] = c;
    }
    total += chunk_sum;
    rows += chunk_keep;
    __syncthreads();
  }
}

int check_tracks_args(const char* who, const int32_t* node, const int32_t* kind, const int64_t* rec_ptr,
                      int64_t n_records, int B, int dim, const int32_t* col_of_node, int64_t max_lines) {
  GDM_REQUIRE(rec_ptr && col_of_node && (n_records == 0 || (node && kind)), "%s: null pointer", who);
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && dim >= 1 && dim <= kMaxDim && n_records >= 0,
              "%s: 1 <= B <= 2^20, 1 <= dim <= %d, n_records >= 0", who, kMaxDim);
  GDM_REQUIRE(max_lines >= 0 && max_lines <= GDM_DES_TRACKS_MAX_LINES, "%s: max_lines must be in 0..%lld", who,
              (long long)GDM_DES_TRACKS_MAX_LINES);
  GDM_REQUIRE((((uintptr_t)node | (uintptr_t)kind | (uintptr_t)col_of_node) & 3) == 0 && ((uintptr_t)rec_ptr & 7) == 0,
              "%s: an array is not aligned to its element size", who);
  return GDM_OK;
}

}  // namespace

extern "C" int gdm_des_log_tracks_count(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr,
                                        int64_t n_records, int B, int dim, const int32_t* col_of_node,
                                        int64_t max_lines, int64_t* n_rows, int64_t* row_ptr, int32_t* status,
                                        void* stream) {
  const int rc = check_tracks_args("gdm_des_log_tracks_count", node, kind, rec_ptr, n_records, B, dim, col_of_node,
                                   max_lines);
  if (rc != GDM_OK) return rc;
  GDM_REQUIRE(n_rows && row_ptr && status, "gdm_des_log_tracks_count: null pointer");
  GDM_REQUIRE((((uintptr_t)n_rows | (uintptr_t)row_ptr) & 7) == 0 && ((uintptr_t)status & 3) == 0,
              "gdm_des_log_tracks_count: an array is not aligned to its element size");
  hipLaunchKernelGGL(des_tracks_count_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, node, kind, rec_ptr,
                     n_records, dim, col_of_node, max_lines, n_rows, status);
  GDM_LAUNCH_OK("gdm_des_log_tracks_count");
  hipLaunchKernelGGL(des_tracks_scan_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, B, n_rows, row_ptr);
  GDM_LAUNCH_OK("gdm_des_log_tracks_count");
  return GDM_OK;
}

extern "C" int gdm_des_log_tracks(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr, int64_t n_records,
                                  int B, int dim, const int32_t* col_of_node, int S, int64_t max_lines,
                                  const int64_t* row_ptr, int64_t n_rows_cap, int32_t* tracks, void* stream) {
  const int rc = check_tracks_args("gdm_des_log_tracks", node, kind, rec_ptr, n_records, B, dim, col_of_node, max_lines);
  if (rc != GDM_OK) return rc;
  GDM_REQUIRE(row_ptr && (tracks || n_rows_cap == 0), "gdm_des_log_tracks: null pointer");
  GDM_REQUIRE(S >= 1 && S <= dim && n_rows_cap >= 0 && n_rows_cap <= ((int64_t)1 << 40),
              "gdm_des_log_tracks: 1 <= S <= dim and 0 <= n_rows_cap <= 2^40");
  GDM_REQUIRE(((uintptr_t)row_ptr & 7) == 0 && ((uintptr_t)tracks & 3) == 0,
              "gdm_des_log_tracks: an array is not aligned to its element size");
  if (n_rows_cap == 0) return GDM_OK;
  hipLaunchKernelGGL(des_tracks_fill_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, node, kind, rec_ptr,
                     n_records, dim, col_of_node, S, max_lines, row_ptr, n_rows_cap, tracks);
  GDM_LAUNCH_OK("gdm_des_log_tracks");
  return GDM_OK;
}

// Both steps on host arrays, record by record as the notebook's loop: the device's oracle.
extern "C" int gdm_des_log_tracks_host(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr,
                                       int64_t n_records, int B, int dim, const int32_t* col_of_node, int S,
                                       int64_t max_lines, int64_t* n_rows, int64_t* row_ptr, int32_t* status,
                                       int32_t* tracks, int64_t n_rows_cap) {
  const int rc = check_tracks_args("gdm_des_log_tracks_host", node, kind, rec_ptr, n_records, B, dim, col_of_node,
                                   max_lines);
  if (rc != GDM_OK) return rc;
  GDM_REQUIRE(n_rows && row_ptr && status && (tracks || n_rows_cap == 0), "gdm_des_log_tracks_host: null pointer");
  GDM_REQUIRE(S >= 1 && S <= dim && n_rows_cap >= 0, "gdm_des_log_tracks_host: 1 <= S <= dim and n_rows_cap >= 0");
  std::vector<int32_t> cnt(S);
  std::vector<uint8_t> seen(S);
  for (int b = 0; b < B; ++b) {                           // the columns of a sample: inside 0..S-1, each at most once
    const int32_t* cols = col_of_node + (int64_t)b * dim;
    seen.assign(S, 0);
    for (int i = 0; i < dim; ++i) {
      GDM_REQUIRE(cols[i] >= -1 && cols[i] < S, "gdm_des_log_tracks_host: column %d at sample %d, node %d is outside -1..%d",
                  cols[i], b, i, S - 1);
      if (cols[i] < 0) continue;
      GDM_REQUIRE(!seen[cols[i]], "gdm_des_log_tracks_host: column %d is given twice at sample %d", cols[i], b);
      seen[cols[i]] = 1;
    }
  }
  int64_t at = 0;
  row_ptr[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t lo = rec_ptr[b], hi = rec_ptr[b + 1];
    int64_t rows = 0;
    int st = GDM_DES_TRACKS_EPTR;
    if (lo >= 0 && hi >= lo && hi <= n_records) {
      const int64_t room = n_rows_cap > at ? n_rows_cap - at : 0;
      rows = des_tracks::sample_rows(node, kind, lo, hi - lo < max_lines ? hi - lo : max_lines,
                                     col_of_node + (int64_t)b * dim, dim, S, cnt.data(),
                                     room > 0 ? tracks + at * S : nullptr, room, &st);
    }
    at += rows;
    n_rows[b] = rows;
    status[b] = st;
    row_ptr[b + 1] = at;
  }
  if (at > n_rows_cap && (tracks || n_rows_cap > 0)) {
    gdm_set_error("gdm_des_log_tracks_host: tracks too small (%lld rows needed)", (long long)at);
    return GDM_EWORKSPACE;
  }
  return GDM_OK;
}
