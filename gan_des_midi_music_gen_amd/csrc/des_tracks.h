// The queue-track rule of des_tracks.hip for ONE log on the host, record by record as the reference notebook's loop:
// what gdm_des_log_tracks_host runs per sample and tools/des_log_dist_host.cpp runs under the host sanitizers.  Plain
// C++, no HIP.
#pragma once
#include <cstdint>

#define DES_TRACKS_ENODE 1 /* an arrival or departure at a node without a column */

namespace des_tracks {

// Records [lo, lo + n) of node / kind; cols (dim): the column of a node, -1 = not tracked; cnt (S): scratch.  Row r of
// the sample is written to rows + r * S while r < rows_cap (rows may be null with rows_cap 0: the rows are counted
// only).  Returns the number of rows (row 0, the zeros, included); *status = DES_TRACKS_ENODE and 0 rows for a record
// at a node without a column.
inline int64_t sample_rows(const int32_t* node, const int32_t* kind, int64_t lo, int64_t n, const int32_t* cols, int dim,
                           int S, int32_t* cnt, int32_t* rows, int64_t rows_cap, int* status) {
  *status = 0;
  for (int j = 0; j < S; ++j) cnt[j] = 0;
  int64_t total = 0, r = 0;
  auto put = [&]() {
    if (r < rows_cap)
      for (int j = 0; j < S; ++j) rows[r * S + j] = cnt[j];
    ++r;
  };
  put();
  for (int64_t i = lo; i < lo + n; ++i) {
    const int delta = kind[i] == 0 ? 1 : (kind[i] == 1 ? -1 : 0);
    if (delta == 0) continue;
    const int32_t nd = node[i];
    if (nd < 0 || nd >= dim || cols[nd] < 0 || cols[nd] >= S) {
      *status = DES_TRACKS_ENODE;
      return 0;
    }
    cnt[cols[nd]] += delta;
    total += delta;
    if (total > 0) put();
  }
  return r;
}

}  // namespace des_tracks
