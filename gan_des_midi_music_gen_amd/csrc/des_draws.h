// The per-sample draws and parameters of the G -> DES bridges' prologue, for the "des_device" back end: what
// matrix_sim_process.py's _midi_draws / _wav_draws / _draw_residue_columns / _reseed draw from numpy's legacy stream and
// what _midi_spec / _wav_spec compute in float32 (MMGAN_MIDI_DES/matrix_sim_process.py:44, 72-74, 102, 114-115 and
// GAN_DES/matrix_sim_process.py:28, 30, 57-59, 67, 87, 105-106), ONE source for the host entry gdm_des_draws_host and the
// device kernel (des_draws.hip).  Compiles as host code, as gfx950 device code and as plain C++ without any HIP include.
//
// Every sample owns a stream: RandomState(base[b]) = init_genrand (des::seed_key of des_sim.h), position 624, no cached
// gauss.  On it, in this order (numpy 1.x / 2.x legacy RandomState, checked against numpy itself by
// tests/test_des_draws.py):
//   sources    choice(dim, size=k, replace=False) = permutation(dim)[:k]: a Fisher-Yates pass over arange(dim),
//              `for i in dim-1 .. 1: j = random_interval(i); swap(a[i], a[j])`.  The pass runs over ALL dim entries and
//              also when k == 0 (numpy slices afterwards), so its words are consumed whatever k is.  k = dim / 4 (MIDI
//              route) or S / 8 (wav route, only when no column of the source row passes the threshold).
//   interval   random_interval(max): 0 without a draw when max == 0, else the smallest mask 2^n - 1 >= max and 32-bit
//              words rejected while (word & mask) > max.
//   residue    row i's candidates are the columns that are not zero in the scan's zero_mask, not sources and not i, in
//              ascending order; choice(list) = list[randint(0, len)]: masked rejection on 32-bit words like
//              random_interval(len - 1), no word for a one-element list, ValueError for an empty one.  dim <= 64, so the
//              candidate set is one 64-bit word, its size a popcount and the drawn entry the k-th set bit.
//   reseed     s1 = randint(0, 99999) = random_interval(99998); seed(array([s1])) = init_genrand(s1) (numpy squeezes the
//              size-1 array to an integer); seeds = randint(0, 99999).
// The stream after the last draw is what the simulator starts from (as "des_batch" does with its snapshots).
//
// What raises in the reference is a status code here; such a sample gets zero src / cols / seed, its stream back at the
// post-init_genrand state of base[b], and scale -1 on every node, which des::Sim::spec_ok refuses: the simulator ends
// the sample with DES_STOP_ERROR and zero records.
//
// Every loop is bounded: each 32-bit word counts against a budget of DES_DRAW_FACTOR * (2 dim + 2) -- a healthy sample
// makes at most 2 dim + 1 interval draws, each accepted with p > 1/2 -- and every index is checked before it forms an
// address.
#pragma once
#include "des_sim.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define DES_DRAWS_OK 0
#define DES_DRAWS_EMPTY 1          /* np.random.choice([]): ValueError */
#define DES_DRAWS_MULTI_SOURCE 2   /* wav route: more than one thresholded source: ValueError (line 30) */
#define DES_DRAWS_SOURCE_RANGE 3   /* wav route: a thresholded column >= dim: IndexError (line 67) */
#define DES_DRAWS_BUDGET 4         /* draw budget exhausted */
#define DES_DRAWS_CUSTOMERS 5      /* MIDI route: int(3000 * p[6]) of a NaN / inf / beyond int64: ValueError / OverflowError */
#define DES_DRAWS_ROUTE_MIDI 0
#define DES_DRAWS_ROUTE_WAV 1
#define DES_DRAWS_MAX_DIM 64
#define DES_DRAWS_QUEUE_CAP 254    /* queue_list = [2 * 127] * dim */
#define DES_DRAWS_NO_INSTRUMENT (-2147483647 - 1)   /* instrument override: "None" */

namespace des {

struct DrawStream {
  uint32_t* key;              // 624 words
  int32_t pos;
  int64_t draws_left;
  int status;

  DES_HD void seed(uint32_t s) {
    seed_key(key, s);
    pos = DES_MT_N;
  }
  DES_HD uint32_t next32() {
    if (draws_left <= 0) {
      if (!status) status = DES_DRAWS_BUDGET;
      return 0;
    }
    --draws_left;
    uint32_t p = (uint32_t)pos;
    if (p >= DES_MT_N) {                              // (an out-of-range position cannot form an address)
      Sim<MathPortable, OutSoa>::twist(key);
      p = 0;
    }
    uint32_t y = key[p];
    pos = (int32_t)(p + 1);
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
  DES_HD uint32_t interval(uint32_t max) {
    if (max == 0) return 0;
    uint32_t mask = max;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v;
    do { v = next32() & mask; } while (v > max && !status);
    return status ? 0 : v;
  }
};

DES_HD inline int popcount64(uint64_t x) {
  x = x - ((x >> 1) & 0x5555555555555555ULL);
  x = (x & 0x3333333333333333ULL) + ((x >> 2) & 0x3333333333333333ULL);
  x = (x + (x >> 4)) & 0x0f0f0f0f0f0f0f0fULL;
  return (int)((x * 0x0101010101010101ULL) >> 56);
}
// index of the k-th (0-based) set bit of x; 64 when x has no more than k bits
DES_HD inline int select64(uint64_t x, int k) {
  for (int n = 0; n < k && x; ++n) x &= x - 1;       // at most 63 rounds
  if (!x) return 64;
  int i = 0;
  while (!((x >> i) & 1) && i < 63) ++i;
  return i;
}
DES_HD inline uint64_t low_bits(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1); }

// The dependent chain of one sample.  zero_mask: dim words; thr: S flags (wav route) or null; key: 624 words of
// storage; perm: dim bytes of scratch; src, cols: dim entries; pre_status: a status found before the chain (the sample
// then draws nothing).  Returns the status; pos_out is the stream position.
DES_HD inline int draw_chain(int route, int dim, int S, uint32_t base, int pre_status, const uint64_t* zero_mask,
                             const uint8_t* thr, uint32_t* key, int32_t* pos_out, uint8_t* perm, uint8_t* src,
                             int32_t* cols, int64_t* seed_out) {
  DrawStream st;
  st.key = key;
  st.draws_left = (int64_t)DES_DRAW_FACTOR * (2 * dim + 2);
  st.status = pre_status;
  st.seed(base);
  uint64_t src_bits = 0;
  int n_random = dim / 4;
  if (!st.status && route == DES_DRAWS_ROUTE_WAV) {
    n_random = S / 8;
    int hits = 0, hit = -1;
    if (thr)
      for (int x = 0; x < S; ++x)
        if (thr[x]) { ++hits; hit = x; }
    if (hits > 1) st.status = DES_DRAWS_MULTI_SOURCE;
    else if (hits == 1) {
      n_random = -1;
      if (hit >= dim) st.status = DES_DRAWS_SOURCE_RANGE;
      else src_bits = 1ULL << hit;
    }
  }
  if (!st.status && n_random >= 0) {
    for (int i = 0; i < dim; ++i) perm[i] = (uint8_t)i;
    for (int i = dim - 1; i >= 1 && !st.status; --i) {
      const uint32_t j = st.interval((uint32_t)i);
      if (j > (uint32_t)i) { if (!st.status) st.status = DES_DRAWS_BUDGET; break; }
      const uint8_t t = perm[i];
      perm[i] = perm[j];
      perm[j] = t;
    }
    for (int i = 0; i < n_random && i < dim && !st.status; ++i) src_bits |= 1ULL << (perm[i] & 63);
  }
  const uint64_t all = low_bits(dim);
  for (int i = 0; i < dim && !st.status; ++i) {
    const uint64_t cand = ~zero_mask[i] & ~src_bits & ~(1ULL << i) & all;
    const int n = popcount64(cand);
    if (n == 0) { st.status = DES_DRAWS_EMPTY; break; }
    const uint32_t k = st.interval((uint32_t)(n - 1));
    const int c = select64(cand, (int)k);
    if (st.status) break;
    if (c >= dim) { st.status = DES_DRAWS_BUDGET; break; }
    cols[i] = c;
  }
  int64_t seeds = 0;
  if (!st.status) {
    const uint32_t s1 = st.interval(99998u);
    if (!st.status) {
      st.seed(s1);
      seeds = (int64_t)st.interval(99998u);
    }
  }
  if (st.status) {                                    // defined values for a refused sample
    st.seed(base);
    src_bits = 0;
    seeds = 0;
    for (int i = 0; i < dim; ++i) cols[i] = 0;
  }
  for (int i = 0; i < dim; ++i) src[i] = (uint8_t)((src_bits >> i) & 1);
  *seed_out = seeds;
  *pos_out = st.pos;
  return st.status;
}

// ---- the float32 arithmetic of _midi_spec / _wav_spec, widened exactly like float(np.float32) ----
DES_HD inline uint32_t fbits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
DES_HD inline float fabs_bits(float x) {              // np.abs: the sign bit cleared (built with -fno-honor-nans)
  uint32_t u = fbits(x) & 0x7fffffffu;
  float r;
  __builtin_memcpy(&r, &u, 4);
  return r;
}
// p: the sample's gen2 row (at least 7 entries): np.abs(p[1] * 50), np.abs(p[2] * 50) / np.abs(p[3] * 10), np.abs(p[4] * 10)
DES_HD inline void midi_node(const float* p, bool is_src, double* loc, double* scale) {
  const float l = is_src ? p[1] * 50.0f : p[3] * 10.0f, s = is_src ? p[2] * 50.0f : p[4] * 10.0f;
  *loc = (double)fabs_bits(l);
  *scale = (double)fabs_bits(s);
}
// 30 * r3, 15 * r4 / 5 * r3, 3 * r4 on the two normalised rows of the scan
DES_HD inline void wav_node(float r3, float r4, bool is_src, double* loc, double* scale) {
  *loc = (double)(is_src ? 30.0f * r3 : 5.0f * r3);
  *scale = (double)(is_src ? 15.0f * r4 : 3.0f * r4);
}
// max(200, max(1000, int(3000 * p[6]))): float32 product, truncation; DES_DRAWS_CUSTOMERS where Python raises
DES_HD inline int midi_customers(float p6, int64_t* out) {
  const float x = 3000.0f * p6;
  *out = 1000;
  if ((fbits(x) & 0x7f800000u) == 0x7f800000u) return DES_DRAWS_CUSTOMERS;
  if (!(fabs_bits(x) < 9223372036854775808.0f)) return DES_DRAWS_CUSTOMERS;
  int64_t c = (int64_t)x;
  if (c < 1000) c = 1000;
  if (c < 200) c = 200;
  *out = c;
  return DES_DRAWS_OK;
}

// Per-node outputs of sample-local node i once the chain's status is known
DES_HD inline void node_outputs(int route, int i, int dim, const float* params, bool is_src, int status,
                                int32_t scan_instrument, int32_t scan_note, int32_t instrument_override, double* loc,
                                double* scale, int32_t* queue_cap, int32_t* instrument, int32_t* note_level) {
  double l, s;
  if (route == DES_DRAWS_ROUTE_MIDI) midi_node(params, is_src, &l, &s);
  else wav_node(params[i], params[dim + i], is_src, &l, &s);
  *loc = l;
  *scale = status ? -1.0 : s;                         // spec_ok refuses the sample: DES_STOP_ERROR, zero records
  *queue_cap = DES_DRAWS_QUEUE_CAP;
  *instrument = instrument_override == DES_DRAWS_NO_INSTRUMENT ? scan_instrument : instrument_override;
  *note_level = scan_note;
}

}  // namespace des
