// What the two readers of a DES log (des_midi.hip, des_notes.hip) decide the same way.
#pragma once
#include "gdm_common.h"

// Python's % on integers (result takes the divisor's sign)
__device__ __forceinline__ int64_t pymod(int64_t a, int64_t m) {
  int64_t r = a % m;
  if (r != 0 && ((r < 0) != (m < 0))) r += m;
  return r;
}

// Does the reference reader's regex match the record's line?  It does iff kind is arrival / departure, the integers
// (event id, node) print without a sign and repr(value) is plain digits: +0.0 or 1e-4 <= value < 1e16.  Non-negative
// doubles order like their bit patterns, so the test is on the value's `bits`; `upper` is the caller's upper bound (at
// most 1e16's bits).
constexpr uint64_t kDesBits1em4 = 0x3F1A36E2EB1C432DULL;      // 1e-4
constexpr uint64_t kDesBits1e16 = 0x4341C37937E08000ULL;      // 1e16
__device__ __forceinline__ bool des_line_matches(int kind, int64_t id, int node, uint64_t bits, uint64_t upper) {
  return (kind == 0 || kind == 1) && id >= 0 && node >= 0 && (bits == 0 || (bits >= kDesBits1em4 && bits < upper));
}
