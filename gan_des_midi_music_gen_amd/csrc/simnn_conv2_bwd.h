// What conv2's two backward kernels (simnn_conv2_bwd_data.hip, simnn_conv2_bwd_weight.hip) share and nobody else
// needs: the selector tables that turn code2's pair bytes back into the sparse full-resolution gradient.
#pragma once
#include "simnn_trunk.h"

// Selector tables for code2's pair bytes (bf16 kernels): entry e = c_even + 5 * c_odd at byte offset 8e of
//   table A: {selector for position 0, position 1}   table B: {position 2, position 3}   table C: {live channels, -}
// A selector moves the even channel's bf16 gradient (bytes 0,1 of the packed pair) and/or the odd channel's (bytes 2,3)
// to its place when that channel's argmax is the position, and writes zero (0x0c) otherwise.  25 entries x 8 B: two
// entries share a 16-byte LDS slot only 16 entries apart -> a table read is at most 2-way conflicted.  Table B sits
// more than 2040 bytes behind table A so that the compiler cannot merge the two 8-byte reads of a pair into one
// ds_read2_b64 (8 LDS cycles per wave instead of 2 + 2).
// Tables A' / B' hold the same selectors with the two pooling COLUMNS swapped ({position 1, 0} / {3, 2}): lanes whose
// pooled pixel has an odd column index expand through them and store their first record one column to the right, their
// second one to the left -- two neighbouring pooled pixels (128 bytes apart in a 64-byte-record image, i.e. on the same
// 32 store banks) then hit opposite halves of the bank window: every expansion ds_write_b128 was 2-way conflicted.
// (A' is shifted by 13 entries against A inside the 256-byte bank window: an A read and an A' read of the same half-wave
// then collide only for entry pairs (e, e + 13), not for equal entries -- "both channels dead" is by far the most common.)
constexpr int C2T_SWAP = 256 + 104, C2T_C = 576, C2T_B = 2304, C2T_BYTES = (C2T_B + C2T_SWAP + 256 + 15) / 16 * 16;
static_assert(C2T_BYTES % 16 == 0, "what follows the tables in LDS is read with 16-byte accesses (a misaligned "
                                   "ds_read_b128 is replayed at 64 cycles per wave instruction: the kernel ran 45 % slower)");
__device__ __forceinline__ void code2_tables_init(uint32_t* tab) {
  const int e = threadIdx.x;
  if (e < 25) {
    const uint32_t c0 = e % 5, c1 = e / 5;
    auto sel = [&](uint32_t pos) { return (c0 == pos ? 0x0100u : 0x0c0cu) | (c1 == pos ? 0x03020000u : 0x0c0c0000u); };
    tab[2 * e] = sel(0); tab[2 * e + 1] = sel(1);
    tab[C2T_B / 4 + 2 * e] = sel(2); tab[C2T_B / 4 + 2 * e + 1] = sel(3);
    tab[C2T_SWAP / 4 + 2 * e] = sel(1); tab[C2T_SWAP / 4 + 2 * e + 1] = sel(0);
    tab[(C2T_B + C2T_SWAP) / 4 + 2 * e] = sel(3); tab[(C2T_B + C2T_SWAP) / 4 + 2 * e + 1] = sel(2);
    tab[C2T_C / 4 + 2 * e] = (c0 != 4 ? 0x0100u : 0x0c0cu) | (c1 != 4 ? 0x03020000u : 0x0c0c0000u);
    tab[C2T_C / 4 + 2 * e + 1] = 0x0c0c0c0cu;
  }
}
// the four position-masked copies of one packed channel pair gw whose pair byte is `off8` (already a table offset)
__device__ __forceinline__ void code2_expand_pair(const unsigned char* tab, uint32_t off8, uint32_t gw, uint32_t (&out)[4]) {
  const u32x2 sa = *(const u32x2*)(tab + off8), sb = *(const u32x2*)(tab + C2T_B + off8);
  out[0] = __builtin_amdgcn_perm(0u, gw, sa[0]);
  out[1] = __builtin_amdgcn_perm(0u, gw, sa[1]);
  out[2] = __builtin_amdgcn_perm(0u, gw, sb[0]);
  out[3] = __builtin_amdgcn_perm(0u, gw, sb[1]);
}
// fp32 kernels: the two channel codes of a pair byte
__device__ __forceinline__ void code2_pair_codes(uint32_t byte8, uint32_t& c_even, uint32_t& c_odd) {
  const uint32_t n = byte8 >> 3;            // 0..24
  c_odd = (n * 13u) >> 6;                   // n / 5
  c_even = n - 5u * c_odd;
}
