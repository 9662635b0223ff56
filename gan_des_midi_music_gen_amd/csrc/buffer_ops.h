// Buffer-descriptor memory access, the transposing LDS read and the dynamic-LDS launch helper shared by the .hip files.
#pragma once
#include "gdm_common.h"

// Tile staging goes through buffer descriptors: a lane that falls outside the image hands the load an offset past
// num_records and the hardware returns zeros (stores are dropped), so halo handling needs no branch and no select.
// Branch-free staging matters twice: the loads of a tile issue back to back, and hipcc's s_waitcnt bookkeeping stays
// exact (with loads inside exec-masked branches it drained the whole queue -- vmcnt(0) -- right after issuing a
// prefetch, which turned "prefetch" into "wait").  All tensors addressed this way are < 2 GiB (checked on the host).
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr uint32_t BUF_OOB = 0x80000000u;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  // descriptor words must be provably wave-uniform, or every buffer op gets wrapped in a waterfall loop
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0,
                                           __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// AUX = cache policy of the access (0 default, 2 non-temporal)
template <int AUX = 0>
__device__ __forceinline__ f32x4 buf_load16(rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ uint64_t buf_load8(rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ float buf_load4(rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ void buf_store16(rsrc_t r, uint32_t off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_store8(rsrc_t r, uint32_t off, uint64_t v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, off, 0, AUX);
}
__device__ __forceinline__ void buf_store4(rsrc_t r, uint32_t off, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b32(v, r, off, 0, 0);
}
template <int AUX = 0>
__device__ __forceinline__ void buf_store2(rsrc_t r, uint32_t off, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, r, off, 0, AUX);
}

// ds_read_b64_tr_b16: the hardware transpose for operands whose contraction index is the slow axis of the LDS image
__device__ __forceinline__ bf16x4 lds_tr16(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
}

// Raise a kernel's dynamic-LDS limit once per kernel and process (not a stream operation: kept out of graph capture
// by doing it on the first, un-captured launch only; the size per kernel never changes).  Keyed by the kernel's
// address: template instantiations that share a signature share K.
template <typename K>
inline void allow_lds(K kernel, size_t bytes) {
  static const void* done[16];
  static int n_done = 0;
  for (int i = 0; i < n_done; ++i)
    if (done[i] == (const void*)kernel) return;
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (n_done < 16) done[n_done++] = (const void*)kernel;
}
