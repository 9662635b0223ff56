// The trunk's fixed-order slab sum (simnn_trunk.h: gdm_launch_slab_sum), launched by conv1's and conv2's weight
// gradients and by the fused conv2 backward's _finish.
#include "simnn_trunk.h"

namespace {

// =====================================================================================================================
// Fixed-order sum of `nslabs` slabs of `width` floats (deterministic replacement for float atomics), with the
// gradient's final placement fused into the last level.
// A 1024-thread workgroup owns 64 consecutive elements of one slab group; wave w adds slabs w, w+16, ... of its group
// (coalesced 256-B rows), the 16 partials are added in wave order.  Wide slabs (conv2's 4640 floats x up to 1024 slabs)
// take two levels (groups of <= 256 slabs, then the group partials in order); 80-float slabs take one launch.
// SINK: 0 = out[group][i];  1 = conv1 gradients (dw[64], db[16], optional accumulate);  2 = conv2 gradients
// (slab order [o 32][tap 9][ci 16] -> dw[o][ci][tap], then db[32]).
// =====================================================================================================================
template <int SINK>
__global__ __launch_bounds__(1024) void slab_sum_kernel(const float* __restrict__ slabs, int nslabs, int per_group,
                                                        int width, float* __restrict__ out, float* __restrict__ dw,
                                                        float* __restrict__ db, int accumulate) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int k0 = blockIdx.y * per_group, k1 = min(nslabs, k0 + per_group);
  // wave wv adds slabs k0 + wv + 16 j; eight independent partial sums so that eight row loads are in flight at once
  float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < width) {
    int k = k0 + wv;
    for (; k + 16 * 7 < k1; k += 16 * 8) {
#pragma unroll
      for (int q = 0; q < 8; ++q) s8[q] += slabs[(int64_t)(k + 16 * q) * width + i];
    }
    for (; k < k1; k += 16) s8[0] += slabs[(int64_t)k * width + i];      // (no run-time register index)
  }
  part[wv][lane] = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
  __syncthreads();
  if (wv == 0 && i < width) {
    float t = part[0][lane];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += part[w][lane];
    if constexpr (SINK == 0) {
      out[(int64_t)blockIdx.y * width + i] = t;
    } else if constexpr (SINK == 1) {
      float* dst = i < 64 ? dw + i : db + (i - 64);
      *dst = accumulate ? *dst + t : t;
    } else {
      if (i < 4608) {
        const int ci = i & 15, tap = (i >> 4) % 9, o = i / 144;
        dw[(o * 16 + ci) * 9 + tap] = t;
      } else {
        db[i - 4608] = t;
      }
    }
  }
}

// sums `nslabs` slabs into their sink using `scratch` (>= slab_groups(nslabs, width) * width floats)
inline int slab_groups(int nslabs, int width) {
  if (width <= 128 || nslabs <= 64) return 1;
  const int g = (nslabs + 255) / 256;
  return g > 64 ? 64 : g;
}

template <int SINK>
void launch(const float* slabs, int nslabs, int width, float* scratch, float* dw, float* db, int accumulate,
            hipStream_t s) {
  const int groups = slab_groups(nslabs, width);
  const int per = (nslabs + groups - 1) / groups;
  const unsigned gx = (unsigned)((width + 63) / 64);
  if (groups == 1) {
    hipLaunchKernelGGL(slab_sum_kernel<SINK>, dim3(gx, 1), dim3(1024), 0, s, slabs, nslabs, per, width, (float*)nullptr,
                       dw, db, accumulate);
  } else {
    hipLaunchKernelGGL(slab_sum_kernel<0>, dim3(gx, groups), dim3(1024), 0, s, slabs, nslabs, per, width, scratch,
                       (float*)nullptr, (float*)nullptr, 0);
    hipLaunchKernelGGL(slab_sum_kernel<SINK>, dim3(gx, 1), dim3(1024), 0, s, (const float*)scratch, groups, groups, width,
                       (float*)nullptr, dw, db, accumulate);
  }
}

}  // namespace

void gdm_launch_slab_sum(int sink, const float* slabs, int nslabs, int width, float* scratch, float* dw, float* db,
                         int accumulate, hipStream_t s) {
  if (sink == 1) launch<1>(slabs, nslabs, width, scratch, dw, db, accumulate, s);
  else launch<2>(slabs, nslabs, width, scratch, dw, db, accumulate, s);
}
