// Mel-spectrogram featuriser (reference GAN_DES/util.py:37-61 -> torchaudio MelSpectrogram + AmplitudeToDB): the step
// that produces model 1's discriminator input.  The two contractions (DFT and mel filter bank) are fp32 GEMMs
// (gdm_gemm, exact-fp32 MFMA); this file holds the three data-movement / pointwise kernels around them.
#include "buffer_ops.h"

namespace {

// Centred STFT frames with reflect padding:  out[(b * frames + f)][n] = x_b[reflect(f * hop + n - n_fft / 2)].
// (The Hann window is folded into the DFT matrix on the host.)  Four consecutive n per lane: 16-byte stores.
__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ x, int64_t L, int64_t x_stride,
                                                          int hop, int n_fft, int frames, int64_t total4,
                                                          float* __restrict__ out) {
  const int per_row = n_fft / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i % per_row) * 4;
    const int64_t row = i / per_row;
    const int f = (int)(row % frames);
    const int64_t b = row / frames;
    const float* xb = x + b * x_stride;
    const int64_t s0 = (int64_t)f * hop + n - n_fft / 2;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int64_t s = s0 + e;
      s = s < 0 ? -s : s;
      s = s >= L ? 2 * (L - 1) - s : s;
      v[e] = xb[s];
    }
    *(f32x4*)(out + row * n_fft + n) = v;
  }
}

// c (rows, 2 * nfreq) = [re | im]  ->  p (rows, ldp) = re^2 + im^2 (columns nfreq .. ldp-1 are written as zeros)
__global__ __launch_bounds__(256) void power_spectrum_kernel(const float* __restrict__ c, int64_t rows, int nfreq,
                                                             int ldp, float* __restrict__ p) {
  const int64_t total = rows * ldp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % ldp);
    const int64_t r = i / ldp;
    float v = 0.f;
    if (k < nfreq) {
      const float re = c[r * 2 * nfreq + k], im = c[r * 2 * nfreq + nfreq + k];
      v = re * re + im * im;
    }
    p[i] = v;
  }
}

// NaN as torch.clamp / amax / maximum treat it (AmplitudeToDB): it passes the amin clamp and takes over the window maximum,
// hence the floor.  The library is built with -fno-honor-nans -- fmaxf drops a NaN operand and a float select may assume
// there is none -- so NaN is told by its bits and chosen among bit patterns; NaN-free values take the fmaxf they always took.
__device__ __forceinline__ uint32_t f2u(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ bool nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ float max_nan(float a, float b) {
  const uint32_t ua = f2u(a), ub = f2u(b), um = f2u(fmaxf(a, b));
  return __builtin_bit_cast(float, nan_bits(ua) ? ua : nan_bits(ub) ? ub : um);
}

// One workgroup per window: mel (frames, n_mels) -> dB, raised to (window max - top_db), written as (n_mels, frames).
__global__ __launch_bounds__(1024) void power_to_db_kernel(const float* __restrict__ mel, int frames, int n_mels,
                                                           float top_db, float amin, float* __restrict__ out) {
  extern __shared__ float db_s[];              // [n_mels][frames + 1] (padded: transposed write without bank conflicts)
  __shared__ float red[16];
  const int t = threadIdx.x, n = frames * n_mels, ld = frames + 1;
  const float* m = mel + (int64_t)blockIdx.x * n;
  float mx = -INFINITY;
  for (int i = t; i < n; i += 1024) {
    const int f = i / n_mels, k = i % n_mels;              // coalesced read along the mel axis
    const float p = m[i];
    const uint32_t up = f2u(p), ud = f2u(10.0f * log10f(fmaxf(p, amin)));
    const float d = __builtin_bit_cast(float, nan_bits(up) ? up : ud);
    db_s[k * ld + f] = d;
    mx = max_nan(mx, d);
  }
  for (int o = 32; o > 0; o >>= 1) mx = max_nan(mx, __shfl_xor(mx, o, 64));
  if ((t & 63) == 0) red[t >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = max_nan(mx, red[w]);
  const uint32_t um = f2u(mx), uf = f2u(top_db >= 0.f ? mx - top_db : -INFINITY);
  const float floor_db = __builtin_bit_cast(float, top_db >= 0.f && nan_bits(um) ? um : uf);
  float* o = out + (int64_t)blockIdx.x * n;
  for (int i = t; i < n; i += 1024) {
    const int k = i / frames, f = i % frames;              // coalesced write along the time axis
    o[i] = max_nan(db_s[k * ld + f], floor_db);
  }
}

// ---- PCM front end (GAN_DES/datasets.py:26-43, util.py:89-119: torchaudio.load(normalize=True) + the window loops) ----
// The file's interleaved little-endian sample bytes are decoded where they are read.  One fp32 per stored sample first,
// then the mono rule: channel c, or channels added left to right in fp32 and divided once (waveform.mean(dim=0)).
template <int FMT>
__device__ __forceinline__ float pcm_decode(const uint8_t* __restrict__ p, int64_t e) {
#pragma clang fp contract(off)
  if constexpr (FMT == GDM_PCM_U8) {
    return (float)((int)p[e] - 128) * 0x1p-7f;
  } else if constexpr (FMT == GDM_PCM_S16) {
    return (float)((const int16_t*)p)[e] * 0x1p-15f;
  } else if constexpr (FMT == GDM_PCM_S24) {
    const uint8_t* q = p + 3 * e;                              // no alignment to rely on: three byte loads
    const int32_t v = (int32_t)((uint32_t)q[0] << 8 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 24) >> 8;
    return (float)v * 0x1p-23f;
  } else if constexpr (FMT == GDM_PCM_S32) {
    return (float)((const int32_t*)p)[e] * 0x1p-31f;           // int -> float rounds to nearest even; the scale is exact
  } else {
    return ((const float*)p)[e];
  }
}

// MEAN: waveform.mean(dim=0); otherwise channel `mix` (InputSong's channel = 0)
template <int FMT, bool MEAN>
__device__ __forceinline__ float pcm_mono(const uint8_t* __restrict__ p, int channels, int mix, int64_t s) {
#pragma clang fp contract(off)
  const int64_t e = s * channels;
  if constexpr (!MEAN) {
    return pcm_decode<FMT>(p, e + mix);
  } else {
    float acc = pcm_decode<FMT>(p, e);
    for (int c = 1; c < channels; ++c) acc = acc + pcm_decode<FMT>(p, e + c);
    return acc / (float)channels;
  }
}

// out[t] = mono(first + t); four consecutive t per lane, one 16-byte store where all four exist and out allows it
template <int FMT, bool MEAN>
__global__ __launch_bounds__(256) void pcm_to_float_kernel(const uint8_t* __restrict__ pcm, int channels, int mix,
                                                           int64_t first, int64_t count, float* __restrict__ out) {
  const int64_t total4 = (count + 3) / 4;
  const bool wide = ((uintptr_t)out & 15) == 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i * 4;
    if (wide && t + 4 <= count) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = pcm_mono<FMT, MEAN>(pcm, channels, mix, first + t + e);
      *(f32x4*)(out + t) = v;
    } else {
      for (int64_t u = t; u < count && u < t + 4; ++u) out[u] = pcm_mono<FMT, MEAN>(pcm, channels, mix, first + u);
    }
  }
}

// stft_frames_kernel reading the song itself: window w starts at start0 + w * stride (w < n_regular) or at tail_start,
// and the reflection stays inside the window's win_len samples.
template <int FMT, bool MEAN>
__global__ __launch_bounds__(256) void pcm_stft_frames_kernel(const uint8_t* __restrict__ pcm, int channels, int mix,
                                                              int64_t start0, int64_t stride, int n_regular,
                                                              int64_t tail_start, int64_t L, int hop, int n_fft,
                                                              int frames, int64_t total4, float* __restrict__ out) {
  const int per_row = n_fft / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i % per_row) * 4;
    const int64_t row = i / per_row;
    const int f = (int)(row % frames);
    const int64_t w = row / frames;
    const int64_t start = w < n_regular ? start0 + w * stride : tail_start;
    const int64_t s0 = (int64_t)f * hop + n - n_fft / 2;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int64_t s = s0 + e;
      s = s < 0 ? -s : s;
      s = s >= L ? 2 * (L - 1) - s : s;
      v[e] = pcm_mono<FMT, MEAN>(pcm, channels, mix, start + s);
    }
    *(f32x4*)(out + row * n_fft + n) = v;
  }
}

inline unsigned blocks_for(int64_t total) {
  int64_t b = (total + 255) / 256;
  return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int gdm_stft_frames(const float* x, int B, int64_t L, int64_t x_stride, int hop, int n_fft, int frames,
                               float* out, void* stream) {
  GDM_REQUIRE(x && out, "gdm_stft_frames: null pointer");
  GDM_REQUIRE(B > 0 && hop > 0 && n_fft >= 4 && n_fft % 4 == 0 && frames > 0, "gdm_stft_frames: bad arguments");
  GDM_REQUIRE(L > n_fft / 2, "gdm_stft_frames: reflect padding needs more than n_fft/2 = %d samples, got %lld", n_fft / 2,
              (long long)L);
  GDM_REQUIRE((int64_t)(frames - 1) * hop <= L, "gdm_stft_frames: %d frames of hop %d exceed %lld samples", frames, hop,
              (long long)L);
  GDM_REQUIRE(((uintptr_t)out & 15) == 0, "gdm_stft_frames: output must be 16-byte aligned");
  const int64_t total4 = (int64_t)B * frames * (n_fft / 4);
  hipLaunchKernelGGL(stft_frames_kernel, dim3(blocks_for(total4)), dim3(256), 0, (hipStream_t)stream, x, L, x_stride, hop,
                     n_fft, frames, total4, out);
  GDM_LAUNCH_OK("gdm_stft_frames");
  return GDM_OK;
}

extern "C" int gdm_power_spectrum(const float* c, int64_t rows, int nfreq, int ldp, float* p, void* stream) {
  GDM_REQUIRE(c && p && rows > 0 && nfreq > 0 && ldp >= nfreq, "gdm_power_spectrum: bad arguments");
  hipLaunchKernelGGL(power_spectrum_kernel, dim3(blocks_for(rows * ldp)), dim3(256), 0, (hipStream_t)stream, c, rows,
                     nfreq, ldp, p);
  GDM_LAUNCH_OK("gdm_power_spectrum");
  return GDM_OK;
}

extern "C" int gdm_power_to_db(const float* mel, int B, int frames, int n_mels, float top_db, float amin, float* out,
                               void* stream) {
  GDM_REQUIRE(mel && out && B > 0 && frames > 0 && n_mels > 0 && amin > 0.f, "gdm_power_to_db: bad arguments");
  const size_t sm = (size_t)n_mels * (frames + 1) * sizeof(float);
  GDM_REQUIRE(sm <= 150 * 1024, "gdm_power_to_db: a %d x %d window does not fit the LDS staging (150 KB)", n_mels, frames);
  allow_lds(power_to_db_kernel, 150 * 1024);
  hipLaunchKernelGGL(power_to_db_kernel, dim3(B), dim3(1024), sm, (hipStream_t)stream, mel, frames, n_mels, top_db, amin,
                     out);
  GDM_LAUNCH_OK("gdm_power_to_db");
  return GDM_OK;
}

// format x mono rule -> kernel instance; LAUNCH(kernel template) expands to the 10-way switch once per entry point
#define GDM_PCM_DISPATCH(LAUNCH)                                                      \
  switch (fmt * 2 + (mix < 0)) {                                                      \
    case GDM_PCM_U8 * 2: LAUNCH(GDM_PCM_U8, false); break;                            \
    case GDM_PCM_U8 * 2 + 1: LAUNCH(GDM_PCM_U8, true); break;                         \
    case GDM_PCM_S16 * 2: LAUNCH(GDM_PCM_S16, false); break;                          \
    case GDM_PCM_S16 * 2 + 1: LAUNCH(GDM_PCM_S16, true); break;                       \
    case GDM_PCM_S24 * 2: LAUNCH(GDM_PCM_S24, false); break;                          \
    case GDM_PCM_S24 * 2 + 1: LAUNCH(GDM_PCM_S24, true); break;                       \
    case GDM_PCM_S32 * 2: LAUNCH(GDM_PCM_S32, false); break;                          \
    case GDM_PCM_S32 * 2 + 1: LAUNCH(GDM_PCM_S32, true); break;                       \
    case GDM_PCM_F32 * 2: LAUNCH(GDM_PCM_F32, false); break;                          \
    default: LAUNCH(GDM_PCM_F32, true); break;                                        \
  }

// what both PCM entry points ask of the buffer description (n_samples is bounded so that no byte index overflows)
static int pcm_check(const char* who, const void* pcm, int fmt, int channels, int mix, int64_t n_samples) {
  GDM_REQUIRE(pcm, "%s: null pointer", who);
  GDM_REQUIRE(fmt >= GDM_PCM_U8 && fmt <= GDM_PCM_F32, "%s: unknown sample format %d", who, fmt);
  GDM_REQUIRE(channels >= 1 && channels <= 8, "%s: %d channels (1 to 8 are supported)", who, channels);
  GDM_REQUIRE(mix >= -1 && mix < channels, "%s: mix = %d is neither -1 (mean) nor one of %d channels", who, mix, channels);
  GDM_REQUIRE(n_samples > 0 && n_samples <= ((int64_t)1 << 40), "%s: bad sample count %lld", who, (long long)n_samples);
  const int align = fmt == GDM_PCM_S16 ? 2 : (fmt == GDM_PCM_S32 || fmt == GDM_PCM_F32) ? 4 : 1;
  GDM_REQUIRE(((uintptr_t)pcm & (align - 1)) == 0, "%s: the sample buffer must be aligned to its %d-byte elements", who, align);
  return GDM_OK;
}

extern "C" int gdm_pcm_to_float(const void* pcm, int fmt, int channels, int mix, int64_t n_samples, int64_t first,
                                int64_t count, float* out, void* stream) {
  if (int rc = pcm_check("gdm_pcm_to_float", pcm, fmt, channels, mix, n_samples)) return rc;
  GDM_REQUIRE(out, "gdm_pcm_to_float: null pointer");
  GDM_REQUIRE(first >= 0 && count > 0 && first <= n_samples && count <= n_samples - first,
              "gdm_pcm_to_float: samples %lld .. +%lld are not within the %lld of the buffer", (long long)first,
              (long long)count, (long long)n_samples);
  const uint8_t* p = (const uint8_t*)pcm;
#define GDM_PCM_LAUNCH(F, M)                                                                                          \
  hipLaunchKernelGGL((pcm_to_float_kernel<F, M>), dim3(blocks_for((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, \
                     p, channels, mix, first, count, out)
  GDM_PCM_DISPATCH(GDM_PCM_LAUNCH)
#undef GDM_PCM_LAUNCH
  GDM_LAUNCH_OK("gdm_pcm_to_float");
  return GDM_OK;
}

extern "C" int gdm_pcm_stft_frames(const void* pcm, int fmt, int channels, int mix, int64_t n_samples, int64_t start0,
                                   int64_t stride, int n_regular, int64_t tail_start, int64_t win_len, int hop, int n_fft,
                                   int frames, float* out, void* stream) {
  if (int rc = pcm_check("gdm_pcm_stft_frames", pcm, fmt, channels, mix, n_samples)) return rc;
  GDM_REQUIRE(out, "gdm_pcm_stft_frames: null pointer");
  GDM_REQUIRE(hop > 0 && n_fft >= 4 && n_fft % 4 == 0 && frames > 0, "gdm_pcm_stft_frames: bad arguments");
  GDM_REQUIRE(win_len > n_fft / 2, "gdm_pcm_stft_frames: reflect padding needs more than n_fft/2 = %d samples, got %lld",
              n_fft / 2, (long long)win_len);
  GDM_REQUIRE((int64_t)(frames - 1) * hop <= win_len, "gdm_pcm_stft_frames: %d frames of hop %d exceed %lld samples",
              frames, hop, (long long)win_len);
  GDM_REQUIRE(win_len <= n_samples, "gdm_pcm_stft_frames: a window of %lld samples in a song of %lld", (long long)win_len,
              (long long)n_samples);
  const int64_t last_ok = n_samples - win_len;                  // the largest start a window may have
  const bool tail = tail_start >= 0;
  GDM_REQUIRE(n_regular >= 0 && (n_regular > 0 || tail), "gdm_pcm_stft_frames: no window");
  if (n_regular > 0) {
    GDM_REQUIRE(start0 >= 0 && start0 <= last_ok, "gdm_pcm_stft_frames: window 0 starts at %lld, outside 0 .. %lld",
                (long long)start0, (long long)last_ok);
    // |stride| <= n_samples <= 2^40 and n_regular < 2^31: the product below cannot overflow
    GDM_REQUIRE(stride >= -n_samples && stride <= n_samples, "gdm_pcm_stft_frames: stride %lld", (long long)stride);
    const int64_t end = start0 + (int64_t)(n_regular - 1) * stride;          // starts are linear in w: two ends suffice
    GDM_REQUIRE(end >= 0 && end <= last_ok, "gdm_pcm_stft_frames: window %d starts at %lld, outside 0 .. %lld",
                n_regular - 1, (long long)end, (long long)last_ok);
  }
  GDM_REQUIRE(!tail || tail_start <= last_ok, "gdm_pcm_stft_frames: the tail window starts at %lld, outside 0 .. %lld",
              (long long)tail_start, (long long)last_ok);
  GDM_REQUIRE(((uintptr_t)out & 15) == 0, "gdm_pcm_stft_frames: output must be 16-byte aligned");
  const int64_t total4 = ((int64_t)n_regular + (tail ? 1 : 0)) * frames * (n_fft / 4);
  const uint8_t* p = (const uint8_t*)pcm;
#define GDM_PCM_LAUNCH(F, M)                                                                                         \
  hipLaunchKernelGGL((pcm_stft_frames_kernel<F, M>), dim3(blocks_for(total4)), dim3(256), 0, (hipStream_t)stream, p, \
                     channels, mix, start0, stride, n_regular, tail_start, win_len, hop, n_fft, frames, total4, out)
  GDM_PCM_DISPATCH(GDM_PCM_LAUNCH)
#undef GDM_PCM_LAUNCH
  GDM_LAUNCH_OK("gdm_pcm_stft_frames");
  return GDM_OK;
}
