// The integer synth of model 1's DES bridge: note lists -> the mel featuriser's STFT frame matrix (gdm_synth_frames) or
// 16-bit PCM (gdm_synth_pcm).  It stands where the reference renders its MIDI file through FluidSynth and loads the WAV
// again (GAN_DES/matrix_sim_process.py:114-129); FluidSynth's sound font is not imitated -- the synth is DEFINED here
// (include/gdm.h) and is integer only, so that a numpy mirror can demand equal bits.
//
// A voice (s_on, s_off, pitch p, velocity v) contributes at sample s in [s_on, s_off + R):
//   phase = uint32(inc[p] * (s - s_on));  e_att = min(s - s_on + 1, A);  e_rel = s < s_off ? R : R - (s - s_off)
//   voice = (int64(wave[phase >> 21]) * v * e_att * e_rel) >> SHIFT                     (arithmetic shift)
// and a sample is the int32 sum of its voices clamped to the 16-bit range.
//
// Both kernels work on 2048 output samples per workgroup.  The clips are minutes long and the 216 frames of a clip read
// about a tenth of it, so whole clips are never rendered: a workgroup first COMPACTS the notes that overlap the sample
// range it will touch into LDS (all threads scan the clip's list; the integer sum does not depend on the order, so the
// slots are dealt by an LDS atomic counter), rebased to the range's first sample so that everything after is 32-bit.
// Then every thread produces 8 samples -- the voices in the outer loop, the 8 running sums in registers -- and stores
// them with 16-byte stores.  LDS: 16 bytes per voice the list can hold (notes_cap of them, 5000 at most: 80 KB) + the
// 4 KB wave table.
//
// gdm_synth_windows renders W windows of F clips of ANY length (a MIDI performance: tens of thousands of notes) in one
// launch.  Its note rows carry sample times and ascend in s_on, so a workgroup never scans the clip: two binary searches
// bound the rows that can sound in its 2048 samples, and it walks them in tiles of 1024 rows, each compacted into a
// fixed 16 KB list and added to the same eight register sums.  No cap on notes or on simultaneous voices.
//
// gdm_synth_windows_gm (the end of this file) is its sibling with a timbre per General MIDI family: a fifth column
// holds the program, f = (program & 127) >> 3 picks one of 16 wave tables and one of 16 (attack, release) pairs.
#include "gdm_common.h"
#include "buffer_ops.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 2048;                       // samples per workgroup = GDM_SYNTH_NFFT
constexpr int kPer = kChunk / kThreads;            // 8 per thread
constexpr int kMaxNotes = GDM_DES_NOTES_MAX;
constexpr int kA = GDM_SYNTH_ATTACK, kR = GDM_SYNTH_RELEASE, kShift = GDM_SYNTH_SHIFT;
constexpr int kFrames = GDM_SYNTH_FRAMES;
static_assert(kChunk == GDM_SYNTH_NFFT && GDM_SYNTH_WAVE == 2048, "phase >> 21 indexes a 2048-entry table");

typedef short short8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int64_t tick_to_sample(int64_t tick) { return (tick * 735) >> 3; }

// A voice that sounds somewhere in [lo, lo + 2^13), as the list holds it:
//   x = phase at sample lo (mod 2^32),  y = inc[p],  z = s_on - lo clamped to [-A, 2^13],
//   w = (s_off - lo clamped to [-R, 2^20]) + R  |  v << 24
// The clamps change nothing inside the range: from A samples after s_on the attack is full, and a note-off beyond the
// range is simply "not yet".  They are written as comparisons so that no difference of two times is formed that could
// leave 64 bits, whatever the rows hold (|lo| <= 2^62).
__device__ __forceinline__ int4 voice_entry(int64_t s_on, int64_t s_off, int64_t pitch, int64_t velocity, int64_t lo,
                                            const uint32_t* __restrict__ inc) {
  const uint32_t step = inc[pitch & 127];
  const uint32_t vel = (uint32_t)(velocity & 127);
  const int64_t on_rel = s_on < lo - kA ? (int64_t)-kA : (s_on > lo + (1 << 13) ? (int64_t)1 << 13 : s_on - lo);
  const int64_t off_rel = s_off < lo - kR ? (int64_t)-kR : (s_off > lo + (1 << 20) ? (int64_t)1 << 20 : s_off - lo);
  int4 e;
  e.x = (int)(step * (uint32_t)((uint64_t)lo - (uint64_t)s_on));
  e.y = (int)step;
  e.z = (int)on_rel;
  e.w = (int)((uint32_t)(off_rel + kR) | (vel << 24));
  return e;
}

// Stage the wave table and the voices that sound anywhere in [lo, hi] (hi - lo < 2^13), times given in ticks.  Returns
// the number of listed voices (<= n <= kMaxNotes: the list cannot overflow).
__device__ int stage_voices(const int64_t* __restrict__ notes, int n, int64_t lo, int64_t hi,
                            const int16_t* __restrict__ wave, const uint32_t* __restrict__ inc, int4* s_voice,
                            int16_t* s_wave, int* s_count) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_count = 0;
  for (int i = tid; i < GDM_SYNTH_WAVE; i += kThreads) s_wave[i] = wave[i];
  __syncthreads();
  for (int k = tid; k < n; k += kThreads) {
    const int64_t s_on = tick_to_sample(notes[4 * (int64_t)k + 0]);
    const int64_t s_off = tick_to_sample(notes[4 * (int64_t)k + 1]);
    if (s_on > hi || s_off + kR <= lo) continue;
    s_voice[atomicAdd(s_count, 1)] =
        voice_entry(s_on, s_off, notes[4 * (int64_t)k + 2], notes[4 * (int64_t)k + 3], lo, inc);
  }
  __syncthreads();
  return *s_count;
}

// THE per-sample function of both kernels: acc[e] += the listed voices at t[e] = sample - lo, e < 8.
__device__ __forceinline__ void add_voices(const int4* s_voice, int n, const int16_t* s_wave, const int (&t)[kPer],
                                           int (&acc)[kPer]) {
  for (int k = 0; k < n; ++k) {
    const int4 v = s_voice[k];
    const int off = (int)((uint32_t)v.w & 0xFFFFFFu) - kR, vel = (int)((uint32_t)v.w >> 24);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int d = t[e] - v.z, past = t[e] - off;                  // samples since note-on / since note-off
      if (d >= 0 && past < kR) {
        const uint32_t phase = (uint32_t)v.x + (uint32_t)v.y * (uint32_t)t[e];
        const int e_att = min(d + 1, kA);
        const int e_rel = past < 0 ? kR : kR - past;
        const int64_t p = (int64_t)((int)s_wave[phase >> 21] * vel * e_att) * e_rel;      // the int part is < 2^30
        acc[e] += (int)(p >> kShift);
      }
    }
  }
}

__device__ __forceinline__ int clamp16(int v) { return min(32767, max(-32768, v)); }

// One workgroup per (frame, sample): element n of frame f is the synth at f * hop + n - 1024, reflected inside the clip
// by the rule of pcm_stft_frames_kernel (s < 0 -> -s, then s >= L -> 2 (L - 1) - s), times 2^-15 (PCM_S16's decode).
__global__ __launch_bounds__(kThreads) void synth_frames_kernel(const int64_t* __restrict__ notes, int notes_cap,
                                                                const int32_t* __restrict__ n_notes,
                                                                const int64_t* __restrict__ clip_len,
                                                                const int16_t* __restrict__ wave,
                                                                const uint32_t* __restrict__ inc,
                                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int4* s_voice = reinterpret_cast<int4*>(s_raw);
  __shared__ int16_t s_wave[GDM_SYNTH_WAVE];
  __shared__ int s_count;
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(n_notes[b], 0), min(notes_cap, kMaxNotes));
  const int64_t L = clip_len[b];
  f32x4* o = reinterpret_cast<f32x4*>(out + ((int64_t)b * kFrames + f) * kChunk + tid * kPer);
  if (n == 0 || L <= kChunk / 2) {                     // a blank clip: zero frames (uniform over the workgroup)
    o[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int64_t hop = L / (kFrames - 1);
  const int64_t a = (int64_t)f * hop - kChunk / 2, z = a + kChunk - 1;                  // the unreflected range
  const int64_t lo = max((int64_t)0, min(a, 2 * (L - 1) - z)), hi = min(L - 1, max(z, -a));
  const int nv = stage_voices(notes + (int64_t)b * notes_cap * 4, n, lo, hi, wave, inc, s_voice, s_wave, &s_count);
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    int64_t s = a + tid * kPer + e;
    s = s < 0 ? -s : s;
    s = s >= L ? 2 * (L - 1) - s : s;
    t[e] = (int)min(max(s - lo, (int64_t)0), hi - lo);   // inside by construction; the clamp bounds it for any input
    acc[e] = 0;
  }
  add_voices(s_voice, nv, s_wave, t, acc);
  f32x4 v0, v1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v0[e] = (float)clamp16(acc[e]) * 0x1p-15f;
    v1[e] = (float)clamp16(acc[4 + e]) * 0x1p-15f;
  }
  o[0] = v0;
  o[1] = v1;
}

// One workgroup per 2048 samples of [first, first + count) of ONE clip, as 16-bit PCM.
__global__ __launch_bounds__(kThreads) void synth_pcm_kernel(const int64_t* __restrict__ notes, int notes_cap,
                                                             const int32_t* __restrict__ n_notes,
                                                             const int16_t* __restrict__ wave,
                                                             const uint32_t* __restrict__ inc, int64_t first,
                                                             int64_t count, int16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int4* s_voice = reinterpret_cast<int4*>(s_raw);
  __shared__ int16_t s_wave[GDM_SYNTH_WAVE];
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const int n = min(max(n_notes[0], 0), min(notes_cap, kMaxNotes));
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;                   // first output sample of this workgroup
  const int64_t lo = first + c0;
  const int nv = stage_voices(notes, n, lo, lo + kChunk - 1, wave, inc, s_voice, s_wave, &s_count);
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    t[e] = tid * kPer + e;
    acc[e] = 0;
  }
  add_voices(s_voice, nv, s_wave, t, acc);
  const int64_t i0 = c0 + tid * kPer;
  if (i0 + kPer <= count) {
    short8 v;
#pragma unroll
    for (int e = 0; e < kPer; ++e) v[e] = (short)clamp16(acc[e]);
    *reinterpret_cast<short8*>(out + i0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (i0 + e < count) out[i0 + e] = (int16_t)clamp16(acc[e]);
  }
}

// One workgroup per (2048-sample chunk, window) of gdm_synth_windows.  Rows [r0, r1) are the window's clip; of them only
// [begin, end) can sound in [lo, hi]: rows from `end` on start after hi (s_on ascends), rows before `begin` have all
// ended before lo (off_max is the running maximum of s_off).  Everything read from device memory is clamped before it
// bounds a loop or forms an address: the clip index to [0, F), the row range to [0, n_total], the searches to the range.
constexpr int kTile = GDM_SYNTH_TILE;
constexpr int64_t kTimeMax = (int64_t)1 << 62;

__global__ __launch_bounds__(kThreads) void synth_windows_kernel(const int64_t* __restrict__ notes,
                                                                 const int64_t* __restrict__ off_max, int64_t n_total,
                                                                 const int64_t* __restrict__ note_ptr, int F,
                                                                 const int32_t* __restrict__ win_clip,
                                                                 const int64_t* __restrict__ win_start, int64_t win_len,
                                                                 int64_t out_stride, const int16_t* __restrict__ wave,
                                                                 const uint32_t* __restrict__ inc,
                                                                 int16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) int4 s_voice[kTile];
  __shared__ int16_t s_wave[GDM_SYNTH_WAVE];
  __shared__ int s_count;
  const int tid = threadIdx.x, w = blockIdx.y;
  const int clip = min(max(win_clip[w], 0), F - 1);
  const int64_t r0 = min(max(note_ptr[clip], (int64_t)0), n_total);
  const int64_t r1 = min(max(note_ptr[clip + 1], r0), n_total);
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;                   // first output sample of this workgroup
  const int64_t lo = min(max(win_start[w], -kTimeMax), kTimeMax) + c0, hi = lo + kChunk - 1;
  int64_t a = r0, b = r1;                                            // end: the first row with s_on > hi
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (notes[4 * m] > hi) b = m; else a = m + 1;
  }
  const int64_t end = a;
  a = r0, b = end;                                                   // begin: the first row with off_max + R > lo
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (off_max[m] > lo - kR) b = m; else a = m + 1;
  }
  const int64_t begin = a;
  if (tid == 0) s_count = 0;
  for (int i = tid; i < GDM_SYNTH_WAVE; i += kThreads) s_wave[i] = wave[i];
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    t[e] = tid * kPer + e;
    acc[e] = 0;
  }
  __syncthreads();
  for (int64_t base = begin; base < end; base += kTile) {            // uniform over the workgroup
    const int64_t stop = min(base + kTile, end);
    for (int64_t k = base + tid; k < stop; k += kThreads) {
      const int64_t s_on = notes[4 * k + 0], s_off = notes[4 * k + 1];
      if (s_on > hi || s_off <= lo - kR) continue;
      s_voice[atomicAdd(&s_count, 1)] = voice_entry(s_on, s_off, notes[4 * k + 2], notes[4 * k + 3], lo, inc);
    }
    __syncthreads();
    add_voices(s_voice, s_count, s_wave, t, acc);                    // <= kTile entries: the list cannot overflow
    __syncthreads();
    if (tid == 0) s_count = 0;                                       // ordered before the next tile's adds by its barrier
    __syncthreads();
  }
  const int64_t i0 = c0 + tid * kPer;
  int16_t* o = out + (int64_t)w * out_stride;
  if (i0 + kPer <= win_len) {
    short8 v;
#pragma unroll
    for (int e = 0; e < kPer; ++e) v[e] = (short)clamp16(acc[e]);
    *reinterpret_cast<short8*>(o + i0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (i0 + e < win_len) o[i0 + e] = (int16_t)clamp16(acc[e]);
  }
}

int tables_ok(const char* who, const void* notes, int notes_cap, const void* n_notes, const void* wave, const void* inc) {
  GDM_REQUIRE(notes && n_notes && wave && inc, "%s: null pointer", who);
  GDM_REQUIRE(notes_cap > 0 && notes_cap <= GDM_DES_NOTES_MAX, "%s: %d notes per clip (1 .. %d fit the voice list)", who,
              notes_cap, GDM_DES_NOTES_MAX);
  GDM_REQUIRE(((uintptr_t)notes & 7) == 0 && ((uintptr_t)wave & 1) == 0 && ((uintptr_t)inc & 3) == 0,
              "%s: notes / wave / inc must be aligned to their elements", who);
  return GDM_OK;
}

}  // namespace

extern "C" int gdm_synth_frames(const int64_t* notes, int notes_cap, const int32_t* n_notes, const int64_t* clip_len,
                                int B, const int16_t* wave, const uint32_t* inc, float* frames, void* stream) {
  if (int rc = tables_ok("gdm_synth_frames", notes, notes_cap, n_notes, wave, inc)) return rc;
  GDM_REQUIRE(clip_len && frames, "gdm_synth_frames: null pointer");
  GDM_REQUIRE(B > 0 && B <= 65535, "gdm_synth_frames: B = %d (1 .. 65535)", B);
  GDM_REQUIRE(((uintptr_t)frames & 15) == 0, "gdm_synth_frames: frames must be 16-byte aligned (16-byte stores)");
  allow_lds(synth_frames_kernel, kMaxNotes * sizeof(int4));
  hipLaunchKernelGGL(synth_frames_kernel, dim3(kFrames, B), dim3(kThreads), notes_cap * sizeof(int4), (hipStream_t)stream, notes,
                     notes_cap, n_notes, clip_len, wave, inc, frames);
  GDM_LAUNCH_OK("gdm_synth_frames");
  return GDM_OK;
}

extern "C" int gdm_synth_pcm(const int64_t* notes, int notes_cap, const int32_t* n_notes, const int16_t* wave,
                             const uint32_t* inc, int64_t first, int64_t count, int16_t* out, void* stream) {
  if (int rc = tables_ok("gdm_synth_pcm", notes, notes_cap, n_notes, wave, inc)) return rc;
  GDM_REQUIRE(out && ((uintptr_t)out & 15) == 0, "gdm_synth_pcm: out must be a 16-byte aligned buffer (16-byte stores)");
  GDM_REQUIRE(first >= 0 && first <= ((int64_t)1 << 40) && count > 0 && count <= ((int64_t)1 << 30),
              "gdm_synth_pcm: samples %lld .. +%lld (first within 0 .. 2^40, 1 .. 2^30 samples per call)",
              (long long)first, (long long)count);
  allow_lds(synth_pcm_kernel, kMaxNotes * sizeof(int4));
  hipLaunchKernelGGL(synth_pcm_kernel, dim3((unsigned)((count + kChunk - 1) / kChunk)), dim3(kThreads),
                     notes_cap * sizeof(int4),
                     (hipStream_t)stream, notes, notes_cap, n_notes, wave, inc, first, count, out);
  GDM_LAUNCH_OK("gdm_synth_pcm");
  return GDM_OK;
}

extern "C" int gdm_synth_windows(const int64_t* notes, const int64_t* off_max, int64_t n_total, const int64_t* note_ptr,
                                 int F, const int32_t* win_clip, const int64_t* win_start, int W, int64_t win_len,
                                 int64_t out_stride, const int16_t* wave, const uint32_t* inc, int16_t* out,
                                 void* stream) {
  GDM_REQUIRE(n_total >= 0, "gdm_synth_windows: n_total = %lld", (long long)n_total);
  GDM_REQUIRE((notes && off_max) || n_total == 0, "gdm_synth_windows: null pointer (notes / off_max of %lld rows)",
              (long long)n_total);
  GDM_REQUIRE(note_ptr && win_clip && win_start && wave && inc && out, "gdm_synth_windows: null pointer");
  GDM_REQUIRE(((uintptr_t)notes & 7) == 0 && ((uintptr_t)off_max & 7) == 0 && ((uintptr_t)note_ptr & 7) == 0 &&
                  ((uintptr_t)win_start & 7) == 0 && ((uintptr_t)win_clip & 3) == 0 && ((uintptr_t)wave & 1) == 0 &&
                  ((uintptr_t)inc & 3) == 0,
              "gdm_synth_windows: notes / off_max / note_ptr / win_clip / win_start / wave / inc must be aligned to "
              "their elements");
  GDM_REQUIRE(((uintptr_t)out & 15) == 0, "gdm_synth_windows: out must be 16-byte aligned (16-byte stores)");
  GDM_REQUIRE(F >= 1, "gdm_synth_windows: F = %d clips (at least 1)", F);
  GDM_REQUIRE(W >= 1 && W <= 65535, "gdm_synth_windows: W = %d windows (1 .. 65535)", W);
  GDM_REQUIRE(win_len >= 1 && win_len <= ((int64_t)1 << 30), "gdm_synth_windows: win_len = %lld (1 .. 2^30 samples)",
              (long long)win_len);
  GDM_REQUIRE(out_stride >= win_len && out_stride % 8 == 0,
              "gdm_synth_windows: out_stride = %lld (at least win_len = %lld and a multiple of 8: 16-byte stores)",
              (long long)out_stride, (long long)win_len);
  hipLaunchKernelGGL(synth_windows_kernel, dim3((unsigned)((win_len + kChunk - 1) / kChunk), W), dim3(kThreads), 0,
                     (hipStream_t)stream, notes, off_max, n_total, note_ptr, F, win_clip, win_start, win_len, out_stride,
                     wave, inc, out);
  GDM_LAUNCH_OK("gdm_synth_windows");
  return GDM_OK;
}

// ---- gdm_synth_windows_gm: the windows kernel with 16 timbres ------------------------------------------------------------
// Same windows, tiles and searches as synth_windows_kernel.  What differs: rows of five columns; the family's wave table
// and envelope per voice; `end_max` (the running maximum of s_off + R_row) where off_max stands, because the release now
// varies per row.  All 16 tables (64 KB) and the envelopes are staged in LDS: the inner loop reads one table entry per
// voice and sample at a data-dependent index -- per-lane LDS reads, where a global load would touch a cache line per
// lane.  81 KB of LDS per workgroup: one workgroup of four waves per CU half, which the eight sums per thread keep busy.
namespace {

constexpr int kFam = GDM_SYNTH_GM_FAMILIES;
constexpr int kEnvMax = GDM_SYNTH_GM_ENV_MAX;
constexpr size_t kGmWaveBytes = (size_t)kFam * GDM_SYNTH_WAVE * sizeof(int16_t);
constexpr size_t kGmLdsBytes = kGmWaveBytes + (size_t)kTile * sizeof(int4) + 2 * kFam * sizeof(int) + 16;
static_assert(kEnvMax == kA * kR, "the default envelopes keep A_f * R_f at the one voice's A * R");

// A voice that sounds somewhere in [lo, lo + 2^13):
//   x = phase at sample lo (mod 2^32),  y = inc[p],  z = (s_on - lo clamped to [-2^21, 2^13]) << 4 | family,
//   w = (s_off - lo clamped to [-2^21, 2^20]) + 2^21  |  v << 24
// As in voice_entry the clamps change nothing inside the range (A_f, R_f <= 2^21) and are written as comparisons.
__device__ __forceinline__ int4 voice_entry_gm(int64_t s_on, int64_t s_off, int64_t pitch, int64_t velocity, int family,
                                               int64_t lo, const uint32_t* __restrict__ inc) {
  const uint32_t step = inc[pitch & 127];
  const uint32_t vel = (uint32_t)(velocity & 127);
  const int64_t on_rel = s_on < lo - kEnvMax ? (int64_t)-kEnvMax : (s_on > lo + (1 << 13) ? (int64_t)1 << 13 : s_on - lo);
  const int64_t off_rel =
      s_off < lo - kEnvMax ? (int64_t)-kEnvMax : (s_off > lo + (1 << 20) ? (int64_t)1 << 20 : s_off - lo);
  int4 e;
  e.x = (int)(step * (uint32_t)((uint64_t)lo - (uint64_t)s_on));
  e.y = (int)step;
  e.z = (int)(on_rel * 16) | family;
  e.w = (int)((uint32_t)(off_rel + kEnvMax) | (vel << 24));
  return e;
}

__device__ __forceinline__ void add_voices_gm(const int4* s_voice, int n, const int16_t* s_waves, const int* s_env,
                                              const int (&t)[kPer], int (&acc)[kPer]) {
  for (int k = 0; k < n; ++k) {
    const int4 v = s_voice[k];
    const int family = v.z & (kFam - 1), on = v.z >> 4;
    const int A = s_env[2 * family], R = s_env[2 * family + 1];
    const int off = (int)((uint32_t)v.w & 0xFFFFFFu) - kEnvMax, vel = (int)((uint32_t)v.w >> 24);
    const int16_t* wave = s_waves + family * GDM_SYNTH_WAVE;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int d = t[e] - on, past = t[e] - off;                   // samples since note-on / since note-off
      if (d >= 0 && past < R) {
        const uint32_t phase = (uint32_t)v.x + (uint32_t)v.y * (uint32_t)t[e];
        const int e_att = min(d + 1, A);
        const int e_rel = past < 0 ? R : R - past;
        // |wave * vel| < 2^22 and e_att * e_rel <= 2^42; with A_f * R_f = 2^21 the product stays below 2^43.  Unsigned
        // arithmetic, so that tables beyond that wrap instead of overflowing.
        const uint64_t p = (uint64_t)(int64_t)((int)wave[phase >> 21] * vel) * (uint64_t)((int64_t)e_att * e_rel);
        acc[e] += (int)((int64_t)p >> kShift);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void synth_windows_gm_kernel(
    const int64_t* __restrict__ notes, const int64_t* __restrict__ end_max, int64_t n_total,
    const int64_t* __restrict__ note_ptr, int F, const int32_t* __restrict__ win_clip,
    const int64_t* __restrict__ win_start, int64_t win_len, int64_t out_stride, const int16_t* __restrict__ waves,
    const int32_t* __restrict__ env, const uint32_t* __restrict__ inc, int16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int16_t* s_waves = reinterpret_cast<int16_t*>(s_raw);
  int4* s_voice = reinterpret_cast<int4*>(s_raw + kGmWaveBytes);
  int* s_env = reinterpret_cast<int*>(s_raw + kGmWaveBytes + (size_t)kTile * sizeof(int4));
  int* s_count = s_env + 2 * kFam;
  const int tid = threadIdx.x, w = blockIdx.y;
  const int clip = min(max(win_clip[w], 0), F - 1);
  const int64_t r0 = min(max(note_ptr[clip], (int64_t)0), n_total);
  const int64_t r1 = min(max(note_ptr[clip + 1], r0), n_total);
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;                   // first output sample of this workgroup
  const int64_t lo = min(max(win_start[w], -kTimeMax), kTimeMax) + c0, hi = lo + kChunk - 1;
  int64_t a = r0, b = r1;                                            // end: the first row with s_on > hi
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (notes[5 * m] > hi) b = m; else a = m + 1;
  }
  const int64_t end = a;
  a = r0, b = end;                                                   // begin: the first row with end_max > lo
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (end_max[m] > lo) b = m; else a = m + 1;
  }
  const int64_t begin = a;
  if (tid == 0) *s_count = 0;
  if (tid < 2 * kFam) s_env[tid] = min(max(env[tid], 1), kEnvMax);
  if (begin < end) {                                                 // uniform: a silent chunk reads no table
    const int4* src = reinterpret_cast<const int4*>(waves);
    int4* dst = reinterpret_cast<int4*>(s_waves);
    for (int i = tid; i < (int)(kGmWaveBytes / sizeof(int4)); i += kThreads) dst[i] = src[i];
  }
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    t[e] = tid * kPer + e;
    acc[e] = 0;
  }
  __syncthreads();
  for (int64_t base = begin; base < end; base += kTile) {            // uniform over the workgroup
    const int64_t stop = min(base + kTile, end);
    for (int64_t k = base + tid; k < stop; k += kThreads) {
      const int64_t s_on = notes[5 * k + 0], s_off = notes[5 * k + 1];
      const int family = (int)((notes[5 * k + 4] & 127) >> 3);
      if (s_on > hi || s_off <= lo - s_env[2 * family + 1]) continue;
      s_voice[atomicAdd(s_count, 1)] = voice_entry_gm(s_on, s_off, notes[5 * k + 2], notes[5 * k + 3], family, lo, inc);
    }
    __syncthreads();
    add_voices_gm(s_voice, *s_count, s_waves, s_env, t, acc);        // <= kTile entries: the list cannot overflow
    __syncthreads();
    if (tid == 0) *s_count = 0;                                      // ordered before the next tile's adds by its barrier
    __syncthreads();
  }
  const int64_t i0 = c0 + tid * kPer;
  int16_t* o = out + (int64_t)w * out_stride;
  if (i0 + kPer <= win_len) {
    short8 v;
#pragma unroll
    for (int e = 0; e < kPer; ++e) v[e] = (short)clamp16(acc[e]);
    *reinterpret_cast<short8*>(o + i0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (i0 + e < win_len) o[i0 + e] = (int16_t)clamp16(acc[e]);
  }
}

}  // namespace

extern "C" int gdm_synth_windows_gm(const int64_t* notes, const int64_t* end_max, int64_t n_total,
                                    const int64_t* note_ptr, int F, const int32_t* win_clip, const int64_t* win_start,
                                    int W, int64_t win_len, int64_t out_stride, const int16_t* waves, const int32_t* env,
                                    const uint32_t* inc, int16_t* out, void* stream) {
  GDM_REQUIRE(n_total >= 0, "gdm_synth_windows_gm: n_total = %lld", (long long)n_total);
  GDM_REQUIRE((notes && end_max) || n_total == 0, "gdm_synth_windows_gm: null pointer (notes / end_max of %lld rows)",
              (long long)n_total);
  GDM_REQUIRE(note_ptr && win_clip && win_start && waves && env && inc && out, "gdm_synth_windows_gm: null pointer");
  GDM_REQUIRE(((uintptr_t)notes & 7) == 0 && ((uintptr_t)end_max & 7) == 0 && ((uintptr_t)note_ptr & 7) == 0 &&
                  ((uintptr_t)win_start & 7) == 0 && ((uintptr_t)win_clip & 3) == 0 && ((uintptr_t)env & 3) == 0 &&
                  ((uintptr_t)inc & 3) == 0,
              "gdm_synth_windows_gm: notes / end_max / note_ptr / win_clip / win_start / env / inc must be aligned to "
              "their elements");
  GDM_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)waves & 15) == 0,
              "gdm_synth_windows_gm: out and waves must be 16-byte aligned (16-byte stores and loads)");
  GDM_REQUIRE(F >= 1, "gdm_synth_windows_gm: F = %d clips (at least 1)", F);
  GDM_REQUIRE(W >= 1 && W <= 65535, "gdm_synth_windows_gm: W = %d windows (1 .. 65535)", W);
  GDM_REQUIRE(win_len >= 1 && win_len <= ((int64_t)1 << 30), "gdm_synth_windows_gm: win_len = %lld (1 .. 2^30 samples)",
              (long long)win_len);
  GDM_REQUIRE(out_stride >= win_len && out_stride % 8 == 0,
              "gdm_synth_windows_gm: out_stride = %lld (at least win_len = %lld and a multiple of 8: 16-byte stores)",
              (long long)out_stride, (long long)win_len);
  allow_lds(synth_windows_gm_kernel, kGmLdsBytes);
  hipLaunchKernelGGL(synth_windows_gm_kernel, dim3((unsigned)((win_len + kChunk - 1) / kChunk), W), dim3(kThreads),
                     kGmLdsBytes, (hipStream_t)stream, notes, end_max, n_total, note_ptr, F, win_clip, win_start, win_len,
                     out_stride, waves, env, inc, out);
  GDM_LAUNCH_OK("gdm_synth_windows_gm");
  return GDM_OK;
}
