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
// Every kernel works on 2048 output samples per workgroup: the voices that can sound in them are COMPACTED into an LDS
// list (the integer sum does not depend on the order, so the slots are dealt by an LDS atomic counter), rebased to the
// range's first sample so that everything after is 32-bit; then every thread produces 8 samples -- the voices in the
// outer loop, the 8 running sums in registers -- and stores them with 16-byte stores.
//
// gdm_synth_frames / gdm_synth_pcm take clips of at most 5000 notes in ticks: the clips are minutes long and the 216
// frames of a clip read about a tenth of it, so whole clips are never rendered; all threads scan the clip's list.  LDS:
// 16 bytes per voice the list can hold (notes_cap of them, 5000 at most: 80 KB) + the 4 KB wave table.
//
// gdm_synth_windows / gdm_synth_windows_gm render W windows of F clips of ANY length (a MIDI performance: tens of
// thousands of notes) in one launch.  Their rows carry sample times and ascend in s_on, so a workgroup never scans the
// clip: two binary searches bound the rows that can sound in its 2048 samples, and it walks them in tiles of 1024 rows,
// each compacted into a fixed 16 KB list and added to the same eight register sums.  No cap on notes or on simultaneous
// voices.  The two are ONE kernel, synth_windows_kernel<Timbre>, and differ only in what the timbre policy supplies:
//
//                       PlainTimbre (gdm_synth_windows)              GmTimbre (gdm_synth_windows_gm)
//   row                 4 columns                                    5: the program, family f = (program & 127) >> 3
//   bound column        off_max: running maximum of s_off            end_max: running maximum of s_off + R_f
//   attack, release     the constants A, R                           (A_f, R_f) = env[f] clamped to 1 .. 2^21, from LDS
//   list entry          z = s_on - lo                                z = (s_on - lo) << 4 | f
//   tables              the 4 KB wave, always staged                 16 waves (64 KB), staged when a row can sound
//   product             int32 * int64, signed                        uint64: tables beyond A_f R_f = 2^21 wrap
//   LDS                 20 KB-odd, static                            kLdsBytes = 81 KB-odd, dynamic
//
// The clamps of what is read from device memory, the searches, the tile loop, the sums and the int16 epilogue exist
// once; gdm_synth_frames and gdm_synth_pcm list and add their voices with the plain policy's functions.
#include "gdm_common.h"
#include "buffer_ops.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 2048;                       // samples per workgroup = GDM_SYNTH_NFFT
constexpr int kPer = kChunk / kThreads;            // 8 per thread
constexpr int kMaxNotes = GDM_DES_NOTES_MAX;
constexpr int kA = GDM_SYNTH_ATTACK, kR = GDM_SYNTH_RELEASE, kShift = GDM_SYNTH_SHIFT;
constexpr int kFrames = GDM_SYNTH_FRAMES;
constexpr int kTile = GDM_SYNTH_TILE;
constexpr int kFam = GDM_SYNTH_GM_FAMILIES;
constexpr int kEnvMax = GDM_SYNTH_GM_ENV_MAX;
static_assert(kChunk == GDM_SYNTH_NFFT && GDM_SYNTH_WAVE == 2048, "phase >> 21 indexes a 2048-entry table");
static_assert(kEnvMax == kA * kR, "the default envelopes keep A_f * R_f at the one voice's A * R");

typedef short short8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int64_t tick_to_sample(int64_t tick) { return (tick * 735) >> 3; }

// ---- the two timbre policies --------------------------------------------------------------------------------------------
// A policy object holds the LDS pointers its voices read; everything else about it is compile-time.  stage() takes the
// entry point's table arguments as the kernel does: a pack of __restrict__ pointers (wave | waves, env).
struct PlainTimbre {
  static constexpr int kCols = 4;
  static constexpr int kOnClamp = kA, kOffClamp = kR;             // how far before `lo` a listed time is kept apart
  static constexpr size_t kLdsBytes = 0;                          // dynamic; the windows kernel's 20 KB-odd are static
  struct Voice {
    int on;
    const int16_t* wave;
    static constexpr int A = kA, R = kR;
  };
  int16_t* s_wave;

  // the LDS of the windows kernel: the tile's list, its counter and the table
  static __device__ __forceinline__ PlainTimbre windows_lds(int4*& s_voice, int*& s_count) {
    __shared__ __attribute__((aligned(16))) int4 voice[kTile];
    __shared__ int16_t wave[GDM_SYNTH_WAVE];
    __shared__ int count;
    s_voice = voice;
    s_count = &count;
    return PlainTimbre{wave};
  }
  __device__ __forceinline__ void stage(bool, const int16_t* __restrict__ wave) const {
    for (int i = threadIdx.x; i < GDM_SYNTH_WAVE; i += kThreads) s_wave[i] = wave[i];
  }
  static __device__ __forceinline__ bool bound_reaches(int64_t off_max, int64_t lo) { return off_max > lo - kR; }
  static __device__ __forceinline__ int family(const int64_t*) { return 0; }
  __device__ __forceinline__ int release(int) const { return kR; }
  static __device__ __forceinline__ int pack_on(int on_rel, int) { return on_rel; }
  __device__ __forceinline__ Voice voice(const int4& v) const { return Voice{v.z, s_wave}; }
  static __device__ __forceinline__ int term(int wave, int vel, int e_att, int e_rel) {
    return (int)(((int64_t)(wave * vel * e_att) * e_rel) >> kShift);                       // the int part is < 2^30
  }
};

// All 16 tables (64 KB) and the envelopes are staged in LDS: the inner loop reads one table entry per voice and sample
// at a data-dependent index -- per-lane LDS reads, where a global load would touch a cache line per lane.  81 KB of LDS
// per workgroup: one workgroup of four waves per CU half, which the eight sums per thread keep busy.
struct GmTimbre {
  static constexpr int kCols = 5;
  static constexpr int kOnClamp = kEnvMax, kOffClamp = kEnvMax;   // A_f, R_f <= 2^21
  static constexpr size_t kWaveBytes = (size_t)kFam * GDM_SYNTH_WAVE * sizeof(int16_t);
  static constexpr size_t kLdsBytes = kWaveBytes + (size_t)kTile * sizeof(int4) + 2 * kFam * sizeof(int) + 16;
  struct Voice {
    int on, A, R;
    const int16_t* wave;
  };
  int16_t* s_waves;
  int* s_env;

  static __device__ __forceinline__ GmTimbre windows_lds(int4*& s_voice, int*& s_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    s_voice = reinterpret_cast<int4*>(s_raw + kWaveBytes);
    int* env = reinterpret_cast<int*>(s_raw + kWaveBytes + (size_t)kTile * sizeof(int4));
    s_count = env + 2 * kFam;
    return GmTimbre{reinterpret_cast<int16_t*>(s_raw), env};
  }
  __device__ __forceinline__ void stage(bool any_row, const int16_t* __restrict__ waves,
                                        const int32_t* __restrict__ env) const {
    const int tid = threadIdx.x;
    if (tid < 2 * kFam) s_env[tid] = min(max(env[tid], 1), kEnvMax);
    if (any_row) {                                                   // uniform: a silent chunk reads no table
      const int4* src = reinterpret_cast<const int4*>(waves);
      int4* dst = reinterpret_cast<int4*>(s_waves);
      for (int i = tid; i < (int)(kWaveBytes / sizeof(int4)); i += kThreads) dst[i] = src[i];
    }
  }
  static __device__ __forceinline__ bool bound_reaches(int64_t end_max, int64_t lo) { return end_max > lo; }
  static __device__ __forceinline__ int family(const int64_t* row) { return (int)((row[4] & 127) >> 3); }
  __device__ __forceinline__ int release(int family) const { return s_env[2 * family + 1]; }
  static __device__ __forceinline__ int pack_on(int on_rel, int family) { return on_rel * 16 | family; }
  __device__ __forceinline__ Voice voice(const int4& v) const {
    const int family = v.z & (kFam - 1);
    return Voice{v.z >> 4, s_env[2 * family], s_env[2 * family + 1], s_waves + family * GDM_SYNTH_WAVE};
  }
  // |wave * vel| < 2^22 and e_att * e_rel <= 2^42; with A_f * R_f = 2^21 the product stays below 2^43.  Unsigned
  // arithmetic, so that tables beyond that wrap instead of overflowing.
  static __device__ __forceinline__ int term(int wave, int vel, int e_att, int e_rel) {
    const uint64_t p = (uint64_t)(int64_t)(wave * vel) * (uint64_t)((int64_t)e_att * e_rel);
    return (int)((int64_t)p >> kShift);
  }
};

// A voice that sounds somewhere in [lo, lo + 2^13), as the list holds it:
//   x = phase at sample lo (mod 2^32),  y = inc[p],  z = pack_on(s_on - lo clamped to [-kOnClamp, 2^13], family),
//   w = (s_off - lo clamped to [-kOffClamp, 2^20]) + kOffClamp  |  v << 24
// The clamps change nothing inside the range: from A samples after s_on the attack is full, and a note-off beyond the
// range is simply "not yet".  They are written as comparisons so that no difference of two times is formed that could
// leave 64 bits, whatever the rows hold (|lo| <= 2^62).
template <class T>
__device__ __forceinline__ int4 voice_entry(int64_t s_on, int64_t s_off, int64_t pitch, int64_t velocity, int family,
                                            int64_t lo, const uint32_t* __restrict__ inc) {
  constexpr int64_t kOn = T::kOnClamp, kOff = T::kOffClamp;
  const uint32_t step = inc[pitch & 127];
  const uint32_t vel = (uint32_t)(velocity & 127);
  const int64_t on_rel = s_on < lo - kOn ? -kOn : (s_on > lo + (1 << 13) ? (int64_t)1 << 13 : s_on - lo);
  const int64_t off_rel = s_off < lo - kOff ? -kOff : (s_off > lo + (1 << 20) ? (int64_t)1 << 20 : s_off - lo);
  int4 e;
  e.x = (int)(step * (uint32_t)((uint64_t)lo - (uint64_t)s_on));
  e.y = (int)step;
  e.z = T::pack_on((int)on_rel, family);
  e.w = (int)((uint32_t)(off_rel + kOff) | (vel << 24));
  return e;
}

// THE per-sample function of every kernel: acc[e] += the listed voices at t[e] = sample - lo, e < 8.
template <class T>
__device__ __forceinline__ void add_voices(const int4* s_voice, int n, const T& timbre, const int (&t)[kPer],
                                           int (&acc)[kPer]) {
  for (int k = 0; k < n; ++k) {
    const int4 v = s_voice[k];
    const auto voice = timbre.voice(v);
    const int off = (int)((uint32_t)v.w & 0xFFFFFFu) - T::kOffClamp, vel = (int)((uint32_t)v.w >> 24);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int d = t[e] - voice.on, past = t[e] - off;             // samples since note-on / since note-off
      if (d >= 0 && past < voice.R) {
        const uint32_t phase = (uint32_t)v.x + (uint32_t)v.y * (uint32_t)t[e];
        const int e_att = min(d + 1, (int)voice.A);
        const int e_rel = past < 0 ? (int)voice.R : voice.R - past;
        acc[e] += T::term((int)voice.wave[phase >> 21], vel, e_att, e_rel);
      }
    }
  }
}

__device__ __forceinline__ int clamp16(int v) { return min(32767, max(-32768, v)); }

// The int16 epilogue: a thread's 8 sums to o[i0 .. i0 + 8), of which only indices below `count` exist.
__device__ __forceinline__ void store_pcm(int16_t* __restrict__ o, int64_t i0, int64_t count, const int (&acc)[kPer]) {
  if (i0 + kPer <= count) {
    short8 v;
#pragma unroll
    for (int e = 0; e < kPer; ++e) v[e] = (short)clamp16(acc[e]);
    *reinterpret_cast<short8*>(o + i0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (i0 + e < count) o[i0 + e] = (int16_t)clamp16(acc[e]);
  }
}

// Stage the wave table and the voices that sound anywhere in [lo, hi] (hi - lo < 2^13), times given in ticks.  Returns
// the number of listed voices (<= n <= kMaxNotes: the list cannot overflow).
__device__ int stage_voices(const int64_t* __restrict__ notes, int n, int64_t lo, int64_t hi,
                            const int16_t* __restrict__ wave, const uint32_t* __restrict__ inc, int4* s_voice,
                            const PlainTimbre& timbre, int* s_count) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_count = 0;
  // PlainTimbre::stage, written out: through the call these two kernels get other instructions and run 2 % slower
  for (int i = tid; i < GDM_SYNTH_WAVE; i += kThreads) timbre.s_wave[i] = wave[i];
  __syncthreads();
  for (int k = tid; k < n; k += kThreads) {
    const int64_t s_on = tick_to_sample(notes[4 * (int64_t)k + 0]);
    const int64_t s_off = tick_to_sample(notes[4 * (int64_t)k + 1]);
    if (s_on > hi || s_off + kR <= lo) continue;
    s_voice[atomicAdd(s_count, 1)] =
        voice_entry<PlainTimbre>(s_on, s_off, notes[4 * (int64_t)k + 2], notes[4 * (int64_t)k + 3], 0, lo, inc);
  }
  __syncthreads();
  return *s_count;
}

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
  const PlainTimbre timbre{s_wave};
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
  const int nv = stage_voices(notes + (int64_t)b * notes_cap * 4, n, lo, hi, wave, inc, s_voice, timbre, &s_count);
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    int64_t s = a + tid * kPer + e;
    s = s < 0 ? -s : s;
    s = s >= L ? 2 * (L - 1) - s : s;
    t[e] = (int)min(max(s - lo, (int64_t)0), hi - lo);   // inside by construction; the clamp bounds it for any input
    acc[e] = 0;
  }
  add_voices(s_voice, nv, timbre, t, acc);
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
  const PlainTimbre timbre{s_wave};
  const int tid = threadIdx.x;
  const int n = min(max(n_notes[0], 0), min(notes_cap, kMaxNotes));
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;                   // first output sample of this workgroup
  const int64_t lo = first + c0;
  const int nv = stage_voices(notes, n, lo, lo + kChunk - 1, wave, inc, s_voice, timbre, &s_count);
  int t[kPer], acc[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    t[e] = tid * kPer + e;
    acc[e] = 0;
  }
  add_voices(s_voice, nv, timbre, t, acc);
  store_pcm(out, c0 + tid * kPer, count, acc);
}

// One workgroup per (2048-sample chunk, window) of gdm_synth_windows[_gm].  Rows [r0, r1) are the window's clip; of them
// only [begin, end) can sound in [lo, hi]: rows from `end` on start after hi (s_on ascends), rows before `begin` have
// all ended before lo (bound_max is the running maximum of the row's last sounding sample, as the timbre counts it).
// Everything read from device memory is clamped before it bounds a loop or forms an address: the clip index to [0, F),
// the row range to [0, n_total], the searches to the range.
constexpr int64_t kTimeMax = (int64_t)1 << 62;

template <class T, class... Tab>                                     // Tab: int16_t | int16_t, int32_t (the tables)
__global__ __launch_bounds__(kThreads) void synth_windows_kernel(
    const int64_t* __restrict__ notes, const int64_t* __restrict__ bound_max, int64_t n_total,
    const int64_t* __restrict__ note_ptr, int F, const int32_t* __restrict__ win_clip,
    const int64_t* __restrict__ win_start, int64_t win_len, int64_t out_stride, const Tab* __restrict__... tables,
    const uint32_t* __restrict__ inc, int16_t* __restrict__ out) {
  constexpr int kCols = T::kCols;
  int4* s_voice;
  int* s_count;
  const T timbre = T::windows_lds(s_voice, s_count);
  const int tid = threadIdx.x, w = blockIdx.y;
  const int clip = min(max(win_clip[w], 0), F - 1);
  const int64_t r0 = min(max(note_ptr[clip], (int64_t)0), n_total);
  const int64_t r1 = min(max(note_ptr[clip + 1], r0), n_total);
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;                   // first output sample of this workgroup
  const int64_t lo = min(max(win_start[w], -kTimeMax), kTimeMax) + c0, hi = lo + kChunk - 1;
  int64_t a = r0, b = r1;                                            // end: the first row with s_on > hi
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (notes[kCols * m] > hi) b = m; else a = m + 1;
  }
  const int64_t end = a;
  a = r0, b = end;                                                   // begin: the first row whose bound reaches lo
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (T::bound_reaches(bound_max[m], lo)) b = m; else a = m + 1;
  }
  const int64_t begin = a;
  if (tid == 0) *s_count = 0;
  timbre.stage(begin < end, tables...);
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
      const int64_t* row = notes + kCols * k;
      const int64_t s_on = row[0], s_off = row[1];
      const int family = T::family(row);
      if (s_on > hi || s_off <= lo - timbre.release(family)) continue;
      s_voice[atomicAdd(s_count, 1)] = voice_entry<T>(s_on, s_off, row[2], row[3], family, lo, inc);
    }
    __syncthreads();
    add_voices(s_voice, *s_count, timbre, t, acc);                   // <= kTile entries: the list cannot overflow
    __syncthreads();
    if (tid == 0) *s_count = 0;                                      // ordered before the next tile's adds by its barrier
    __syncthreads();
  }
  store_pcm(out + (int64_t)w * out_stride, c0 + tid * kPer, win_len, acc);
}

int tables_ok(const char* who, const void* notes, int notes_cap, const void* n_notes, const void* wave, const void* inc) {
  GDM_REQUIRE(notes && n_notes && wave && inc, "%s: null pointer", who);
  GDM_REQUIRE(notes_cap > 0 && notes_cap <= GDM_DES_NOTES_MAX, "%s: %d notes per clip (1 .. %d fit the voice list)", who,
              notes_cap, GDM_DES_NOTES_MAX);
  GDM_REQUIRE(((uintptr_t)notes & 7) == 0 && ((uintptr_t)wave & 1) == 0 && ((uintptr_t)inc & 3) == 0,
              "%s: notes / wave / inc must be aligned to their elements", who);
  return GDM_OK;
}

// What the two windows entry points share; `bound` names the second array (off_max / end_max).  Each checks its own
// tables after this.
int windows_ok(const char* who, const char* bound, const void* notes, const void* bound_max, int64_t n_total,
               const void* note_ptr, int F, const void* win_clip, const void* win_start, int W, int64_t win_len,
               int64_t out_stride, const void* inc, const void* out) {
  GDM_REQUIRE(n_total >= 0, "%s: n_total = %lld", who, (long long)n_total);
  GDM_REQUIRE((notes && bound_max) || n_total == 0, "%s: null pointer (notes / %s of %lld rows)", who, bound,
              (long long)n_total);
  GDM_REQUIRE(note_ptr && win_clip && win_start && inc && out,
              "%s: null pointer (note_ptr / win_clip / win_start / inc / out)", who);
  GDM_REQUIRE(((uintptr_t)notes & 7) == 0 && ((uintptr_t)bound_max & 7) == 0 && ((uintptr_t)note_ptr & 7) == 0 &&
                  ((uintptr_t)win_start & 7) == 0 && ((uintptr_t)win_clip & 3) == 0 && ((uintptr_t)inc & 3) == 0,
              "%s: notes / %s / note_ptr / win_clip / win_start / inc must be aligned to their elements", who, bound);
  GDM_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned (16-byte stores)", who);
  GDM_REQUIRE(F >= 1, "%s: F = %d clips (at least 1)", who, F);
  GDM_REQUIRE(W >= 1 && W <= 65535, "%s: W = %d windows (1 .. 65535)", who, W);
  GDM_REQUIRE(win_len >= 1 && win_len <= ((int64_t)1 << 30), "%s: win_len = %lld (1 .. 2^30 samples)", who,
              (long long)win_len);
  GDM_REQUIRE(out_stride >= win_len && out_stride % 8 == 0,
              "%s: out_stride = %lld (at least win_len = %lld and a multiple of 8: 16-byte stores)", who,
              (long long)out_stride, (long long)win_len);
  return GDM_OK;
}

template <class T, class... Tab>
void launch_windows(const int64_t* notes, const int64_t* bound_max, int64_t n_total, const int64_t* note_ptr, int F,
                    const int32_t* win_clip, const int64_t* win_start, int W, int64_t win_len, int64_t out_stride,
                    const uint32_t* inc, int16_t* out, void* stream, const Tab*... tables) {
  if (T::kLdsBytes) allow_lds((synth_windows_kernel<T, Tab...>), T::kLdsBytes);
  hipLaunchKernelGGL((synth_windows_kernel<T, Tab...>), dim3((unsigned)((win_len + kChunk - 1) / kChunk), W),
                     dim3(kThreads), T::kLdsBytes, (hipStream_t)stream, notes, bound_max, n_total, note_ptr, F, win_clip,
                     win_start, win_len, out_stride, tables..., inc, out);
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
  if (int rc = windows_ok("gdm_synth_windows", "off_max", notes, off_max, n_total, note_ptr, F, win_clip, win_start, W,
                          win_len, out_stride, inc, out))
    return rc;
  GDM_REQUIRE(wave, "gdm_synth_windows: null pointer (wave)");
  GDM_REQUIRE(((uintptr_t)wave & 1) == 0, "gdm_synth_windows: wave must be aligned to its elements");
  launch_windows<PlainTimbre>(notes, off_max, n_total, note_ptr, F, win_clip, win_start, W, win_len, out_stride,
                              inc, out, stream, wave);
  GDM_LAUNCH_OK("gdm_synth_windows");
  return GDM_OK;
}

extern "C" int gdm_synth_windows_gm(const int64_t* notes, const int64_t* end_max, int64_t n_total,
                                    const int64_t* note_ptr, int F, const int32_t* win_clip, const int64_t* win_start,
                                    int W, int64_t win_len, int64_t out_stride, const int16_t* waves, const int32_t* env,
                                    const uint32_t* inc, int16_t* out, void* stream) {
  if (int rc = windows_ok("gdm_synth_windows_gm", "end_max", notes, end_max, n_total, note_ptr, F, win_clip, win_start,
                          W, win_len, out_stride, inc, out))
    return rc;
  GDM_REQUIRE(waves && env, "gdm_synth_windows_gm: null pointer (waves / env)");
  GDM_REQUIRE(((uintptr_t)env & 3) == 0, "gdm_synth_windows_gm: env must be aligned to its elements");
  GDM_REQUIRE(((uintptr_t)waves & 15) == 0, "gdm_synth_windows_gm: waves must be 16-byte aligned (16-byte loads)");
  launch_windows<GmTimbre>(notes, end_max, n_total, note_ptr, F, win_clip, win_start, W, win_len, out_stride,
                           inc, out, stream, waves, env);
  GDM_LAUNCH_OK("gdm_synth_windows_gm");
  return GDM_OK;
}
