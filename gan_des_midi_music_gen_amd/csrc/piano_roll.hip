// Piano-roll rasteriser: the scatter at the heart of generate_piano_roll
// (MMGAN_MIDI_DES/datasets.py:29-45) for a batch of MIDI files.
//
//   note_on  (note, step, velocity):  piano_roll[note][step] = velocity;  note_on_time[note] = step
//   note_off (note, step):            off = note_on_time[note];  durations[note][off:step] = step - off
//
// Later messages overwrite earlier ones, so the order of a note's messages matters and nothing else does: rows
// (file, note) are independent.  The host (datasets.py) parses the files, converts message times to one-second steps,
// cuts every file's message list where the reference's loop stops, and hands over each row's messages in file order
// (CSR over file * 128 + note).  One workgroup per file clears the file's two (128, W) planes with coalesced stores,
// then thread `note` replays its row.  Integer work on a few KB per file: bound by launch latency and the planes' bytes.
#include "gdm_common.h"
#include "buffer_ops.h"

namespace {

__global__ __launch_bounds__(128) void piano_roll_kernel(const int32_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ ev_step,
                                                         const int32_t* __restrict__ ev_vel,     // < 0: note_off
                                                         int W, float* __restrict__ roll, float* __restrict__ dur) {
  const int f = blockIdx.x, note = threadIdx.x;
  float* r = roll + (int64_t)f * 128 * W;
  float* d = dur + (int64_t)f * 128 * W;
  for (int i = threadIdx.x; i < 128 * W; i += 128) { r[i] = 0.f; d[i] = 0.f; }
  __syncthreads();
  r += (int64_t)note * W;
  d += (int64_t)note * W;
  int on_time = 0;                                            // note_on_time = np.zeros(128)
  const int e0 = row_ptr[f * 128 + note], e1 = row_ptr[f * 128 + note + 1];
  for (int e = e0; e < e1; ++e) {
    const int step = ev_step[e], vel = ev_vel[e];
    if (vel >= 0) {
      if (step < W) r[step] = (float)vel;                      // (the host cut the list before a note_on with step >= W)
      on_time = step;
    } else {
      const float len = (float)(step - on_time);
      for (int s = on_time; s < step && s < W; ++s) d[s] = len;     // numpy clips the slice at the array's width
    }
  }
}

// The windowed form (data_viewing_and_processing.ipynb cell 11 cuts cell 10's (128, sample_size) planes into windows of
// L steps): one workgroup per OUTPUT window.  Both planes of the window are built in LDS -- cleared, then thread `note`
// replays its row from the start of the file and keeps only what falls into columns [s0, s0 + L): note_on_time
// carries over from earlier windows and a duration keeps its full-length value in every window it crosses -- and
// leave with 16-byte stores, lane after lane (the per-file kernel above writes L floats apart between lanes).  Every
// output plane is written by exactly one workgroup: no atomics and no memset launch.
constexpr int kWinThreads = 256;
constexpr int kWinMaxL = 160 * 1024 / (2 * 128 * 4);           // both planes of a window in one workgroup's LDS

__global__ __launch_bounds__(kWinThreads) void piano_roll_windows_kernel(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ ev_step, const int32_t* __restrict__ ev_vel,
    const int32_t* __restrict__ win_file, const int32_t* __restrict__ win_s0, int L, float* __restrict__ roll,
    float* __restrict__ dur) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  float* r_s = (float*)dyn_smem;                              // [128][L]
  float* d_s = r_s + 128 * L;                                 // [128][L]; 512 L bytes on: 16-byte aligned
  const int n = blockIdx.x, f = win_file[n], s0 = win_s0[n], s1 = s0 + L;
  const int n4 = 2 * 128 * L / 4;                             // float4s of both planes
  f32x4* lds4 = (f32x4*)dyn_smem;
  for (int i = threadIdx.x; i < n4; i += kWinThreads) lds4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  if (threadIdx.x < 128) {
    const int note = threadIdx.x;
    float* r = r_s + note * L;                                // column = step - s0, inside [0, L) only
    float* d = d_s + note * L;
    int on_time = 0;                                          // note_on_time = np.zeros(128)
    const int e0 = row_ptr[f * 128 + note], e1 = row_ptr[f * 128 + note + 1];
    for (int e = e0; e < e1; ++e) {
      const int step = ev_step[e], vel = ev_vel[e];
      if (vel >= 0) {
        if (step >= s0 && step < s1) r[step - s0] = (float)vel;
        on_time = step;
      } else {
        const float len = (float)(step - on_time);
        const int a = on_time > s0 ? on_time : s0, b = step < s1 ? step : s1;
        for (int s = a; s < b; ++s) d[s - s0] = len;
      }
    }
  }
  __syncthreads();
  f32x4* ro = (f32x4*)(roll + (int64_t)n * 128 * L);
  f32x4* dn = (f32x4*)(dur + (int64_t)n * 128 * L);
  const int h4 = n4 / 2;
  for (int i = threadIdx.x; i < h4; i += kWinThreads) {
    ro[i] = lds4[i];
    dn[i] = lds4[h4 + i];
  }
}

}  // namespace

extern "C" int gdm_piano_roll_windows(const int32_t* row_ptr, const int32_t* ev_step, const int32_t* ev_vel,
                                      const int32_t* win_file, const int32_t* win_s0, int n_windows, int L, float* roll,
                                      float* dur, void* stream) {
  GDM_REQUIRE(row_ptr && win_file && win_s0 && roll && dur && n_windows > 0 && L > 0,
              "gdm_piano_roll_windows: bad arguments");
  const size_t lds = (size_t)2 * 128 * 4 * L;
  GDM_REQUIRE(L <= kWinMaxL, "gdm_piano_roll_windows: L = %d needs %zu bytes of LDS, a workgroup has %d (L <= %d)", L,
              lds, 160 * 1024, kWinMaxL);
  GDM_REQUIRE(((uintptr_t)roll | (uintptr_t)dur) % 16 == 0,
              "gdm_piano_roll_windows: roll and dur must be 16-byte aligned");
  allow_lds(piano_roll_windows_kernel, 160 * 1024);
  hipLaunchKernelGGL(piano_roll_windows_kernel, dim3(n_windows), dim3(kWinThreads), lds, (hipStream_t)stream, row_ptr,
                     ev_step, ev_vel, win_file, win_s0, L, roll, dur);
  GDM_LAUNCH_OK("gdm_piano_roll_windows");
  return GDM_OK;
}

extern "C" int gdm_piano_roll_raster(const int32_t* row_ptr, const int32_t* ev_step, const int32_t* ev_vel, int n_files,
                                     int W, float* roll, float* dur, void* stream) {
  GDM_REQUIRE(row_ptr && roll && dur && n_files > 0 && W > 0, "gdm_piano_roll_raster: bad arguments");
  hipLaunchKernelGGL(piano_roll_kernel, dim3(n_files), dim3(128), 0, (hipStream_t)stream, row_ptr, ev_step, ev_vel, W,
                     roll, dur);
  GDM_LAUNCH_OK("gdm_piano_roll_raster");
  return GDM_OK;
}
