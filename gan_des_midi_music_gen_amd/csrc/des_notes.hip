// DES log -> note list for a batch of samples in ONE launch: model 1's consumer behind the DES core, the reader of
// process_adjsim_log (GAN_DES/sim_log_process_music.py:159-185) and MidiGenerator.process_line (:65-133).  Same shape as
// des_midi.hip, one workgroup per sample:
//
//   1. all 256 threads STAGE the (at most 5000) records the reference's reader looks at into LDS: does the regex match
//      the line's text (decided numerically), does the event id pass the fixed 3 / 5 / 7 filter, max(0, int(value)).
//      A record that is not processed is marked inactive; 'processing' lines never match the regex.
//   2. ONE lane replays the active records in order: the per-node queue_lengths (which go negative) and future_events
//      (never cleared: every later departure of the node sounds the same note again), the two queue-length folds, the
//      customer-id fold and the running tick count.  Every departure of a node that has a future event appends a
//      note_on and a note_off, so the track is strictly sequential and its cumulative delta times are the note's ticks.
//
// What the reference would raise for is reported in the status word (a note for a node without note level: KeyError;
// a note outside 0..127: mido refuses the message).  A clip that would pass 2^40 samples is marked GDM_DES_NOTES_ELONG
// and left blank.  The `instruments` list does not reach process_line's output (its program_change lines are commented
// out upstream) and is not an argument.
//
// gdm_des_log_to_notes_pc is the same staging and the same replay for the stand-alone demo's copy of MidiGenerator
// (SIMULATOR/simulation_to_wav.py:162-214), where those program_change lines are NOT commented out: every note_on and
// every note_off is preceded by a program_change carrying the same delta time, so each delta counts twice and each note
// has its node's program (a fifth column).  One source, a template flag; the flag-off instance is the kernel above.
#include "des_log.h"
#include "buffer_ops.h"

namespace {

constexpr int kMaxLines = GDM_DES_NOTES_MAX;      // process_adjsim_log: `max = 5000`
constexpr int kThreads = 256;
constexpr int kMaxDim = GDM_DES_MIDI_MAX_NODES;
constexpr int64_t kMaxTick = ((((int64_t)1 << 40) - GDM_SYNTH_RELEASE) << 3) / 735;   // sample(tick) + release <= 2^40
constexpr size_t kLdsBytes = (size_t)kMaxLines * (8 + 8 + 4);

// What only the program_change variant takes: the programs, the tick -> sample rule sample(tick) = tick * mul / div,
// the samples a clip lasts beyond its last note_off, and the last tick whose sample + tail stays within 2^40.
struct PcArgs {
  const int32_t* instruments;
  int64_t mul, div, tail, max_tick;
};

// the programs of the sample's nodes: LDS that only the program_change instance declares
__device__ __forceinline__ int* program_table() {
  __shared__ int s_prog[kMaxDim];
  return s_prog;
}

__device__ __forceinline__ PcArgs pc_args() { return PcArgs{}; }
__device__ __forceinline__ PcArgs pc_args(const PcArgs& pc) { return pc; }

// Extra = {} (gdm_des_log_to_notes: the kernel's arguments are what they always were) or {PcArgs}
template <bool PC, typename... Extra>
__global__ __launch_bounds__(kThreads) void des_log_to_notes_kernel(
    const double* __restrict__ value, const int64_t* __restrict__ event_id, const int32_t* __restrict__ node,
    const int32_t* __restrict__ kind, const int64_t* __restrict__ rec_ptr, int64_t n_records,
    const int32_t* __restrict__ note_levels, int dim, int64_t* __restrict__ notes, int notes_cap,
    int32_t* __restrict__ n_notes, int64_t* __restrict__ clip_len, int32_t* __restrict__ status, Extra... extra) {
  static_assert(sizeof...(Extra) == (PC ? 1 : 0), "the program_change instance takes one PcArgs");
  constexpr int kCols = PC ? 5 : 4;
  const PcArgs pc = pc_args(extra...);
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int64_t* s_time = reinterpret_cast<int64_t*>(s_raw);                   // max(0, int(value)), or -1: not processed
  int64_t* s_eid = s_time + kMaxLines;
  uint32_t* s_meta = reinterpret_cast<uint32_t*>(s_eid + kMaxLines);     // node | departure << 31
  __shared__ int s_q[kMaxDim], s_fvel[kMaxDim], s_fsrv[kMaxDim], s_note[kMaxDim];
  __shared__ int64_t s_ftime[kMaxDim];
  int* s_prog = nullptr;
  if constexpr (PC) s_prog = program_table();

  const int b = blockIdx.x, tid = threadIdx.x;
  // ---- 1. stage the records
  int64_t r0 = rec_ptr[b], r1 = rec_ptr[b + 1];
  r0 = min(max(r0, (int64_t)0), n_records);
  r1 = min(max(r1, r0), n_records);
  const int n_look = (int)min(r1 - r0, (int64_t)kMaxLines);
  for (int r = tid; r < n_look; r += kThreads) {
    const uint64_t vb = (uint64_t)__double_as_longlong(value[r0 + r]);
    const int64_t e = event_id[r0 + r];
    const int nd = node[r0 + r], kd = kind[r0 + r];
    int64_t t = -1;
    if (des_line_matches(kd, e, nd, vb, kDesBits1e16) && (e % 3 == 0 || e % 5 == 0 || e % 7 == 0))
      t = (int64_t)__longlong_as_double((long long)vb);
    s_time[r] = t;
    s_eid[r] = e;
    s_meta[r] = (uint32_t)nd | ((uint32_t)(kd == 1) << 31);
  }
  for (int i = tid; i < kMaxDim; i += kThreads) {
    s_q[i] = INT_MIN;                                       // no entry in queue_lengths yet
    s_ftime[i] = -1;                                        // no entry in future_events yet
    s_note[i] = i < dim ? note_levels[(int64_t)b * dim + i] : 0;
    if constexpr (PC) s_prog[i] = i < dim ? pc.instruments[(int64_t)b * dim + i] : 0;
  }
  __syncthreads();

  // ---- 2. the serial replay
  if (tid != 0) return;
  int64_t* out = notes + (int64_t)b * notes_cap * kCols;
  int64_t ticks = 0;
  int n = 0, err = 0;
  for (int r = 0; r < n_look && !err; ++r) {
    const int64_t mt = s_time[r];
    if (mt < 0) continue;
    const uint32_t m = s_meta[r];
    const int nd = (int)(m & 0x7FFFFFFFu);
    if ((m >> 31) == 0) {                                                  // arrival
      if (nd >= dim) continue;           // only the entry's existence matters for such a node: see the departure
      int q = s_q[nd];
      q = q == INT_MIN ? 1 : q + 1;
      s_q[nd] = q;
      if (q >= 127 && q < 254) q = min(127, max(0, 254 - q));
      else if (q >= 254) q = min(127, max(0, q % 127));
      const int64_t max_id = max((int64_t)1, pymod(30 + q, 127));
      int64_t cid = s_eid[r];
      if (cid >= max_id && cid < 2 * max_id) cid = min(max_id, max((int64_t)0, 2 * max_id - cid));
      else if (cid >= 2 * max_id) cid = min(max_id, max((int64_t)0, cid % max_id));
      s_ftime[nd] = mt;
      s_fvel[nd] = 60 + (int)(cid % 67);
      s_fsrv[nd] = q;
    } else {                                                               // departure
      bool has;
      if (nd < dim) {
        has = s_ftime[nd] >= 0;
      } else {                           // did a processed arrival name this node before?  (never, for DES-core logs)
        has = false;
        for (int k = 0; k < r && !has; ++k) has = s_time[k] >= 0 && s_meta[k] == (uint32_t)nd;
      }
      if (has) {
        if (nd >= dim) { err = GDM_DES_NOTES_ENODE; break; }
        if constexpr (PC) {                                                // the program_change is built first
          if (s_prog[nd] < 0 || s_prog[nd] > 127) { err = GDM_DES_NOTES_EPROGRAM; break; }
        }
        const int pitch = s_note[nd];
        if (pitch < 0 || pitch > 127) { err = GDM_DES_NOTES_EPITCH; break; }
        const int64_t on = s_ftime[nd];                                    // max(0, time): already >= 0
        const int64_t off = mt + max(0, s_fsrv[nd]);                       // time + (midi_time - time) + max(0, service)
        int64_t t_on;
        if constexpr (PC) {              // program_change + note_on, program_change + note_off: every delta twice
          if (on > ((pc.max_tick - ticks) >> 1)) { err = GDM_DES_NOTES_ELONG; break; }   // 2 on > room, before adding
          ticks += 2 * on;
          t_on = ticks;
          if (off > ((pc.max_tick - ticks) >> 1)) { err = GDM_DES_NOTES_ELONG; break; }
          ticks += 2 * off;
        } else {
          if (on > kMaxTick - ticks) { err = GDM_DES_NOTES_ELONG; break; }   // tested before adding: nothing overflows
          ticks += on;
          t_on = ticks;
          if (off > kMaxTick - ticks) { err = GDM_DES_NOTES_ELONG; break; }
          ticks += off;
        }
        if (n < notes_cap) {
          out[kCols * n + 0] = t_on;
          out[kCols * n + 1] = ticks;
          out[kCols * n + 2] = pitch;
          out[kCols * n + 3] = s_fvel[nd];
          if constexpr (PC) out[kCols * n + 4] = s_prog[nd];
          ++n;
        }
      }
      if (nd < dim) {
        const int q = s_q[nd];
        s_q[nd] = q == INT_MIN ? 0 : q - 1;
      }
    }
  }
  if (err) n = 0;
  n_notes[b] = n;
  if constexpr (PC) clip_len[b] = n > 0 ? (ticks * pc.mul) / pc.div + pc.tail : 0;    // ticks * mul <= 2^60
  else clip_len[b] = n > 0 ? ((ticks * 735) >> 3) + GDM_SYNTH_RELEASE : 0;
  status[b] = err;
}

}  // namespace

extern "C" int gdm_des_log_to_notes(const double* value, const int64_t* event_id, const int32_t* node,
                                    const int32_t* kind, const int64_t* rec_ptr, int64_t n_records,
                                    const int32_t* note_levels, int dim, int B, int64_t* notes, int notes_cap,
                                    int32_t* n_notes, int64_t* clip_len, int32_t* status, void* stream) {
  GDM_REQUIRE(rec_ptr && note_levels && notes && n_notes && clip_len && status, "gdm_des_log_to_notes: null pointer");
  GDM_REQUIRE(n_records >= 0 && (n_records == 0 || (value && event_id && node && kind)),
              "gdm_des_log_to_notes: records missing");
  GDM_REQUIRE(B > 0 && dim > 0 && dim <= GDM_DES_MIDI_MAX_NODES, "gdm_des_log_to_notes: need B > 0, 0 < dim <= %d",
              GDM_DES_MIDI_MAX_NODES);
  GDM_REQUIRE(notes_cap >= GDM_DES_NOTES_MAX, "gdm_des_log_to_notes: room for %d notes per sample, below %d", notes_cap,
              GDM_DES_NOTES_MAX);
  allow_lds(des_log_to_notes_kernel<false>, kLdsBytes);
  hipLaunchKernelGGL(des_log_to_notes_kernel<false>, dim3(B), dim3(kThreads), kLdsBytes, (hipStream_t)stream, value, event_id,
                     node, kind, rec_ptr, n_records, note_levels, dim, notes, notes_cap, n_notes, clip_len, status);
  GDM_LAUNCH_OK("gdm_des_log_to_notes");
  return GDM_OK;
}

extern "C" int gdm_des_log_to_notes_pc(const double* value, const int64_t* event_id, const int32_t* node,
                                       const int32_t* kind, const int64_t* rec_ptr, int64_t n_records,
                                       const int32_t* instruments, const int32_t* note_levels, int dim, int B,
                                       int64_t tick_mul, int64_t tick_div, int64_t tail, int64_t* notes, int notes_cap,
                                       int32_t* n_notes, int64_t* clip_len, int32_t* status, void* stream) {
  GDM_REQUIRE(rec_ptr && instruments && note_levels && notes && n_notes && clip_len && status,
              "gdm_des_log_to_notes_pc: null pointer");
  GDM_REQUIRE(n_records >= 0 && (n_records == 0 || (value && event_id && node && kind)),
              "gdm_des_log_to_notes_pc: records missing");
  GDM_REQUIRE(B > 0 && dim > 0 && dim <= GDM_DES_MIDI_MAX_NODES, "gdm_des_log_to_notes_pc: need B > 0, 0 < dim <= %d",
              GDM_DES_MIDI_MAX_NODES);
  GDM_REQUIRE(notes_cap >= GDM_DES_NOTES_MAX, "gdm_des_log_to_notes_pc: room for %d notes per sample, below %d",
              notes_cap, GDM_DES_NOTES_MAX);
  GDM_REQUIRE(tick_mul >= 1 && tick_mul <= (1 << 20) && tick_div >= 1 && tick_div <= (1 << 20) && tail >= 0 &&
                  tail <= ((int64_t)1 << 30),
              "gdm_des_log_to_notes_pc: sample(tick) = tick * %lld / %lld + a tail of %lld samples (1 .. 2^20 each, "
              "tail 0 .. 2^30)", (long long)tick_mul, (long long)tick_div, (long long)tail);
  GDM_REQUIRE(((uintptr_t)value & 7) == 0 && ((uintptr_t)event_id & 7) == 0 && ((uintptr_t)rec_ptr & 7) == 0 &&
                  ((uintptr_t)notes & 7) == 0 && ((uintptr_t)clip_len & 7) == 0 && ((uintptr_t)node & 3) == 0 &&
                  ((uintptr_t)kind & 3) == 0 && ((uintptr_t)instruments & 3) == 0 && ((uintptr_t)note_levels & 3) == 0 &&
                  ((uintptr_t)n_notes & 3) == 0 && ((uintptr_t)status & 3) == 0,
              "gdm_des_log_to_notes_pc: every array must be aligned to its elements");
  PcArgs pc;
  pc.instruments = instruments;
  pc.mul = tick_mul;
  pc.div = tick_div;
  pc.tail = tail;
  pc.max_tick = ((((int64_t)1 << 40) - tail) * tick_div) / tick_mul;       // sample(max_tick) + tail <= 2^40; < 2^60
  allow_lds((des_log_to_notes_kernel<true, PcArgs>), kLdsBytes);
  hipLaunchKernelGGL((des_log_to_notes_kernel<true, PcArgs>), dim3(B), dim3(kThreads), kLdsBytes, (hipStream_t)stream, value, event_id,
                     node, kind, rec_ptr, n_records, note_levels, dim, notes, notes_cap, n_notes, clip_len, status, pc);
  GDM_LAUNCH_OK("gdm_des_log_to_notes_pc");
  return GDM_OK;
}
