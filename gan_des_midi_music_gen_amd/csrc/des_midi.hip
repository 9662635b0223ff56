// DES log -> MIDI track -> piano-roll planes for a batch of samples in ONE launch (the consumer behind the DES core:
// process_adjsim_log / MidiGenerator, MMGAN_MIDI_DES/sim_log_to_midi.py:14-277, and generate_piano_roll on the file it
// builds, datasets.py:13-54).  One workgroup per sample:
//
//   1. all 256 threads clear the sample's two planes and STAGE its records: each of the (at most 5000) records the
//      reference's reader looks at is reduced to one 32-bit word in LDS -- does the reference's regex match the line's
//      text, does the event id pass the three skip moduli, int(value), node, kind, and the note velocity (a pure
//      function of the event id and the sample's parameters).  Everything that does not depend on the running state is
//      done here, in parallel and with coalesced loads.
//   2. ONE lane replays the words in order: the running previous_time, the per-node queue counts and future_events,
//      program changes, the 500-message limit; then save_midi (remove-while-iterating, end_of_track, clean_midi_file)
//      and the tick -> second -> step conversion of generate_piano_roll.  This is a dependent chain by construction
//      (every message's time depends on the one before); its latency is the kernel's bound.
//   3. thread `note` rasters its row (last write wins), all threads copy the track out.
//
// The np.random.randint fallbacks of MidiGenerator.__init__ (lines 24-31) are unreachable -- skip_k = max(2, .) is never
// 0 -- and are not built.  The 'processing' branch of process_line is dead too: the reader's regex never matches such a
// line.
#include "des_log.h"

namespace {

constexpr int kMaxLines = 5000;          // process_adjsim_log: `max = 5000`
constexpr int kTrackLimit = 500;         // process_line: len(self.track) < 500
constexpr int kThreads = 256;
constexpr int kMaxDim = GDM_DES_MIDI_MAX_NODES;
constexpr uint32_t kInactive = 0xFFFFFFFFu;
constexpr uint32_t kNoNode = 0x3FFF;     // node >= dim: the reference's dict lookups raise KeyError for it

struct Params {
  int skip1, skip2, skip3, base, tempo, var, key, err;
};

// int(np.float32 * python int): the product is rounded to float32 (NumPy >= 2 scalar promotion), then truncated.
// Finite-ness is tested on the bits: this library is compiled without NaN semantics.
__device__ __forceinline__ bool f32_int(float g, float k, int* out) {
  const float x = g * k;
  const uint32_t bits = __float_as_uint(x);
  if (((bits >> 23) & 0xFF) == 0xFF || fabsf(x) >= 2147483648.f) return false;
  *out = (int)x;
  return true;
}

__device__ Params midi_params(const float* g) {
  Params p;
  p.err = 0;
  int v = 0;
  bool ok = true;
  ok &= f32_int(g[0], 10.f, &v);  p.skip1 = max(2, v);
  ok &= f32_int(g[1], 10.f, &v);  p.skip2 = max(2, v);
  ok &= f32_int(g[2], 10.f, &v);  p.skip3 = max(2, v);
  ok &= f32_int(g[3], 90.f, &v);  p.base = v < 50 ? 80 : v;
  {
    const float x = g[4] * 1000000.f;                       // min(int(.), 16777215): any large value is capped
    const uint32_t bits = __float_as_uint(x);
    if (((bits >> 23) & 0xFF) == 0xFF) ok = false;
    v = (ok && x < 16777215.f) ? (x > -2147483648.f ? (int)x : -1) : 16777215;
    p.tempo = v == 0 ? 500000 : v;
    if (p.tempo < 0) ok = false;                            // MetaMessage('set_tempo') refuses it
  }
  ok &= f32_int(g[5], 63.f, &v);  p.var = v == 0 ? 30 : v;
  ok &= f32_int(g[5], 11.f, &v);  p.key = (int)pymod(v, 11);
  if (!ok) p.err = GDM_DES_MIDI_EPARAMS;
  return p;
}

__global__ __launch_bounds__(kThreads) void des_log_to_roll_kernel(
    const double* __restrict__ value, const int64_t* __restrict__ event_id, const int32_t* __restrict__ node,
    const int32_t* __restrict__ kind, const int64_t* __restrict__ rec_ptr, int64_t n_records,
    const float* __restrict__ tails, int tail_stride, const int32_t* __restrict__ instruments,
    const int32_t* __restrict__ note_levels, int dim, const int32_t* __restrict__ save, int width, int col0, int W,
    int sequence_length, float* __restrict__ planes, int32_t* __restrict__ track_out, int track_cap,
    int32_t* __restrict__ track_len, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ uint32_t s_rec[kMaxLines];
  __shared__ int4 s_track[GDM_DES_MIDI_TRACK_CAP];
  __shared__ uint32_t s_ev[GDM_DES_MIDI_TRACK_CAP];          // step << 16 | vel (255: note_off) << 8 | note
  __shared__ int s_q[kMaxDim], s_ftime[kMaxDim], s_fvel[kMaxDim], s_fsrv[kMaxDim];
  __shared__ int s_inst[kMaxDim], s_note[kMaxDim];           // the sample's rows: read inside the serial chain
  __shared__ int s_on[128];
  __shared__ int s_ntrack, s_nev;

  const int b = blockIdx.x, tid = threadIdx.x;
  const Params p = midi_params(tails + (int64_t)b * tail_stride);      // same in every thread

  // ---- 1a. clear the planes (256 * W floats per sample: always a multiple of 4 floats and 16-byte aligned)
  {
    float4* pl = reinterpret_cast<float4*>(planes + (int64_t)b * 256 * W);
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < 64 * W; i += kThreads) pl[i] = z;
  }
  // ---- 1b. stage the records
  int64_t r0 = rec_ptr[b], r1 = rec_ptr[b + 1];
  r0 = min(max(r0, (int64_t)0), n_records);
  r1 = min(max(r1, r0), n_records);
  const int n_look = (int)min(r1 - r0, (int64_t)kMaxLines);
  constexpr uint64_t kBits200 = 0x4069000000000000ULL;      // 200.0
  for (int r = tid; r < n_look; r += kThreads) {
    const uint64_t vb = (uint64_t)__double_as_longlong(value[r0 + r]);
    const int64_t e = event_id[r0 + r];
    const int nd = node[r0 + r], kd = kind[r0 + r];
    // values in [200, 1e16) match the regex but fail `midi_time < 200`: inactive either way
    const bool live = des_line_matches(kd, e, nd, vb, kBits200);
    uint32_t w = kInactive;
    if (live && (e % p.skip1 == 0 || e % p.skip2 == 0 || e % p.skip3 == 0)) {
      const int mt = (int)__longlong_as_double((long long)vb);          // max(0, int(float(.))), < 200
      const int64_t max_id = (int64_t)p.base + p.var;
      int64_t cid = (int64_t)p.base - p.var + e;
      uint32_t zero_div = 0;
      if (cid > max_id) {
        if (max_id == 0) { zero_div = 1; cid = 0; }
        else cid = max_id - pymod(cid, max_id);
      }
      const uint32_t vel = (uint32_t)pymod(cid, 126);
      const uint32_t nf = nd < dim ? (uint32_t)nd : kNoNode;
      w = (uint32_t)mt | (vel << 8) | ((uint32_t)kd << 15) | (nf << 16) | (zero_div << 30);
    }
    s_rec[r] = w;
  }
  for (int i = tid; i < kMaxDim; i += kThreads) {
    s_q[i] = INT_MIN;
    s_ftime[i] = INT_MIN;
    if (i < dim) {
      s_inst[i] = instruments[(int64_t)b * dim + i];
      s_note[i] = note_levels[(int64_t)b * dim + i];
    }
  }
  if (tid < 128) s_on[tid] = 0;
  __syncthreads();

  // ---- 2. the serial replay
  if (tid == 0) {
    const int* inst = s_inst;
    const int* notes = s_note;
    int err = p.err, nt = 0, nev = 0;
    const int do_save = save[b] != 0;
    if (!err) {
      s_track[0] = make_int4(GDM_MIDI_SET_TEMPO, p.tempo, 0, 0);
      s_track[1] = make_int4(GDM_MIDI_TIME_SIGNATURE, 4, 4, 0);
      s_track[2] = make_int4(GDM_MIDI_KEY_SIGNATURE, p.key, 0, 0);
      s_track[3] = make_int4(GDM_MIDI_PROGRAM_CHANGE, 0, 0, 0);
      nt = 4;
      int prev = 0, cur_inst = 0;
      for (int r = 0; r < n_look && nt < kTrackLimit && !err; ++r) {
        const uint32_t w = s_rec[r];
        if (w == kInactive) continue;
        int mt = (int)(w & 0xFF);
        if (prev > mt) mt = prev;
        const int nd = (int)((w >> 16) & 0x3FFF);
        if (((w >> 15) & 1) == 0) {                                      // arrival
          if (nd == (int)kNoNode) { err = GDM_DES_MIDI_ENODE; break; }
          if ((w >> 30) & 1) { err = GDM_DES_MIDI_EMODULO; break; }
          int q = s_q[nd];
          q = q == INT_MIN ? 1 : q + 1;
          s_q[nd] = q;
          if (q >= 127 && q < 254) q = min(127, max(0, 254 - q));
          else if (q >= 254) q = min(127, max(0, q % 127));
          const int vel = (int)((w >> 8) & 0x7F);
          s_ftime[nd] = mt;
          s_fvel[nd] = vel;
          s_fsrv[nd] = q;
          prev = mt;                                                     // on_time = max(previous_time, midi_time)
          const int in = inst[nd], nl = notes[nd];
          if (in < 0 || in > 127 || nl < 0 || nl > 127) { err = GDM_DES_MIDI_ERANGE; break; }
          if (cur_inst != in) {
            cur_inst = in;
            s_track[nt++] = make_int4(GDM_MIDI_PROGRAM_CHANGE, in, 0, mt);
          }
          s_track[nt++] = make_int4(GDM_MIDI_NOTE_ON, nl, vel, mt);
        } else if (nd != (int)kNoNode) {                                 // departure
          if (s_ftime[nd] != INT_MIN) {
            const int t0 = s_ftime[nd];
            const int off = max(prev, t0 + (mt - t0) + max(0, s_fsrv[nd]));
            prev = off;
            const int in = inst[nd];
            if (cur_inst != in) {
              cur_inst = in;
              s_track[nt++] = make_int4(GDM_MIDI_PROGRAM_CHANGE, in, 0, off);
            }
            s_track[nt++] = make_int4(GDM_MIDI_NOTE_OFF, notes[nd], s_fvel[nd], off);
          }
          const int q = s_q[nd];
          s_q[nd] = q == INT_MIN ? 0 : q - 1;
        }
      }
    }
    if (err) nt = 0;
    if (!err && do_save) {
      // save_midi: `for msg in track: if msg.time > 200: track.remove(msg)` -- the list shrinks under the iterator, so
      // the message after a removed one is never looked at.  (mido's remove() takes the first EQUAL message, not this
      // one; message times never decrease along the track, so every message from the first time > 200 on is dropped by
      // clean_midi_file below whichever of two equal messages went first: the saved track is the same.)
      int wr = 0;
      for (int r = 0; r < nt;) {
        if (s_track[r].w > 200) {
          if (r + 1 < nt) s_track[wr++] = s_track[r + 1];
          r += 2;
        } else {
          s_track[wr++] = s_track[r];
          r += 1;
        }
      }
      s_track[wr++] = make_int4(GDM_MIDI_END_OF_TRACK, 0, 0, 0);
      nt = wr;
      // clean_midi_file: a note_on of a sounding note and a note_off of a silent one go; "sounding" is a non-zero
      // note_on TIME, so a note_on at time 0 does not count
      wr = 0;
      for (int r = 0; r < nt; ++r) {
        const int4 m = s_track[r];
        bool drop = false;
        if (m.x == GDM_MIDI_NOTE_ON) {
          if (s_on[m.y] > 0) drop = true; else s_on[m.y] = m.w;
        } else if (m.x == GDM_MIDI_NOTE_OFF) {
          if (s_on[m.y] == 0) drop = true; else s_on[m.y] = 0;
        }
        if (m.w > 200) drop = true;
        if (!drop) s_track[wr++] = m;
      }
      nt = wr;
      // generate_piano_roll's event loop: message times are DELTA ticks to mido (480 per beat); a delta is converted with
      // the tempo in force before the message; seconds accumulate in float64 in message order
      double scale = 500000 * 1e-6 / 480.0, t = 0.0;
      for (int r = 0; r < nt; ++r) {
        const int4 m = s_track[r];
        if (m.x == GDM_MIDI_END_OF_TRACK) continue;
        const double sec = m.w > 0 ? (double)m.w * scale : 0.0;
        t = t + sec;
        if (m.x == GDM_MIDI_SET_TEMPO) scale = (double)m.y * 1e-6 / 480.0;
        const double rs = __builtin_rint(t);                              // int(round(.)): half to even
        if (rs >= (double)sequence_length) break;
        const int step = (int)rs;
        if (m.x == GDM_MIDI_NOTE_ON) {
          if (step >= width) break;                                       // IndexError inside the reference's bare try
          s_ev[nev++] = ((uint32_t)step << 16) | ((uint32_t)m.z << 8) | (uint32_t)m.y;
        } else if (m.x == GDM_MIDI_NOTE_OFF) {
          s_ev[nev++] = ((uint32_t)step << 16) | (255u << 8) | (uint32_t)m.y;
        }
      }
    }
    s_ntrack = nt;
    s_nev = nev;
    status[b] = (err << 8) | ((!err && do_save) ? 1 : 0);
    track_len[b] = nt;
  }
  __syncthreads();

  // ---- 3. raster (thread = note row) and track copy
  const int nt = s_ntrack, nev = s_nev;
  if (tid < 128 && nev > 0) {
    float* r = planes + ((int64_t)b * 256 + tid) * W;
    float* d = r + (int64_t)128 * W;
    int on = 0;                                                           // note_on_time = np.zeros(128)
    for (int i = 0; i < nev; ++i) {
      const uint32_t ev = s_ev[i];
      if ((int)(ev & 0xFF) != tid) continue;
      const int step = (int)(ev >> 16), vel = (int)((ev >> 8) & 0xFF);
      if (vel != 255) {
        const int c = step - col0;                                        // step < width; the final slice starts at col0
        if (c >= 0 && c < W) r[c] = (float)vel;
        on = step;
      } else {
        const float len = (float)(step - on);
        for (int s = max(on, col0); s < step && s - col0 < W; ++s) d[s - col0] = len;
      }
    }
  }
  int4* out = reinterpret_cast<int4*>(track_out) + (int64_t)b * track_cap;
  for (int i = tid; i < nt && i < track_cap; i += kThreads) out[i] = s_track[i];
}

}  // namespace

extern "C" int gdm_des_log_to_roll(const double* value, const int64_t* event_id, const int32_t* node,
                                   const int32_t* kind, const int64_t* rec_ptr, int64_t n_records, const float* tails,
                                   int tail_stride, const int32_t* instruments, const int32_t* note_levels, int dim,
                                   const int32_t* save, int B, int start, int end, int sequence_length, float* planes,
                                   int W, int32_t* track, int track_cap, int32_t* track_len, int32_t* status,
                                   void* stream) {
  GDM_REQUIRE(rec_ptr && tails && instruments && note_levels && save && planes && track && track_len && status,
              "gdm_des_log_to_roll: null pointer");
  GDM_REQUIRE(n_records >= 0 && (n_records == 0 || (value && event_id && node && kind)),
              "gdm_des_log_to_roll: records missing");
  GDM_REQUIRE(B > 0 && dim > 0 && dim <= GDM_DES_MIDI_MAX_NODES && tail_stride >= 6,
              "gdm_des_log_to_roll: need B > 0, 0 < dim <= %d, at least 6 tail values", GDM_DES_MIDI_MAX_NODES);
  GDM_REQUIRE(((uintptr_t)planes & 15) == 0 && ((uintptr_t)track & 15) == 0,
              "gdm_des_log_to_roll: planes and track must be 16-byte aligned (written with 16-byte stores)");
  GDM_REQUIRE(track_cap >= GDM_DES_MIDI_TRACK_CAP, "gdm_des_log_to_roll: track capacity below %d",
              GDM_DES_MIDI_TRACK_CAP);
  const int width = end - start;
  GDM_REQUIRE(width > 0 && width < 32768 && sequence_length >= 0 && sequence_length < 32768 && start >= 0,
              "gdm_des_log_to_roll: bad window");
  // generate_piano_roll's last lines: `[:, start:end]` of the already end - start wide planes if end < 128 (the
  // comparison is with the number of ROWS), else `[:, :end]`
  const int col0 = end < 128 ? (start < width ? start : width) : 0;
  const int col1 = end < width ? end : width;
  GDM_REQUIRE(W == col1 - col0 && W > 0, "gdm_des_log_to_roll: W = %d, but the reference's final slice leaves %d columns",
              W, col1 - col0);
  hipLaunchKernelGGL(des_log_to_roll_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, value, event_id, node,
                     kind, rec_ptr, n_records, tails, tail_stride, instruments, note_levels, dim, save, width, col0, W,
                     sequence_length, planes, track, track_cap, track_len, status);
  GDM_LAUNCH_OK("gdm_des_log_to_roll");
  return GDM_OK;
}
