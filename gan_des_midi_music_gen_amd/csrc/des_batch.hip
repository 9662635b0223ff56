// The discrete-event simulator of des_sim.h for a BATCH of samples on the device: the stage between the batched
// prologue (des_prologue.hip: gdm_des_routing writes the routing matrices this kernel reads) and the batched log
// consumers (des_midi.hip, des_notes.hip), so that neither the routing matrices nor the event logs visit the host.
//
// One simulation is one dependent chain of events: there is nothing to spread over lanes inside it.  The mapping is one
// WAVE (a 64-thread workgroup) per sample:
//   * all lanes stage the per-node parameters in LDS, build the routing tables (one node per lane) and seed the node
//     generators (one 624-step recurrence per lane);
//   * lane 0 then runs the chain -- the same des::Sim<MathPortable> code the host mirror gdm_des_run_batch_host runs, so
//     the two agree bit for bit -- and writes the records with ordinary vector stores, sample b at b * max_records;
//   * a one-workgroup pack kernel scans the B counts into rec_ptr and closes the gaps in place (no gap, no copy: a
//     sample that reaches the record cap, which is what the bridges' runs do, already sits where the CSR wants it).
// LDS holds the event list, the per-node scalars, the global generator and the seeder; the node generators live there
// too when dim <= kLdsGenDim (15 nodes: 37 KB), otherwise in the caller's workspace together with the routing tables
// and the FIFO rings (L2-resident: about 330 KB per sample at dim 61, capacity 254).
// The prologue up to the chain, the LDS block and the workspace layout are des_wave.h's, shared with the log-free
// statistics kernel of des_stats.hip.
// Bounds: every index the chain computes is checked in des_sim.h before it forms an address; every loop is bounded by
// max_events, max_records or the draw budget.
#include "gdm_common.h"
#include "des_sim.h"
#include "des_wave.h"

#pragma clang fp contract(off)

namespace {

using des_wave::kMaxDim;
using des_wave::ws_layout;
constexpr int kPackThreads = 256;
typedef des::Sim<des::MathPortable, des::OutSoa> DevSim;

__global__ __launch_bounds__(GDM_WAVE) void des_batch_kernel(
    const double* __restrict__ adj, int dim, const double* __restrict__ loc, const double* __restrict__ scale,
    const int32_t* __restrict__ queue_cap, const int64_t* __restrict__ seed,
    const int64_t* __restrict__ number_of_customers, int max_queue_cap, int64_t max_events, int64_t max_records,
    uint32_t* __restrict__ mt_key, int32_t* __restrict__ mt_pos, int32_t* __restrict__ mt_has_gauss,
    double* __restrict__ mt_gauss, double* __restrict__ value, int64_t* __restrict__ event_id,
    int32_t* __restrict__ node, int32_t* __restrict__ kind, int64_t* __restrict__ n_records,
    int32_t* __restrict__ stop_reason, unsigned char* __restrict__ workspace) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];       // node generators when dim <= kLdsGenDim
  __shared__ des_wave::Lds lds;

  const int b = blockIdx.x, lane = threadIdx.x;
  const des_wave::WsLayout w = ws_layout(dim, max_queue_cap, false);
  unsigned char* ws = workspace + (size_t)b * w.per_sample;

  DevSim s;
  const int64_t rec0 = (int64_t)b * max_records;
  s.out = des::OutSoa{value + rec0, event_id + rec0, node + rec0, kind + rec0};
  s.out_cap = max_records;
  s.max_records = max_records;
  // ---- all lanes: the shared prologue (des_wave.h)
  const bool ok = des_wave::prologue(s, lds, s_dyn, ws, w, b, lane, adj, dim, loc, scale, queue_cap, seed, max_queue_cap,
                                     max_events, mt_key, mt_pos, mt_has_gauss, mt_gauss);
  // ---- lane 0: the chain
  if (lane == 0) {
    int reason = DES_STOP_ERROR;
    int64_t n = 0;
    if (ok) {
      reason = s.run(number_of_customers[b], max_events);
      des_wave::store_generator_scalars(lds, dim, b, mt_pos, mt_has_gauss, mt_gauss);
      n = reason == DES_STOP_ERROR ? 0 : (s.n_out < max_records ? s.n_out : max_records);
    }
    n_records[b] = n;
    stop_reason[b] = reason;
  }
  __syncthreads();
  if (ok) des_wave::store_generator_words(lds, b, lane, mt_key);
}

// counts -> rec_ptr (exclusive scan, one workgroup), then the records of sample b move from b * max_records down to
// rec_ptr[b].  A destination never lies above its source and a sample's destination range ends at or below the next
// sample's source, so ascending samples and ascending chunks -- each chunk read completely before it is written -- are
// safe in place.
__global__ __launch_bounds__(kPackThreads) void des_pack_kernel(int B, int64_t max_records,
                                                                const int64_t* __restrict__ n_records,
                                                                int64_t* __restrict__ rec_ptr, double* value,
                                                                int64_t* event_id, int32_t* node, int32_t* kind) {
  __shared__ int64_t s_scan[kPackThreads];
  const int t = threadIdx.x;
  int64_t carry = 0;
  for (int base = 0; base < B; base += kPackThreads) {
    int64_t v = 0;
    if (base + t < B) {
      v = n_records[base + t];
      v = v < 0 ? 0 : (v > max_records ? max_records : v);
    }
    s_scan[t] = v;
    __syncthreads();
    for (int off = 1; off < kPackThreads; off <<= 1) {
      const int64_t x = t >= off ? s_scan[t - off] : 0;
      __syncthreads();
      s_scan[t] += x;
      __syncthreads();
    }
    if (base + t < B) rec_ptr[base + t + 1] = carry + s_scan[t];
    carry += s_scan[kPackThreads - 1];
    __syncthreads();
  }
  if (t == 0) rec_ptr[0] = 0;
  __syncthreads();
  for (int b = 1; b < B; ++b) {
    const int64_t dst = rec_ptr[b], n = rec_ptr[b + 1] - dst, src = (int64_t)b * max_records;
    if (dst == src || n <= 0) continue;                 // uniform over the workgroup
    for (int64_t c = 0; c < n; c += kPackThreads) {
      const int64_t i = c + t;
      double v = 0.0;
      int64_t e = 0;
      int32_t nd = 0, kd = 0;
      if (i < n) {
        v = value[src + i];
        e = event_id[src + i];
        nd = node[src + i];
        kd = kind[src + i];
      }
      __syncthreads();
      if (i < n) {
        value[dst + i] = v;
        event_id[dst + i] = e;
        node[dst + i] = nd;
        kind[dst + i] = kd;
      }
      __syncthreads();
    }
  }
}

__global__ void des_math_probe_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ log_out,
                                      double* __restrict__ factor_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double l = des::MathPortable::log(x[i]);
  log_out[i] = l;
  factor_out[i] = des::MathPortable::sqrt(-2.0 * l / x[i]);
}

}  // namespace

extern "C" int64_t gdm_des_batch_workspace_bytes(int B, int dim, int max_queue_cap) {
  if (B < 1 || dim < 1 || dim > kMaxDim || max_queue_cap < 1 || max_queue_cap > GDM_DES_BATCH_MAX_QUEUE_CAP) return -1;
  return (int64_t)(ws_layout(dim, max_queue_cap, false).per_sample * (size_t)B);
}

extern "C" int gdm_des_run_batch(const double* adj, int B, int dim, const double* loc, const double* scale,
                                 const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                                 int max_queue_cap, int64_t max_events, int64_t max_records, uint32_t* mt_key,
                                 int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss, double* value,
                                 int64_t* event_id, int32_t* node, int32_t* kind, int64_t n_records_cap,
                                 int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  GDM_REQUIRE(adj && loc && scale && queue_cap && seed && number_of_customers && mt_key && mt_pos && has_gauss &&
                  cached_gauss && value && event_id && node && kind && rec_ptr && n_records && stop_reason && workspace,
              "gdm_des_run_batch: null pointer");
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && dim >= 1 && dim <= kMaxDim && max_queue_cap >= 1 &&
                  max_queue_cap <= GDM_DES_BATCH_MAX_QUEUE_CAP,
              "gdm_des_run_batch: B >= 1, 1 <= dim <= %d, 1 <= max_queue_cap <= %d", kMaxDim, GDM_DES_BATCH_MAX_QUEUE_CAP);
  GDM_REQUIRE(max_events >= 1 && max_events <= GDM_DES_BATCH_MAX_EVENTS,
              "gdm_des_run_batch: max_events must be in 1..%lld", (long long)GDM_DES_BATCH_MAX_EVENTS);
  GDM_REQUIRE(max_records >= 1 && max_records <= ((int64_t)1 << 31),
              "gdm_des_run_batch: a record cap is required (max_records >= 1)");
  GDM_REQUIRE(n_records_cap >= (int64_t)B * max_records,
              "gdm_des_run_batch: the record arrays must hold B * max_records = %lld records",
              (long long)((int64_t)B * max_records));
  const int64_t need = gdm_des_batch_workspace_bytes(B, dim, max_queue_cap);
  if (need < 0 || workspace_bytes < (size_t)need || ((uintptr_t)workspace & 15)) {
    gdm_set_error("gdm_des_run_batch: workspace too small or not 16-byte aligned (%lld bytes needed)", (long long)need);
    return GDM_EWORKSPACE;
  }
  const size_t lds_dyn = des_wave::lds_dyn_bytes(dim);
  hipLaunchKernelGGL(des_batch_kernel, dim3(B), dim3(GDM_WAVE), lds_dyn, (hipStream_t)stream, adj, dim, loc, scale,
                     queue_cap, seed, number_of_customers, max_queue_cap, max_events, max_records, mt_key, mt_pos,
                     has_gauss, cached_gauss, value, event_id, node, kind, n_records, stop_reason,
                     (unsigned char*)workspace);
  GDM_LAUNCH_OK("gdm_des_run_batch");
  return gdm_des_pack(B, max_records, n_records, rec_ptr, value, event_id, node, kind, stream);
}

extern "C" int gdm_des_pack(int B, int64_t max_records, const int64_t* n_records, int64_t* rec_ptr, double* value,
                            int64_t* event_id, int32_t* node, int32_t* kind, void* stream) {
  GDM_REQUIRE(n_records && rec_ptr && value && event_id && node && kind, "gdm_des_pack: null pointer");
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && max_records >= 1 && max_records <= ((int64_t)1 << 31),
              "gdm_des_pack: bad arguments");
  hipLaunchKernelGGL(des_pack_kernel, dim3(1), dim3(kPackThreads), 0, (hipStream_t)stream, B, max_records, n_records,
                     rec_ptr, value, event_id, node, kind);
  GDM_LAUNCH_OK("gdm_des_pack");
  return GDM_OK;
}

extern "C" int gdm_des_math_probe(const double* x, int64_t n, double* log_out, double* factor_out, void* stream) {
  GDM_REQUIRE(n >= 0 && n <= ((int64_t)1 << 30) && (n == 0 || (x && log_out && factor_out)),
              "gdm_des_math_probe: bad arguments");
  if (n == 0) return GDM_OK;
  hipLaunchKernelGGL(des_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n,
                     log_out, factor_out);
  GDM_LAUNCH_OK("gdm_des_math_probe");
  return GDM_OK;
}
