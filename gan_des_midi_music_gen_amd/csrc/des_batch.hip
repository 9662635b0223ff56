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
// One kernel template over one body (batch_sample), instantiated for the three node policies of des_wave.h:
// des_batch_kernel<NormalOnly> draws 'normal' only (the bridges' nets); des_batch_kernel<AnyDist> takes a kind per node
// (normal, exponential, uniform), its row staged into LDS (512 B more), and leaves the generator state of a sample that
// errors as it came; des_batch_kernel<AnyNode> is that kernel with the reference's 'queue' and 'branch' nodes as well
// (kinds and node state, 2 KB of LDS).  (Older texts call the three des_batch_kernel, des_batch_dist_kernel,
// des_batch_net_kernel.)  One launcher template (launch_batch) is behind the three entries.
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

// the inputs and outputs the kernels share
struct BatchArgs {
  const double* adj;
  int dim;
  const double *loc, *scale;
  const int32_t* queue_cap;
  const int64_t *seed, *number_of_customers;
  int max_queue_cap;
  int64_t max_events, max_records;
  uint32_t* mt_key;
  int32_t *mt_pos, *mt_has_gauss;
  double *mt_gauss, *value;
  int64_t* event_id;
  int32_t *node, *kind;
  int64_t* n_records;
  int32_t* stop_reason;
  unsigned char* workspace;
};

// One sample, every lane of its wave.  s.dist is the caller's (what it points to is staged before the call: the
// prologue's first barrier orders it before lane 0 reads it).  kErrorKeepsState: a sample whose chain ends in
// DES_STOP_ERROR leaves the generator state as it came (the entries with kinds, as the statistics kernels); without
// it the state is written back whenever the spec passed the prologue's checks (gdm_des_run_batch, as ever).
template <bool kErrorKeepsState, class SimT>
__device__ __forceinline__ void batch_sample(SimT& s, des_wave::Lds& lds, unsigned char* s_dyn, const BatchArgs& a) {
  const int b = blockIdx.x, lane = threadIdx.x, dim = a.dim;
  const int64_t max_records = a.max_records;
  const des_wave::WsLayout w = ws_layout(dim, a.max_queue_cap, false);
  unsigned char* ws = a.workspace + (size_t)b * w.per_sample;

  const int64_t rec0 = (int64_t)b * max_records;
  s.out = des::OutSoa{a.value + rec0, a.event_id + rec0, a.node + rec0, a.kind + rec0};
  s.out_cap = max_records;
  s.max_records = max_records;
  // ---- all lanes: the shared prologue (des_wave.h)
  const bool ok = des_wave::prologue(s, lds, s_dyn, ws, w, b, lane, a.adj, dim, a.loc, a.scale, a.queue_cap, a.seed,
                                     a.max_queue_cap, a.max_events, a.mt_key, a.mt_pos, a.mt_has_gauss, a.mt_gauss);
  // ---- lane 0: the chain
  if (lane == 0) {
    int reason = DES_STOP_ERROR;
    int64_t n = 0;
    if (ok) {
      reason = s.run(a.number_of_customers[b], a.max_events);
      if (!kErrorKeepsState || reason != DES_STOP_ERROR)
        des_wave::store_generator_scalars(lds, dim, b, a.mt_pos, a.mt_has_gauss, a.mt_gauss);
      n = reason == DES_STOP_ERROR ? 0 : (s.n_out < max_records ? s.n_out : max_records);
    }
    a.n_records[b] = n;
    a.stop_reason[b] = reason;
    if (kErrorKeepsState) lds.ok = reason != DES_STOP_ERROR;
  }
  __syncthreads();
  if (kErrorKeepsState ? lds.ok != 0 : ok) des_wave::store_generator_words(lds, b, lane, a.mt_key);
}

// The kernels' parameter list and the BatchArgs of it, under the names the entries below use too.  Kernel parameters
// stay plain __restrict__ pointers: with the struct as the parameter the compiler loses the no-alias facts and the
// kernels come out longer.
#define DES_BATCH_PARAMS                                                                                               \
  const double *__restrict__ adj, int dim, const double *__restrict__ loc, const double *__restrict__ scale,           \
      const int32_t *__restrict__ queue_cap, const int64_t *__restrict__ seed,                                         \
      const int64_t *__restrict__ number_of_customers, int max_queue_cap, int64_t max_events, int64_t max_records,     \
      uint32_t *__restrict__ mt_key, int32_t *__restrict__ mt_pos, int32_t *__restrict__ mt_has_gauss,                 \
      double *__restrict__ mt_gauss, double *__restrict__ value, int64_t *__restrict__ event_id,                       \
      int32_t *__restrict__ node, int32_t *__restrict__ kind, int64_t *__restrict__ n_records,                         \
      int32_t *__restrict__ stop_reason, unsigned char *__restrict__ workspace
#define DES_BATCH_ARGS                                                                                                 \
  BatchArgs {                                                                                                          \
    adj, dim, loc, scale, queue_cap, seed, number_of_customers, max_queue_cap, max_events, max_records, mt_key,        \
        mt_pos, mt_has_gauss, mt_gauss, value, event_id, node, kind, n_records, stop_reason,                           \
        (unsigned char*)workspace                                                                                      \
  }

// One kernel per node policy (des_wave.h) over that body.  flatten, as des_stats_kernel: three kinds at three draw sites
// exceed the inliner's budget, and a chain function left out of line takes the Sim by address -- scratch per lane and a
// load for every member; inlined whole there is no scratch.  The policy's block is staged before the prologue, whose
// first barrier orders it before lane 0 reads it.  The policies with kinds keep the generator state of a sample that
// errors (kErrorKeepsState above).
template <class Policy>
__global__ __launch_bounds__(GDM_WAVE) __attribute__((flatten)) void des_batch_kernel(
    DES_BATCH_PARAMS, const int32_t* __restrict__ node_kind) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];       // node generators when dim <= kLdsGenDim
  __shared__ des_wave::Lds lds;
  __shared__ typename Policy::Block pl;
  des::Sim<des::MathPortable, des::OutSoa, des::NoStats, typename Policy::Dist> s;
  Policy::stage(s.dist, pl, node_kind, dim, blockIdx.x, threadIdx.x);
  batch_sample<Policy::kHasKind>(s, lds, s_dyn, DES_BATCH_ARGS);
}

// des_wave::AnyDist keeps the statement order its kernel always had, the kinds staged in the kernel's own body: through
// AnyDist::stage the compiler schedules the chain differently (83 VGPRs for 95, 142 instructions more), and at B = 256
// that kernel measured 0.5 % above the parent's where the parent's two runs lay 0.2 % apart (DESIGN.md section 7,
// f19).  This form gives the parent's kernel, instruction for instruction.
template <>
__global__ __launch_bounds__(GDM_WAVE) __attribute__((flatten)) void des_batch_kernel<des_wave::AnyDist>(
    DES_BATCH_PARAMS, const int32_t* __restrict__ dist_kind) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ des_wave::Lds lds;
  __shared__ des_wave::DistLds dl;
  for (int i = threadIdx.x; i < dim; i += GDM_WAVE) dl.kind[i] = dist_kind[(int64_t)blockIdx.x * dim + i];
  des::Sim<des::MathPortable, des::OutSoa, des::NoStats, des::AnyDist> s;
  s.dist.kind = dl.kind;
  batch_sample<true>(s, lds, s_dyn, DES_BATCH_ARGS);
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

// The checks the device entries make on the host; `who` names the entry in the message.  They check less than the
// statistics entries (no alignment of the arrays but `kind`): adding that is a change of behaviour, left for another day.
static int check_batch_args(const char* who, const BatchArgs& a, int B, const int32_t* dist_kind, bool with_kind,
                            int64_t n_records_cap, const int64_t* rec_ptr, size_t workspace_bytes) {
  GDM_REQUIRE(a.adj && a.loc && a.scale && a.queue_cap && a.seed && a.number_of_customers && a.mt_key && a.mt_pos &&
                  a.mt_has_gauss && a.mt_gauss && a.value && a.event_id && a.node && a.kind && rec_ptr && a.n_records &&
                  a.stop_reason && a.workspace && (dist_kind || !with_kind),
              "%s: null pointer", who);
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && a.dim >= 1 && a.dim <= kMaxDim && a.max_queue_cap >= 1 &&
                  a.max_queue_cap <= GDM_DES_BATCH_MAX_QUEUE_CAP,
              "%s: B >= 1, 1 <= dim <= %d, 1 <= max_queue_cap <= %d", who, kMaxDim, GDM_DES_BATCH_MAX_QUEUE_CAP);
  GDM_REQUIRE(a.max_events >= 1 && a.max_events <= GDM_DES_BATCH_MAX_EVENTS, "%s: max_events must be in 1..%lld", who,
              (long long)GDM_DES_BATCH_MAX_EVENTS);
  GDM_REQUIRE(a.max_records >= 1 && a.max_records <= ((int64_t)1 << 31),
              "%s: a record cap is required (max_records >= 1)", who);
  GDM_REQUIRE(n_records_cap >= (int64_t)B * a.max_records,
              "%s: the record arrays must hold B * max_records = %lld records", who,
              (long long)((int64_t)B * a.max_records));
  GDM_REQUIRE(((uintptr_t)dist_kind & 3) == 0, "%s: kind is not aligned to its element size", who);
  const int64_t need = gdm_des_batch_workspace_bytes(B, a.dim, a.max_queue_cap);
  if (need < 0 || workspace_bytes < (size_t)need || ((uintptr_t)a.workspace & 15)) {
    gdm_set_error("%s: workspace too small or not 16-byte aligned (%lld bytes needed)", who, (long long)need);
    return GDM_EWORKSPACE;
  }
  return GDM_OK;
}

// what every entry does: the checks, its policy's kernel, then the pack step (`dist_kind` is nullptr where the policy
// has none)
template <class Policy>
static int launch_batch(const char* who, const BatchArgs& a, int B, const int32_t* dist_kind, int64_t n_records_cap,
                        int64_t* rec_ptr, size_t workspace_bytes, void* stream) {
  const int rc = check_batch_args(who, a, B, dist_kind, Policy::kHasKind, n_records_cap, rec_ptr, workspace_bytes);
  if (rc != GDM_OK) return rc;
  hipLaunchKernelGGL(des_batch_kernel<Policy>, dim3(B), dim3(GDM_WAVE), des_wave::lds_dyn_bytes(a.dim),
                     (hipStream_t)stream, a.adj, a.dim, a.loc, a.scale, a.queue_cap, a.seed, a.number_of_customers,
                     a.max_queue_cap, a.max_events, a.max_records, a.mt_key, a.mt_pos, a.mt_has_gauss, a.mt_gauss,
                     a.value, a.event_id, a.node, a.kind, a.n_records, a.stop_reason, a.workspace, dist_kind);
  GDM_LAUNCH_OK(who);
  return gdm_des_pack(B, a.max_records, a.n_records, rec_ptr, a.value, a.event_id, a.node, a.kind, stream);
}

extern "C" int gdm_des_run_batch(const double* adj, int B, int dim, const double* loc, const double* scale,
                                 const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                                 int max_queue_cap, int64_t max_events, int64_t max_records, uint32_t* mt_key,
                                 int32_t* mt_pos, int32_t* mt_has_gauss, double* mt_gauss, double* value,
                                 int64_t* event_id, int32_t* node, int32_t* kind, int64_t n_records_cap,
                                 int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return launch_batch<des_wave::NormalOnly>("gdm_des_run_batch", DES_BATCH_ARGS, B, nullptr, n_records_cap, rec_ptr,
                                            workspace_bytes, stream);
}

extern "C" int gdm_des_run_batch_dist(const double* adj, int B, int dim, const double* loc, const double* scale,
                                      const int32_t* dist_kind, const int32_t* queue_cap, const int64_t* seed,
                                      const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                                      int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* mt_has_gauss,
                                      double* mt_gauss, double* value, int64_t* event_id, int32_t* node,
                                      int32_t* kind, int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records,
                                      int32_t* stop_reason, void* workspace, size_t workspace_bytes, void* stream) {
  return launch_batch<des_wave::AnyDist>("gdm_des_run_batch_dist", DES_BATCH_ARGS, B, dist_kind, n_records_cap, rec_ptr,
                                         workspace_bytes, stream);
}

extern "C" int gdm_des_run_batch_net(const double* adj, int B, int dim, const double* loc, const double* scale,
                                     const int32_t* node_kind, const int32_t* queue_cap, const int64_t* seed,
                                     const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                                     int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* mt_has_gauss,
                                     double* mt_gauss, double* value, int64_t* event_id, int32_t* node,
                                     int32_t* kind, int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records,
                                     int32_t* stop_reason, void* workspace, size_t workspace_bytes, void* stream) {
  return launch_batch<des_wave::AnyNode>("gdm_des_run_batch_net", DES_BATCH_ARGS, B, node_kind, n_records_cap, rec_ptr,
                                         workspace_bytes, stream);
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
