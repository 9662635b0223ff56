// The batched simulator of des_batch.hip WITHOUT a log: per-node queueing statistics of B samples, O(B * dim) out.
//
// The same event chain (des_sim.h) with the null record sink des::OutNone and the statistics policy des::NodeStats: the
// accumulators every Server / Source of the reference carries (SIMULATOR/simulation_v3.py:207-217, 280-281), from
// which Sim.calculate_metrics (752-824) derives utilisation, waiting times, renege rates and L / LQ / W / WQ.
//
// One kernel template over one body (stats_sample), instantiated for the three node policies of des_wave.h:
// des_stats_kernel<NormalOnly> draws 'normal' only (the bridges' nets); des_stats_kernel<AnyDist> takes a kind per node
// (normal, exponential, uniform), its row staged into LDS; des_stats_kernel<AnyNode> takes the reference's 'queue' and
// 'branch' nodes as well, with the two per-node arrays of that policy -- delayed departures, next departure time -- in
// LDS beside the kinds.  (Older texts call the three des_stats_kernel, des_stats_dist_kernel, des_stats_net_kernel.)
// One launcher template (launch_stats) is behind the three entries.
//
// Mapping as in des_batch.hip, one WAVE per sample (des_wave.h is the shared prologue): all lanes stage the parameters,
// build the routing tables and seed the node generators; lane 0 runs the chain; then ALL lanes write the (dim) rows
// with ordinary vector stores.  No record arrays, no pack step.
// LDS: the block of des_wave.h (16.2 KB) + eight 8-byte and one 4-byte accumulator per node (8.5 KB at the maximum of
// 128 nodes) + the node generators when dim <= 15 (36.6 KB): 61.3 KB, below the 64 KB a workgroup may have; the kinds
// of des_stats_kernel<AnyDist> add 512 B (61.8 KB), the kinds and node state of des_stats_kernel<AnyNode> 2 KB (63.3 KB:
// the static_assert below adds the blocks up).  Global memory holds what a sample cannot keep there: routing tables,
// the FIFO ring of customer ids and, slot for slot beside it, the ring of their arrival times (workspace), and the
// optional time-at-queue-length histogram (an output).
// Bounds: every index the chain computes is checked in des_sim.h before it forms an address -- the arrival-time ring
// is written and read at the slot the id ring was checked for, a histogram column is compared with its stride -- and
// every loop is bounded by max_events or the draw budget.
#include <climits>
#include "gdm_common.h"
#include "des_sim.h"
#include "des_wave.h"

#pragma clang fp contract(off)

namespace {

using des_wave::kMaxDim;

struct StatsLds {
  int64_t served[kMaxDim], reneges[kMaxDim], generated[kMaxDim];
  double time_in_service[kMaxDim], time_in_queue[kMaxDim], queue_area[kMaxDim], arrival_time[kMaxDim],
      last_change[kMaxDim];
  int32_t max_queue[kMaxDim];
  int reason;
};

static_assert(sizeof(des_wave::Lds) + sizeof(StatsLds) + des_wave::kMaxPolicyLds + 16 * 3 +
                      (size_t)des_wave::kLdsGenDim * DES_MT_N * 4 <= 64 * 1024,
              "des_stats_kernel<AnyNode>: static + dynamic LDS beyond a workgroup's 64 KB");

// the (B, dim) and (B) outputs of the kernels, and the inputs they share
struct StatsArgs {
  const double* adj;
  int dim;
  const double *loc, *scale;
  const int32_t* queue_cap;
  const int64_t *seed, *number_of_customers;
  int max_queue_cap;
  int64_t max_events;
  uint32_t* mt_key;
  int32_t *mt_pos, *mt_has_gauss;
  double* mt_gauss;
  int64_t *served, *reneges, *generated;
  int32_t* max_queue;
  double *time_in_service, *time_in_queue, *queue_area, *arrival_time, *clock, *end_time;
  int64_t *total_customers, *events, *n_records;
  int32_t* stop_reason;
  double* queue_time;
  unsigned char* workspace;
};

// One sample, every lane of its wave.  s.dist is the caller's (what it points to is staged before the call: the
// prologue's first barrier orders it before lane 0 reads it).
template <class SimT>
__device__ __forceinline__ void stats_sample(SimT& s, des_wave::Lds& lds, StatsLds& acc, unsigned char* s_dyn,
                                             const StatsArgs& a) {
  const int b = blockIdx.x, lane = threadIdx.x, dim = a.dim;
  const des_wave::WsLayout w = des_wave::ws_layout(dim, a.max_queue_cap, true);
  unsigned char* ws = a.workspace + (size_t)b * w.per_sample;
  const int64_t hist_stride = (int64_t)a.max_queue_cap + 1;
  double* hist = a.queue_time ? a.queue_time + (int64_t)b * dim * hist_stride : nullptr;

  s.out = des::OutNone{};
  s.out_cap = INT64_MAX;
  s.max_records = 0;
  s.stats.served = acc.served;
  s.stats.reneges = acc.reneges;
  s.stats.generated = acc.generated;
  s.stats.max_queue = acc.max_queue;
  s.stats.time_in_service = acc.time_in_service;
  s.stats.time_in_queue = acc.time_in_queue;
  s.stats.queue_area = acc.queue_area;
  s.stats.arrival_time = acc.arrival_time;
  s.stats.last_change = acc.last_change;
  s.stats.atime = reinterpret_cast<double*>(ws + w.atime);
  s.stats.queue_time = hist;
  s.stats.ring_stride = a.max_queue_cap;
  s.stats.hist_stride = hist_stride;
  // ---- all lanes: zero accumulators (and the sample's histogram), then the shared prologue (its barriers order them)
  s.stats.reset(dim, lane, GDM_WAVE);
  if (hist)
    for (int64_t i = lane; i < (int64_t)dim * hist_stride; i += GDM_WAVE) hist[i] = 0.0;
  const bool ok = des_wave::prologue(s, lds, s_dyn, ws, w, b, lane, a.adj, dim, a.loc, a.scale, a.queue_cap, a.seed,
                                     a.max_queue_cap, a.max_events, a.mt_key, a.mt_pos, a.mt_has_gauss, a.mt_gauss);
  // ---- lane 0: the chain
  if (lane == 0) {
    int reason = DES_STOP_ERROR;
    if (ok) reason = s.run(a.number_of_customers[b], a.max_events);
    const bool keep = reason != DES_STOP_ERROR;           // a sample that errors: zeros, its generator as it came
    if (keep) des_wave::store_generator_scalars(lds, dim, b, a.mt_pos, a.mt_has_gauss, a.mt_gauss);
    a.clock[b] = keep ? s.clock : 0.0;
    a.end_time[b] = keep ? s.stats.end_time : 0.0;
    a.total_customers[b] = keep ? s.total_customers : 0;
    a.events[b] = keep ? s.stats.events : 0;
    a.n_records[b] = keep ? s.n_out : 0;
    a.stop_reason[b] = reason;
    acc.reason = reason;
  }
  __syncthreads();
  // ---- all lanes: the rows
  const bool keep = acc.reason != DES_STOP_ERROR;
  for (int i = lane; i < dim; i += GDM_WAVE) {
    const int64_t o = (int64_t)b * dim + i;
    a.served[o] = keep ? acc.served[i] : 0;
    a.reneges[o] = keep ? acc.reneges[i] : 0;
    a.generated[o] = keep ? acc.generated[i] : 0;
    a.max_queue[o] = keep ? acc.max_queue[i] : 0;
    a.time_in_service[o] = keep ? acc.time_in_service[i] : 0.0;
    a.time_in_queue[o] = keep ? acc.time_in_queue[i] : 0.0;
    a.queue_area[o] = keep ? acc.queue_area[i] : 0.0;
    a.arrival_time[o] = keep ? acc.arrival_time[i] : 0.0;
  }
  if (keep) {
    des_wave::store_generator_words(lds, b, lane, a.mt_key);
  } else if (hist) {
    for (int64_t i = lane; i < (int64_t)dim * hist_stride; i += GDM_WAVE) hist[i] = 0.0;
  }
}

// The kernels' parameter list and the StatsArgs of it, under the names the entries below use too.  Kernel parameters
// stay plain __restrict__ pointers: with the struct as the parameter the compiler loses the no-alias facts and all
// three kernels come out longer.
#define DES_STATS_PARAMS                                                                                               \
  const double *__restrict__ adj, int dim, const double *__restrict__ loc, const double *__restrict__ scale,           \
      const int32_t *__restrict__ queue_cap, const int64_t *__restrict__ seed,                                         \
      const int64_t *__restrict__ number_of_customers, int max_queue_cap, int64_t max_events,                          \
      uint32_t *__restrict__ mt_key, int32_t *__restrict__ mt_pos, int32_t *__restrict__ mt_has_gauss,                 \
      double *__restrict__ mt_gauss, int64_t *__restrict__ served, int64_t *__restrict__ reneges,                      \
      int64_t *__restrict__ generated, int32_t *__restrict__ max_queue, double *__restrict__ time_in_service,          \
      double *__restrict__ time_in_queue, double *__restrict__ queue_area, double *__restrict__ arrival_time,          \
      double *__restrict__ clock, double *__restrict__ end_time, int64_t *__restrict__ total_customers,                \
      int64_t *__restrict__ events, int64_t *__restrict__ n_records, int32_t *__restrict__ stop_reason,                \
      double *__restrict__ queue_time, unsigned char *__restrict__ workspace
#define DES_STATS_ARGS                                                                                                 \
  StatsArgs {                                                                                                          \
    adj, dim, loc, scale, queue_cap, seed, number_of_customers, max_queue_cap, max_events, mt_key, mt_pos,             \
        mt_has_gauss, mt_gauss, served, reneges, generated, max_queue, time_in_service, time_in_queue, queue_area,     \
        arrival_time, clock, end_time, total_customers, events, n_records, stop_reason, queue_time,                    \
        (unsigned char*)workspace                                                                                      \
  }

// One kernel per node policy (des_wave.h) over that body.  flatten: three kinds at three draw sites exceed the inliner's
// budget, and a chain function left out of line takes the Sim by address -- 384 bytes of scratch per lane and a load
// for every member; inlined whole there is no scratch.  The policy's block is staged before the prologue, whose first
// barrier orders it before lane 0 reads it.  (With its kinds staged through AnyDist::stage and no longer in the kernel's
// own body, des_stats_kernel<AnyDist> is scheduled differently from the kernel it replaces: 86 VGPRs for 104, 114
// instructions more, and measured 0.7 to 1.5 % faster; DESIGN.md section 7, f19.  The other two are the same code.)
template <class Policy>
__global__ __launch_bounds__(GDM_WAVE) __attribute__((flatten)) void des_stats_kernel(
    DES_STATS_PARAMS, const int32_t* __restrict__ kind) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];       // node generators when dim <= kLdsGenDim
  __shared__ des_wave::Lds lds;
  __shared__ StatsLds acc;
  __shared__ typename Policy::Block pl;
  des::Sim<des::MathPortable, des::OutNone, des::NodeStats, typename Policy::Dist> s;
  Policy::stage(s.dist, pl, kind, dim, blockIdx.x, threadIdx.x);
  stats_sample(s, lds, acc, s_dyn, DES_STATS_ARGS);
}

// the checks the device entries make on the host; `who` names the entry in the message
int check_stats_args(const char* who, const StatsArgs& a, int B, const int32_t* kind, bool with_kind,
                     size_t workspace_bytes) {
  GDM_REQUIRE(a.adj && a.loc && a.scale && a.queue_cap && a.seed && a.number_of_customers && a.mt_key && a.mt_pos &&
                  a.mt_has_gauss && a.mt_gauss && a.served && a.reneges && a.generated && a.max_queue &&
                  a.time_in_service && a.time_in_queue && a.queue_area && a.arrival_time && a.clock && a.end_time &&
                  a.total_customers && a.events && a.n_records && a.stop_reason && a.workspace && (kind || !with_kind),
              "%s: null pointer", who);
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && a.dim >= 1 && a.dim <= kMaxDim && a.max_queue_cap >= 1 &&
                  a.max_queue_cap <= GDM_DES_BATCH_MAX_QUEUE_CAP,
              "%s: 1 <= B <= 2^20, 1 <= dim <= %d, 1 <= max_queue_cap <= %d", who, kMaxDim, GDM_DES_BATCH_MAX_QUEUE_CAP);
  GDM_REQUIRE(a.max_events >= 1 && a.max_events <= GDM_DES_BATCH_MAX_EVENTS, "%s: max_events must be in 1..%lld", who,
              (long long)GDM_DES_BATCH_MAX_EVENTS);
  const uintptr_t a8 = (uintptr_t)a.adj | (uintptr_t)a.loc | (uintptr_t)a.scale | (uintptr_t)a.seed |
                       (uintptr_t)a.number_of_customers | (uintptr_t)a.mt_gauss | (uintptr_t)a.served |
                       (uintptr_t)a.reneges | (uintptr_t)a.generated | (uintptr_t)a.time_in_service |
                       (uintptr_t)a.time_in_queue | (uintptr_t)a.queue_area | (uintptr_t)a.arrival_time |
                       (uintptr_t)a.clock | (uintptr_t)a.end_time | (uintptr_t)a.total_customers |
                       (uintptr_t)a.events | (uintptr_t)a.n_records | (uintptr_t)a.queue_time;
  const uintptr_t a4 = (uintptr_t)a.queue_cap | (uintptr_t)a.mt_key | (uintptr_t)a.mt_pos | (uintptr_t)a.mt_has_gauss |
                       (uintptr_t)a.max_queue | (uintptr_t)a.stop_reason | (uintptr_t)kind;
  GDM_REQUIRE((a8 & 7) == 0 && (a4 & 3) == 0, "%s: an array is not aligned to its element size", who);
  const int64_t need = gdm_des_stats_workspace_bytes(B, a.dim, a.max_queue_cap);
  GDM_REQUIRE(need >= 0 && workspace_bytes >= (size_t)need && ((uintptr_t)a.workspace & 15) == 0,
              "%s: workspace too small or not 16-byte aligned (%lld bytes needed)", who, (long long)need);
  return GDM_OK;
}

// what every entry does: the checks, then its policy's kernel (`kind` is nullptr where the policy has none)
template <class Policy>
int launch_stats(const char* who, const StatsArgs& a, int B, const int32_t* kind, size_t workspace_bytes,
                 void* stream) {
  const int rc = check_stats_args(who, a, B, kind, Policy::kHasKind, workspace_bytes);
  if (rc != GDM_OK) return rc;
  hipLaunchKernelGGL(des_stats_kernel<Policy>, dim3(B), dim3(GDM_WAVE), des_wave::lds_dyn_bytes(a.dim),
                     (hipStream_t)stream, a.adj, a.dim, a.loc, a.scale, a.queue_cap, a.seed, a.number_of_customers,
                     a.max_queue_cap, a.max_events, a.mt_key, a.mt_pos, a.mt_has_gauss, a.mt_gauss, a.served, a.reneges,
                     a.generated, a.max_queue, a.time_in_service, a.time_in_queue, a.queue_area, a.arrival_time,
                     a.clock, a.end_time, a.total_customers, a.events, a.n_records, a.stop_reason, a.queue_time,
                     a.workspace, kind);
  GDM_LAUNCH_OK(who);
  return GDM_OK;
}

}  // namespace

extern "C" int64_t gdm_des_stats_workspace_bytes(int B, int dim, int max_queue_cap) {
  if (B < 1 || B > (1 << 20) || dim < 1 || dim > kMaxDim || max_queue_cap < 1 ||
      max_queue_cap > GDM_DES_BATCH_MAX_QUEUE_CAP)
    return -1;
  return (int64_t)(des_wave::ws_layout(dim, max_queue_cap, true).per_sample * (size_t)B);
}

extern "C" int gdm_des_stats_batch(const double* adj, int B, int dim, const double* loc, const double* scale,
                                   const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                                   int max_queue_cap, int64_t max_events, uint32_t* mt_key, int32_t* mt_pos,
                                   int32_t* mt_has_gauss, double* mt_gauss, int64_t* served, int64_t* reneges,
                                   int64_t* generated, int32_t* max_queue, double* time_in_service,
                                   double* time_in_queue, double* queue_area, double* arrival_time, double* clock,
                                   double* end_time, int64_t* total_customers, int64_t* events, int64_t* n_records,
                                   int32_t* stop_reason, double* queue_time, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  return launch_stats<des_wave::NormalOnly>("gdm_des_stats_batch", DES_STATS_ARGS, B, nullptr, workspace_bytes, stream);
}

extern "C" int gdm_des_stats_batch_dist(const double* adj, int B, int dim, const double* loc, const double* scale,
                                        const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                                        const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                                        uint32_t* mt_key, int32_t* mt_pos, int32_t* mt_has_gauss, double* mt_gauss,
                                        int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                                        double* time_in_service, double* time_in_queue, double* queue_area,
                                        double* arrival_time, double* clock, double* end_time,
                                        int64_t* total_customers, int64_t* events, int64_t* n_records,
                                        int32_t* stop_reason, double* queue_time, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return launch_stats<des_wave::AnyDist>("gdm_des_stats_batch_dist", DES_STATS_ARGS, B, kind, workspace_bytes, stream);
}

extern "C" int gdm_des_stats_batch_net(const double* adj, int B, int dim, const double* loc, const double* scale,
                                       const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                                       const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                                       uint32_t* mt_key, int32_t* mt_pos, int32_t* mt_has_gauss, double* mt_gauss,
                                       int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                                       double* time_in_service, double* time_in_queue, double* queue_area,
                                       double* arrival_time, double* clock, double* end_time,
                                       int64_t* total_customers, int64_t* events, int64_t* n_records,
                                       int32_t* stop_reason, double* queue_time, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return launch_stats<des_wave::AnyNode>("gdm_des_stats_batch_net", DES_STATS_ARGS, B, kind, workspace_bytes, stream);
}
