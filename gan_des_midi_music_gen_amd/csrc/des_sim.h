// The event logic of the queueing-network discrete-event simulator (SIMULATOR/simulation_v3.py: Sim.run 426-516,
// Initialization 518-534, ProcessArrival 536-588, ScheduleDeparture 591-612, ProcessDeparture 615-677, get_destination
// 699-743, FlowBranchOperator 25-74), ONE source for the host core (gdm_des_run, des_core.hip), the host batch mirror
// (gdm_des_run_batch_host) and the device kernel (des_batch.hip).  Compiles as host code, as gfx950 device code and as
// plain C++ without any HIP include.
//
// What is reproduced bit for bit (tests/golden/des_core.npz pins it through gdm_des_run):
//   * numpy's legacy MT19937 RandomState: per-node generators seeded from RandomState(seed).randint(3, 9999999), and the
//     GLOBAL np.random stream FlowBranchOperator.randomly_select_child draws from (simulation_v3.py:57,62),
//   * scipy.stats.norm(loc, scale).rvs(random_state=rng) = rng.standard_normal() * scale + loc (legacy polar gauss),
//   * Python's heapq order for simultaneous events (Event.__lt__ compares times only).
//
// Storage is the caller's, with capacities that follow from the spec (nothing grows):
//   event list   at most one pending arrival per source and one departure per server: dim entries (+1)
//   FIFO rings   ring_stride customer ids per server; admission keeps a queue below queue_cap[node], so a stride of
//                max(queue_cap) is never exceeded (only the id of a queued event is ever read back)
//   routing      children / cdf per node, dim entries each, computed once with the operations (and their order) of
//                FlowBranchOperator.__init__ and numpy's legacy choice(p=...)
//   generators   dim node states + the global one + the seeder, 624 words each
// Every capacity is checked where it is used and every index that was computed from data is checked before it forms an
// address; an overrun ends the sample with DES_STOP_ERROR.
//
// Every loop is bounded: each 32-bit generator draw counts against `draws_left`.  The batch entries set it to
// DES_DRAW_FACTOR * (max_events + dim + 1): a healthy event makes at most one service draw, one inter-arrival draw and
// one routing draw, about 10 words on average (a polar pair costs 4 words per attempt, accepted with p = pi/4), so 64
// per event is out of reach of a healthy run and stops `while service <= 0` for loc << 0 after a bounded time
// (DES_STOP_BUDGET).  gdm_des_run passes INT64_MAX: today's behaviour.
//
// What a run leaves behind is two more policies.  Out is the record sink: the 'Music' log as an array of structs, as four
// field arrays, or nothing at all (OutNone).  Stats is the accumulator set: NoStats (empty, every hook a no-op: the logging
// builds) or NodeStats, the per-node queueing statistics of the reference's Server / Source objects, or SnapStats,
// NodeStats with snapshots of them at customer counts of the same run.
//
// Dist is the distribution policy: NormalOnly (empty: every draw is norm_rvs, the bridges' nets) or AnyDist, a kind per
// node -- normal, exponential or uniform -- or AnyNode, which adds the reference's two node kinds without a distribution:
// 'queue' (a waiting room whose departures wait for an idle child) and 'branch' (a zero-time router).
//
// Math is a policy (template parameter): log / sqrt of the polar method.  DesMathPortable is plain double arithmetic
// (+ - * / and bit manipulation, contraction off, no FMA) and gives the same bits on the host and on gfx950; the host
// core of gdm_des_run uses libm's (what numpy calls), which no portable implementation can match bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define DES_HD __host__ __device__
#else
#define DES_HD
#endif
// a policy's hooks are part of the function that calls them, whatever the inliner's budget says: a NormalOnly build is
// the code it was before there were distribution policies, and an AnyDist build keeps its Sim in registers
#define DES_HOOK DES_HD inline __attribute__((always_inline))

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define DES_STOP_EMPTY 0      /* event list empty */
#define DES_STOP_CUSTOMERS 1  /* number_of_customers reached */
#define DES_STOP_EVENTS 2     /* max_events processed */
#define DES_STOP_ERROR 3      /* bad spec, no destination, customer routed to a source, capacity overrun */
#define DES_STOP_RECORDS 4    /* max_records written */
#define DES_STOP_BUDGET 5     /* draw budget exhausted */
#define DES_DRAW_FACTOR 64
#define DES_MT_N 624

namespace des {

DES_HD inline uint64_t bits_of(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
DES_HD inline double double_of(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

// Natural logarithm in the form of fdlibm's e_log.c (argument reduction x = 2^k (1 + f), sqrt(1/2) < 1 + f < sqrt(2);
// log(1 + f) = 2s + s R(s^2), s = f / (2 + f), R a degree-14 minimax polynomial; below 1 ulp).  Only + - * / on
// doubles and integer work on the bit pattern: with contraction off every operation is one IEEE operation.
DES_HD inline double des_log(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16,
               Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  uint64_t u = bits_of(x);
  int32_t hx = (int32_t)(u >> 32);
  const uint32_t lx = (uint32_t)u;
  int32_t k = 0;
  if (hx < 0x00100000) {                                              // x < 2^-1022
    if (((hx & 0x7fffffff) | lx) == 0) return double_of(0xfff0000000000000ULL);      // log(+-0) = -inf
    if (hx < 0) return double_of(0x7ff8000000000000ULL);                             // log(-#) = NaN
    k -= 54;
    x *= two54;
    u = bits_of(x);
    hx = (int32_t)(u >> 32);
  }
  if (hx >= 0x7ff00000) return x + x;
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int32_t i0 = (hx + 0x95f64) & 0x100000;
  u = (u & 0xffffffffULL) | ((uint64_t)(uint32_t)(hx | (i0 ^ 0x3ff00000)) << 32);     // normalise x or x / 2
  x = double_of(u);
  k += i0 >> 20;
  const double f = x - 1.0;
  const double dk = (double)k;
  if ((0x000fffff & (2 + hx)) < 3) {                                  // |f| < 2^-20
    if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  int32_t i = hx - 0x6147a;
  const double w = z * z;
  const int32_t j = 0x6b851 - hx;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  i |= j;
  const double R = t2 + t1;
  if (i > 0) {
    const double hfsq = 0.5 * f * f;
    return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// The portable policy.  sqrt is the compiler's IEEE square root: one correctly rounded instruction on x86-64 and the
// correctly rounded expansion of llvm.sqrt.f64 on gfx950 (tests/test_des_batch_gpu.py compares the two bit for bit).
struct MathPortable {
  DES_HD static double log(double x) { return des_log(x); }
  DES_HD static double sqrt(double x) { return __builtin_sqrt(x); }
};

// ---- routing table of one node (FlowBranchOperator.__init__, simulation_v3.py:25-74, and the cdf numpy's legacy
// choice(children, p=...) builds on every call: p.cumsum(); cdf /= cdf[-1]) ----------------------------------------------
#define DES_BRANCH_UNIFORM 1  /* sum(probabilities) != 1 -> np.random.choice(children) without p (56-58) */
#define DES_BRANCH_SINK 2     /* sum(children) == 0 (73): also true when the only destination is node 0 */
DES_HD inline void make_branch(const double* row, int dim, int self, int32_t* children, double* cdf, int32_t* n_out,
                               uint8_t* flags_out) {
  int n = 0;
  for (int j = 0; j < dim; ++j) {
    const double pj = (j == self) ? 0.0 : row[j];
    if (pj > 0) {                                      // children / probabilities with non-zero probability (38-40)
      children[n] = j;
      cdf[n] = pj;
      ++n;
    }
  }
  double s = 0.0;                                      // Python sum(): left to right, starting from int 0
  for (int i = 0; i < n; ++i) s += cdf[i];
  for (int i = 0; i < n; ++i) cdf[i] = cdf[i] / s;     // line 47 (sum() of the un-normalised list every time)
  double s1 = 0.0;
  for (int i = 0; i < n; ++i) s1 += cdf[i];
  long cs = 0;
  for (int i = 0; i < n; ++i) cs += children[i];
  double acc = 0.0;                                    // cumsum
  for (int i = 0; i < n; ++i) {
    acc += cdf[i];
    cdf[i] = acc;
  }
  if (n > 0) {
    const double last = cdf[n - 1];
    for (int i = 0; i < n; ++i) cdf[i] /= last;
  }
  *n_out = n;
  *flags_out = (uint8_t)((s1 != 1.0 ? DES_BRANCH_UNIFORM : 0) | (cs == 0 ? DES_BRANCH_SINK : 0));
}

// init_genrand of mt19937_seed: the 624 words of RandomState(s); position 624, no cached gauss
DES_HD inline void seed_key(uint32_t* key, uint32_t s) {
  for (int i = 0; i < DES_MT_N; ++i) {
    key[i] = s;
    s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)(i + 1);
  }
}

struct Ev {
  double time;
  int64_t id;
  int32_t type;            // 1 arrival, 2 departure
  int32_t server;
  int32_t source;          // -1 = None
  int32_t pad;
};

// Record sinks: array of gdm_des_event-shaped structs (gdm_des_run) or the four field arrays of the CSR layout
struct OutAos {
  struct Rec {
    double value;
    int64_t event_id;
    int32_t node;
    int32_t kind;
  };
  Rec* out;
  DES_HD void put(int64_t i, double v, int64_t id, int node, int kind) const { out[i] = Rec{v, id, node, kind}; }
};
struct OutSoa {
  double* value;
  int64_t* event_id;
  int32_t* node;
  int32_t* kind;
  DES_HD void put(int64_t i, double v, int64_t id, int nd, int kd) const {
    value[i] = v;
    event_id[i] = id;
    node[i] = (int32_t)nd;
    kind[i] = (int32_t)kd;
  }
};

// No records at all (the statistics mode): Sim::n_out keeps counting, so the number of records the run would have
// written is a free statistic.
struct OutNone {
  DES_HD void put(int64_t, double, int64_t, int, int) const {}
};

// ---- statistics policies: the accumulators every Server / Source of the reference carries (simulation_v3.py:207-217,
// 280-281), driven by hooks at the reference's own lines.  NoStats is empty, every hook a no-op: the logging builds.
struct NoStats {
  DES_HD void pop(double) const {}
  DES_HD void event() const {}
  DES_HD void service(int, double) const {}
  DES_HD void renege(int) const {}
  DES_HD void generate(int, double) const {}
  DES_HD void enqueue(int, int64_t, double, int64_t, int64_t) const {}
  DES_HD void dequeue(int, int64_t, double, int64_t) const {}
  DES_HD void held(int, double, int64_t) const {}
  DES_HD void delay(int, double) const {}
  template <class D>
  DES_HD void checkpoint(int64_t, double, const int32_t*, const D&, int64_t, int64_t) const {}
  template <class D>
  DES_HD void finish(const uint8_t*, const int32_t*, int, const D&) const {}
};

// Storage is the caller's: (dim) per array, atime (dim, ring_stride) beside the id ring and indexed like it, queue_time
// (dim, hist_stride) or null.  served .. arrival_time are accumulated in the reference's order and can match it bit
// for bit.  Time at queue length is NOT summed per popped event over all servers as the reference does (472-484, an
// O(dim) loop): a server's share is added when its queue length changes and once at the end, (t - last_change) at a
// time, t = the time of the last popped event -- the same sum in exact arithmetic, rounded differently.
struct NodeStats {
  int64_t* served;            // total_customers_served (596)
  int64_t* reneges;           // 564
  int64_t* generated;         // customers_generated (530, 579)
  int32_t* max_queue;         // max_queue_length (560-561)
  double* time_in_service;    // total_time_in_service (606)
  double* time_in_queue;      // total_time_in_queue (641)
  double* queue_area;         // sum over k of k * queue_length_times[k]
  double* arrival_time;       // Source.arrival_times (526, 578)
  double* last_change;        // scratch: when the node's queue length last changed
  double* atime;              // (dim, ring_stride): Event.arrival_time of the queued customers (558)
  double* queue_time;         // (dim, hist_stride): queue_length_times, dense; null = not wanted
  int64_t ring_stride, hist_stride;
  double end_time;            // the reference's previous_time: the time of the last popped event
  int64_t events;             // processed events

  DES_HD void reset(int dim, int first, int step) {
    for (int i = first; i < dim; i += step) {
      served[i] = reneges[i] = generated[i] = 0;
      max_queue[i] = 0;
      time_in_service[i] = time_in_queue[i] = queue_area[i] = arrival_time[i] = last_change[i] = 0.0;
    }
    end_time = 0.0;
    events = 0;
  }
  DES_HD void pop(double t) { end_time = t; }
  DES_HD void event() { ++events; }
  DES_HD void service(int node, double s) {
    ++served[node];
    time_in_service[node] += s;
  }
  DES_HD void renege(int node) { ++reneges[node]; }
  DES_HD void generate(int source, double dt) {
    arrival_time[source] += dt;
    ++generated[source];
  }
  DES_HD void integrate(int node, double t, int64_t len) {
    const double d = t - last_change[node];
    queue_area[node] += d * (double)len;
    if (queue_time && len >= 0 && len < hist_stride) queue_time[(int64_t)node * hist_stride + len] += d;
    last_change[node] = t;
  }
  // slot: the ring slot Sim checked and used for the customer's id; len: the queue length before the change; held: the
  // node's delayed departures (AnyNode; else 0), which count in the time at queue length (477) but not in max_queue (560)
  DES_HD void enqueue(int node, int64_t slot, double t, int64_t len, int64_t held) {
    atime[(int64_t)node * ring_stride + slot] = t;
    integrate(node, t, len + held);
    if (len + 1 > (int64_t)max_queue[node]) max_queue[node] = (int32_t)(len + 1);
  }
  DES_HD void dequeue(int node, int64_t slot, double t, int64_t len) {
    time_in_queue[node] += t - atime[(int64_t)node * ring_stride + slot];
    integrate(node, t, len);
  }
  // the number of delayed departures of a node is about to change; len: queue length + delayed departures before it
  DES_HD void held(int node, double t, int64_t len) { integrate(node, t, len); }
  DES_HD void delay(int node, double dt) { time_in_queue[node] += dt; }                // 697
  // after every pop, before the customers test: SnapStats' (below); nothing here
  template <class D>
  DES_HD void checkpoint(int64_t, double, const int32_t*, const D&, int64_t, int64_t) const {}
  template <class D>
  DES_HD void finish(const uint8_t* is_source, const int32_t* qlen, int dim, const D& dist) {
    for (int i = 0; i < dim; ++i)
      if (!is_source[i]) integrate(i, end_time, qlen[i] + dist.held(i));
  }
};

// ---- NodeStats with snapshots at customer counts.  number_of_customers enters the run in its stop test alone, so the
// run of n1 customers is a prefix of the run of n2 > n1: the state at the pop where the test for n1 WOULD fire, closed
// the way finish() closes it, is what the run of n1 customers returns -- field for field and bit for bit.
// snap_customers: the sample's n_snap checkpoints, strictly ascending, the last one the run's number_of_customers (the
// caller checks the row, sets next = 0 and passes the last entry to run()).  The accumulators of NodeStats are scratch here; `o` are the sample's
// snapshot rows, (n_snap, dim), (n_snap) and (n_snap, dim, hist_stride).  The RUNNING histogram (NodeStats::queue_time)
// is the last snapshot's slot: the last checkpoint is the run's own stop test, so that snapshot is the final state and
// finish() closes it in place.
// A snapshot's time-at-queue-length terms are closed on a COPY: queue_area, queue_time and last_change keep running
// untouched (an interval split in two rounds differently from then on, and the run would no longer be the run without
// snapshots).  With a histogram one snapshot costs the thread that runs the chain dim * hist_stride doubles.
// Host instantiations only so far (des_core.hip: gdm_des_stats_batch_snap_host; tools/des_snap_host.cpp): a
// one-wave-per-sample kernel over this policy is not part of the library.
struct SnapOut {
  int64_t *served, *reneges, *generated;
  int32_t* max_queue;
  double *time_in_service, *time_in_queue, *queue_area, *arrival_time, *clock, *end_time;
  int64_t *total_customers, *events, *n_records;
  int32_t* stop;
  double* queue_time;
};
struct SnapStats : NodeStats {
  const int64_t* snap_customers;
  int32_t n_snap, next;       // next: the first checkpoint not written yet (the caller sets it to 0)
  int32_t dim;
  const uint8_t* is_source;
  SnapOut o;

  // snapshot s: the state at this pop, its time at queue length closed up to end_time on a copy
  template <class D>
  DES_HD void write(int s, int64_t total_customers, double clock, const int32_t* qlen, const D& dist, int64_t n_out,
                    int64_t processed) {
    if (s < 0 || s >= n_snap) return;
    const int64_t row = (int64_t)s * dim, hs = hist_stride;
    double* h = queue_time ? o.queue_time + row * hs : nullptr;
    for (int i = 0; i < dim; ++i) {
      o.served[row + i] = served[i];
      o.reneges[row + i] = reneges[i];
      o.generated[row + i] = generated[i];
      o.max_queue[row + i] = max_queue[i];
      o.time_in_service[row + i] = time_in_service[i];
      o.time_in_queue[row + i] = time_in_queue[i];
      o.arrival_time[row + i] = arrival_time[i];
      double area = queue_area[i];
      if (h)
        for (int64_t k = 0; k < hs; ++k) h[i * hs + k] = queue_time[i * hs + k];
      if (!is_source[i]) {                                 // finish()'s integrate(), on the copy
        const int64_t len = qlen[i] + dist.held(i);
        const double d = end_time - last_change[i];
        area += d * (double)len;
        if (h && len >= 0 && len < hs) h[i * hs + len] += d;
      }
      o.queue_area[row + i] = area;
    }
    o.clock[s] = clock;
    o.end_time[s] = end_time;
    o.total_customers[s] = total_customers;
    o.events[s] = processed;
    o.n_records[s] = n_out;
    o.stop[s] = DES_STOP_CUSTOMERS;
  }
  // every checkpoint but the last whose stop test fires at this pop (several may: all at or below the number of
  // sources fire at the first); the last one is run()'s own test
  template <class D>
  DES_HD void checkpoint(int64_t total_customers, double clock, const int32_t* qlen, const D& dist, int64_t n_out,
                         int64_t processed) {
    while (next < n_snap - 1 && total_customers > snap_customers[next] - 1) {
      write(next, total_customers, clock, qlen, dist, n_out, processed);
      ++next;
    }
  }
  // After run(): every checkpoint not written yet receives the final state and the run's stop reason -- zeros after
  // an error (the checkpoints written before it are the shorter runs', which ended well).
  DES_HD void flush(int reason, int64_t total_customers, double clock, int64_t n_out) {
    const bool keep = reason != DES_STOP_ERROR;
    const int64_t hs = hist_stride;
    for (int s = next; s < n_snap; ++s) {
      const int64_t row = (int64_t)s * dim;
      for (int i = 0; i < dim; ++i) {
        o.served[row + i] = keep ? served[i] : 0;
        o.reneges[row + i] = keep ? reneges[i] : 0;
        o.generated[row + i] = keep ? generated[i] : 0;
        o.max_queue[row + i] = keep ? max_queue[i] : 0;
        o.time_in_service[row + i] = keep ? time_in_service[i] : 0.0;
        o.time_in_queue[row + i] = keep ? time_in_queue[i] : 0.0;
        o.queue_area[row + i] = keep ? queue_area[i] : 0.0;
        o.arrival_time[row + i] = keep ? arrival_time[i] : 0.0;
        if (!queue_time || (keep && s == n_snap - 1)) continue;           // (the running histogram is the last slot)
        double* h = o.queue_time + (row + i) * hs;
        for (int64_t k = 0; k < hs; ++k) h[k] = keep ? queue_time[i * hs + k] : 0.0;
      }
      o.clock[s] = keep ? clock : 0.0;
      o.end_time[s] = keep ? end_time : 0.0;
      o.total_customers[s] = keep ? total_customers : 0;
      o.events[s] = keep ? events : 0;
      o.n_records[s] = keep ? n_out : 0;
      o.stop[s] = reason;
    }
    next = n_snap;
  }
};

// ---- distribution policies: what a node's service / inter-arrival time is drawn from.  NormalOnly is empty and makes
// the three draw sites today's norm_rvs (the logging builds, the bridges' nets).  AnyDist carries one kind per node and
// adds the two kinds of the reference's Server / Source (simulation_v3.py:181-192, 263-274) that are ONE uniform double
// on the node's legacy stream, in scipy's own order of operations (`vals * scale + loc`, rv_continuous.rvs):
//   kind 1 'exponential'  stats.expon(scale=s).rvs(random_state=rng)      = (-log(1.0 - rng.random_sample())) * s + 0.0
//   kind 2 'uniform'      stats.uniform(loc, s).rvs(random_state=rng)     = rng.random_sample() * s + loc
// scale == 0 returns loc (0.0 for the exponential, whatever loc[] holds) and draws nothing, as scipy does.
#define DES_DIST_NORMAL 0
#define DES_DIST_EXPONENTIAL 1
#define DES_DIST_UNIFORM 2
// What a policy without node kinds answers at the sites where AnyNode (below) acts: nothing is held back, every server
// draws its service time, no departure waits.  Constants and empty bodies: the code is what it was without them.
struct PlainNodes {
  DES_HOOK bool timeless(int) const { return false; }
  DES_HOOK bool waits(int) const { return false; }
  DES_HOOK int64_t held(int) const { return 0; }
  DES_HOOK void scheduled(int, double) const {}
  DES_HOOK void idle(int) const {}
  template <class S>
  DES_HOOK void popped(S&, int, int) const {}
  // a departure with nowhere to go: queue-type nodes (delayed departures) are AnyNode's
  template <class S>
  DES_HOOK void delay(S& s, int, int64_t) const { s.fail(); }
};
struct NormalOnly : PlainNodes {
  template <class S>
  DES_HOOK double rvs(S& s, int node) const { return s.norm_rvs(node); }
  // with scale == 0 the node's value is 0.0 whatever loc[] holds (schedule_departure: `while (service <= 0)`)
  DES_HOOK bool ignores_loc(int) const { return false; }
  DES_HOOK bool kinds_ok(int) const { return true; }
};
struct AnyDist : PlainNodes {
  const int32_t* kind;        // (dim) DES_DIST_*
  template <class S>
  DES_HOOK double rvs(S& s, int node) const {
    const int32_t k = kind[node];
    if (k == DES_DIST_NORMAL) return s.norm_rvs(node);
    if (s.scale[node] == 0.0) return k == DES_DIST_EXPONENTIAL ? 0.0 : s.loc[node];
    const double u = s.next_double(node);                 // both are one uniform double
    if (k == DES_DIST_EXPONENTIAL) return (-S::math::log(1.0 - u)) * s.scale[node] + 0.0;
    return u * s.scale[node] + s.loc[node];
  }
  DES_HOOK bool ignores_loc(int node) const { return kind[node] == DES_DIST_EXPONENTIAL; }
  DES_HOOK bool kinds_ok(int dim) const {
    for (int i = 0; i < dim; ++i)
      if (kind[i] < DES_DIST_NORMAL || kind[i] > DES_DIST_UNIFORM) return false;
    return true;
  }
};

// ---- the node policy with the reference's two kinds WITHOUT a distribution (Server.__init__, 193-197) beside AnyDist's:
//   kind 3 'queue'   a waiting room in front of its children.  Service time 0, no draw.  Its departure takes no routing
//                    draw (get_destination returns None, 707): the first idle child that is a server is taken (628-633);
//                    if there is none and the node is no sink, the departure is scheduled again at the earliest next
//                    departure among the children (656-673, schedule_delayed_departure 679-697) -- exactly another
//                    event's time, so Python's heapq order decides; a delayed event that pops first is delayed again
//   kind 4 'branch'  a router: service time 0, no draw, routed like any server on the global stream
// Both are servers with in_service, a FIFO and a capacity.  `delayed` is the reference's Server.delayed_departures (0 or
// 1: the event list holds one departure per server), `next_departure` its EventList.servers_next_departure: +inf until
// the node first schedules a departure (sources never do), 0 once it goes idle.  Admission and the time at queue length
// count queue + delayed (557, 477).  As a SOURCE either kind raises upstream (Source.__init__: "Distribution not
// supported") and ends the sample here; so does a delayed time of +inf (every child a source: the run is not defined by
// the inputs alone).  Kinds 0..2 draw through AnyDist's own code.
#define DES_DIST_QUEUE 3
#define DES_DIST_BRANCH 4
struct AnyNode {
  const int32_t* kind;        // (dim) DES_DIST_*
  int32_t* delayed;           // (dim)
  double* next_departure;     // (dim)
  DES_HD void reset(int dim, int first, int step) const {
    for (int i = first; i < dim; i += step) {
      delayed[i] = 0;
      next_departure[i] = double_of(0x7ff0000000000000ULL);
    }
  }
  template <class S>
  DES_HOOK double rvs(S& s, int node) const {
    if (kind[node] >= DES_DIST_QUEUE) {                     // only a source gets here (timeless)
      s.fail();
      return 0.0;
    }
    return AnyDist{{}, kind}.rvs(s, node);
  }
  DES_HOOK bool ignores_loc(int node) const { return kind[node] == DES_DIST_EXPONENTIAL; }
  DES_HOOK bool kinds_ok(int dim) const {
    for (int i = 0; i < dim; ++i)
      if (kind[i] < DES_DIST_NORMAL || kind[i] > DES_DIST_BRANCH) return false;
    return true;
  }
  DES_HOOK bool timeless(int node) const { return kind[node] >= DES_DIST_QUEUE; }
  DES_HOOK bool waits(int node) const { return kind[node] == DES_DIST_QUEUE; }
  DES_HOOK int64_t held(int node) const { return delayed[node]; }
  DES_HOOK void scheduled(int node, double t) const { next_departure[node] = t; }       // 609
  DES_HOOK void idle(int node) const { next_departure[node] = 0.0; }                    // 648
  template <class S>
  DES_HOOK void popped(S& s, int node, int was_delayed) const {                         // 622-624
    if (!was_delayed) return;
    s.stats.held(node, s.clock, (int64_t)s.qlen[node] + delayed[node]);
    --delayed[node];
  }
  template <class S>
  DES_HOOK void delay(S& s, int node, int64_t id) const {                               // 656-673, 679-697
    double t = double_of(0x7ff0000000000000ULL);
    const int32_t* ch = s.children + (int64_t)node * s.dim;
    const int n = s.nchild[node] < s.dim ? s.nchild[node] : s.dim;
    for (int k = 0; k < n; ++k) {
      const int c = ch[k];
      if (c < 0 || c >= s.dim || c == node) continue;
      if (next_departure[c] < t) t = next_departure[c];
    }
    if (!(t < double_of(0x7ff0000000000000ULL))) { s.fail(); return; }
    s.in_service[node] = 1;
    s.stats.held(node, s.clock, (int64_t)s.qlen[node] + delayed[node]);
    ++delayed[node];
    s.push(Ev{t, id, 2, node, -1, 1});
    next_departure[node] = t;
    s.stats.delay(node, t - s.clock);
  }
};

template <class Math, class Out, class Stats = NoStats, class Dist = NormalOnly>
struct Sim {
  typedef Math math;
  // ---- storage, set by the caller ----
  int dim;
  const double* loc;          // (dim)
  const double* scale;        // (dim)
  const int32_t* qcap;        // (dim)
  uint8_t* is_source;         // (dim)
  int32_t* in_service;        // (dim)
  int32_t* qhead;             // (dim)
  int32_t* qlen;              // (dim)
  int32_t* nchild;            // (dim)
  uint8_t* bflags;            // (dim)
  int32_t* children;          // (dim, dim)
  double* cdf;                // (dim, dim)
  int64_t* ring;              // (dim, ring_stride)
  int64_t ring_stride;
  uint32_t* node_keys;        // (dim, 624)
  uint32_t* global_key;       // (624)
  uint32_t* seeder_key;       // (624)
  int32_t* pos;               // (dim + 2): nodes, global (index dim), seeder (dim + 1)
  int32_t* has_gauss;         // (dim + 2)
  double* gauss;              // (dim + 2)
  Ev* heap;
  int heap_cap;
  Out out;
  Stats stats;
  Dist dist;
  int64_t out_cap;
  int64_t max_records;        // 0 = no cap
  int64_t draws_left;
  // ---- run state ----
  int heap_n;
  int64_t n_out;
  double clock;
  int64_t total_customers;
  int stop;                   // 0 while running, else a DES_STOP_* code that ends the sample
  bool overflow;              // records were dropped beyond out_cap (n_out keeps counting)

  DES_HD void reset() {
    heap_n = 0;
    n_out = 0;
    clock = 0.0;
    total_customers = 0;
    stop = 0;
    overflow = false;
  }
  DES_HD void fail() {
    if (!stop) stop = DES_STOP_ERROR;
  }
  DES_HD uint32_t* key_of(int g) const {
    return g < dim ? node_keys + (int64_t)g * DES_MT_N : (g == dim ? global_key : seeder_key);
  }

  // ---- numpy.random.RandomState (legacy) ----
  DES_HD static void twist(uint32_t* key) {
    const uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MAT = 0x9908b0dfu;
    int i;
    uint32_t y;
    for (i = 0; i < 624 - 397; ++i) {
      y = (key[i] & UPPER) | (key[i + 1] & LOWER);
      key[i] = key[i + 397] ^ (y >> 1) ^ (-(int32_t)(y & 1) & MAT);
    }
    for (; i < 623; ++i) {
      y = (key[i] & UPPER) | (key[i + 1] & LOWER);
      key[i] = key[i + (397 - 624)] ^ (y >> 1) ^ (-(int32_t)(y & 1) & MAT);
    }
    y = (key[623] & UPPER) | (key[0] & LOWER);
    key[623] = key[396] ^ (y >> 1) ^ (-(int32_t)(y & 1) & MAT);
  }
  DES_HD uint32_t next32(int g) {
    if (draws_left <= 0) {
      if (!stop) stop = DES_STOP_BUDGET;
      return 0;
    }
    --draws_left;
    uint32_t* key = key_of(g);
    uint32_t p = (uint32_t)pos[g];
    if (p >= DES_MT_N) {                              // (an out-of-range position cannot form an address)
      twist(key);
      p = 0;
    }
    uint32_t y = key[p];
    pos[g] = (int32_t)(p + 1);
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
  DES_HD double next_double(int g) {                  // random_sample: 53 bits from two draws
    const int32_t a = (int32_t)(next32(g) >> 5), b = (int32_t)(next32(g) >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
  }
  // randint(low, high) for a range below 2^32: masked rejection on 32-bit draws (_bounded_integers, use_masked)
  DES_HD int64_t randint(int g, int64_t low, int64_t high) {
    const uint64_t rng = (uint64_t)(high - 1 - low);
    if (rng == 0) return low;
    uint32_t mask = (uint32_t)rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v;
    do { v = next32(g) & mask; } while (v > (uint32_t)rng && !stop);
    return low + (int64_t)v;
  }
  DES_HD double standard_normal(int g) {              // legacy_gauss: polar Box-Muller with one cached value
    if (has_gauss[g]) {
      const double t = gauss[g];
      has_gauss[g] = 0;
      gauss[g] = 0.0;
      return t;
    }
    double f, x1, x2, r2;
    do {
      x1 = 2.0 * next_double(g) - 1.0;
      x2 = 2.0 * next_double(g) - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while ((r2 >= 1.0 || r2 == 0.0) && !stop);
    if (stop) return 0.0;
    f = Math::sqrt(-2.0 * Math::log(r2) / r2);
    gauss[g] = f * x1;
    has_gauss[g] = 1;
    return f * x2;
  }
  // scipy.stats.norm(loc, scale).rvs(random_state=rng): no draw at all when scale == 0
  DES_HD double norm_rvs(int node) {
    if (scale[node] == 0.0) return loc[node];
    const double z = standard_normal(node);
    return z * scale[node] + loc[node];
  }

  // ---- setup ----
  // source flags, routing tables and idle servers for nodes [first, dim) in steps of `step` (one lane per node on the
  // device); a negative scale (scipy: "Domain error in arguments") ends the sample
  DES_HD void setup_nodes(const double* adj, int first, int step) {
    for (int i = first; i < dim; i += step) {
      is_source[i] = adj[(int64_t)i * dim + i] > 0;    // sources: diagonal > 0; servers: diagonal <= 0 (363, 379)
      make_branch(adj + (int64_t)i * dim, dim, i, children + (int64_t)i * dim, cdf + (int64_t)i * dim, &nchild[i],
                  &bflags[i]);
      in_service[i] = 0;
      qhead[i] = 0;
      qlen[i] = 0;
    }
  }
  // what the batch entries require of one sample before anything runs (a refused sample stops with DES_STOP_ERROR and
  // leaves the generator state as it came): scale >= 0, every queue fits its ring, a 32-bit seed, a valid position,
  // every kind one the policy knows
  DES_HD bool spec_ok(int64_t seed, int32_t global_pos) const {
    if (seed < 0 || seed > 0xffffffffLL || global_pos < 0 || global_pos > DES_MT_N) return false;
    for (int i = 0; i < dim; ++i)
      if (!(scale[i] >= 0) || (int64_t)qcap[i] > ring_stride) return false;
    return dist.kinds_ok(dim);
  }
  // per-node generator seeds (451-461): servers first, then sources, each in ascending node order
  DES_HD void draw_node_seeds(uint32_t seed, uint32_t* node_seed) {
    const int g = dim + 1;
    seed_key(seeder_key, seed);
    pos[g] = DES_MT_N;
    has_gauss[g] = 0;
    gauss[g] = 0.0;
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < dim; ++i)
        if ((is_source[i] != 0) == (pass == 1)) node_seed[i] = (uint32_t)randint(g, 3, 9999999);
  }
  DES_HD void seed_nodes(const uint32_t* node_seed, int first, int step) {
    for (int i = first; i < dim; i += step) {
      seed_key(node_keys + (int64_t)i * DES_MT_N, node_seed[i]);
      pos[i] = DES_MT_N;
      has_gauss[i] = 0;
      gauss[i] = 0.0;
    }
  }

  // ---- Python's heapq ----
  DES_HD void push(const Ev& e) {                      // heappush = append + _siftdown(heap, 0, len - 1)
    if (heap_n >= heap_cap) { fail(); return; }
    int p = heap_n++;
    while (p > 0) {
      const int parent = (p - 1) >> 1;
      if (e.time < heap[parent].time) { heap[p] = heap[parent]; p = parent; continue; }
      break;
    }
    heap[p] = e;
  }
  DES_HD Ev pop() {                                    // heappop: last element to the root, _siftup, then _siftdown
    const Ev last = heap[--heap_n];
    if (heap_n == 0) return last;
    const Ev ret = heap[0];
    const int end = heap_n;
    int p = 0, child = 1;
    while (child < end) {
      const int right = child + 1;
      if (right < end && !(heap[child].time < heap[right].time)) child = right;
      heap[p] = heap[child];
      p = child;
      child = 2 * p + 1;
    }
    while (p > 0) {                                    // _siftdown(heap, 0, pos)
      const int parent = (p - 1) >> 1;
      if (last.time < heap[parent].time) { heap[p] = heap[parent]; p = parent; continue; }
      break;
    }
    heap[p] = last;
    return ret;
  }

  // ---- the simulation ----
  DES_HD void log(double v, int64_t id, int node, int kind) {
    if (n_out < out_cap) out.put(n_out, v, id, node, kind);
    else overflow = true;
    ++n_out;
    if (max_records > 0 && n_out >= max_records && !stop) stop = DES_STOP_RECORDS;
  }
  // np.random.choice(children[, p]) on the GLOBAL legacy stream; -1 = a sink-like server (get_destination, 699-743)
  DES_HD int destination(int id) {
    if (!is_source[id] && (bflags[id] & DES_BRANCH_SINK)) return -1;
    const int n = nchild[id];
    if (n <= 0 || n > dim) { fail(); return -1; }      // "No children available" / np.random.choice([]) raises
    const int32_t* ch = children + (int64_t)id * dim;
    if (bflags[id] & DES_BRANCH_UNIFORM) {
      const int64_t k = randint(dim, 0, n);
      if (stop || k < 0 || k >= n) { fail(); return -1; }
      return ch[k];
    }
    // legacy choice with p: searchsorted(cdf, random_sample(), side='right')
    const double* c = cdf + (int64_t)id * dim;
    const double u = next_double(dim);
    if (stop) return -1;
    int lo = 0, hi = n;                                // first index with cdf[i] > u
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return ch[lo < n ? lo : n - 1];
  }
  DES_HD void schedule_departure(int server_id, int64_t event_id) {     // 591-612
    in_service[server_id] = 1;
    double service = 0.0;
    if (!dist.timeless(server_id)) {                   // (598: a queue or branch node draws nothing, its service is 0)
      // upstream: the loop never ends -- no draw is made (scale 0: nothing counts against the budget) and the value is <= 0
      if (scale[server_id] == 0.0 && (dist.ignores_loc(server_id) || loc[server_id] <= 0.0)) { fail(); return; }
      while (service <= 0 && !stop) service = dist.rvs(*this, server_id);
      if (stop) return;
    }
    stats.service(server_id, service);
    log(service, event_id, server_id, 2);
    if (stop) return;
    push(Ev{clock + service, event_id, 2, server_id, -1, 0});
    dist.scheduled(server_id, clock + service);
  }
  DES_HD void process_arrival(int server_id, int source, int64_t id) {  // 536-588
    log(clock, id, server_id, 0);
    if (stop) return;
    if (server_id < 0 || server_id >= dim || is_source[server_id]) { fail(); return; }    // KeyError upstream
    if (in_service[server_id] == 0) {
      schedule_departure(server_id, id);
      if (stop) return;
    } else if ((int64_t)qlen[server_id] + dist.held(server_id) < (int64_t)qcap[server_id]) {
      const int64_t n = qlen[server_id];
      if (n < 0 || n >= ring_stride) { fail(); return; }
      int64_t slot = (int64_t)qhead[server_id] + n;
      if (slot >= ring_stride) slot -= ring_stride;
      if (slot < 0 || slot >= ring_stride) { fail(); return; }
      ring[(int64_t)server_id * ring_stride + slot] = id;
      qlen[server_id] = (int32_t)(n + 1);
      stats.enqueue(server_id, slot, clock, n, dist.held(server_id));
    } else {
      stats.renege(server_id);                         // the customer reneges
    }
    if (source >= 0) {
      const double dt = dist.rvs(*this, source);
      if (stop) return;
      stats.generate(source, dt);
      push(Ev{clock + dt, total_customers, 1, server_id, source, 0});
      ++total_customers;
    }
  }
  DES_HD void process_departure(int server_id, int64_t id, int was_delayed) {            // 615-677
    log(clock, id, server_id, 1);
    if (stop) return;
    if (server_id < 0 || server_id >= dim) { fail(); return; }
    dist.popped(*this, server_id, was_delayed);
    int next = dist.waits(server_id) ? -1 : destination(server_id);
    if (stop) return;
    const bool sink = (bflags[server_id] & DES_BRANCH_SINK) != 0;
    if (next < 0) {                                    // sink-like node: first idle child that is a server (628-633)
      const int32_t* ch = children + (int64_t)server_id * dim;
      const int n = nchild[server_id] < dim ? nchild[server_id] : dim;
      for (int k = 0; k < n; ++k) {
        const int c = ch[k];
        if (c >= 0 && c < dim && !is_source[c] && in_service[c] == 0) { next = c; break; }
      }
    }
    if (next >= 0 || sink) {
      if (qlen[server_id] > 0) {
        const int64_t h = qhead[server_id];
        if (h < 0 || h >= ring_stride) { fail(); return; }
        const int64_t customer = ring[(int64_t)server_id * ring_stride + h];
        qhead[server_id] = (int32_t)(h + 1 >= ring_stride ? 0 : h + 1);
        stats.dequeue(server_id, h, clock, qlen[server_id] + dist.held(server_id));
        --qlen[server_id];
        schedule_departure(server_id, customer);
        if (stop) return;
      } else {
        in_service[server_id] = 0;
        dist.idle(server_id);
      }
      if (!sink) process_arrival(next, -1, id);
    } else {
      dist.delay(*this, server_id, id);                // queue-type nodes (delayed departures): AnyNode only, else an error
    }
  }

  // Initialization (518-534) and the event loop (463-516).  Node tables and generators are set up; returns the stop
  // reason.  max_events <= 0: no event cap (gdm_des_run only).
  DES_HD int run(int64_t number_of_customers, int64_t max_events) {
    for (int i = 0; i < dim && !stop; ++i) {
      if (!is_source[i]) continue;
      const double dt = dist.rvs(*this, i);
      if (stop) break;
      stats.generate(i, dt);
      const int next = destination(i);
      if (stop) break;
      push(Ev{clock + dt, total_customers, 1, next, i, 0});
      ++total_customers;
    }
    int reason = DES_STOP_EMPTY;
    int64_t processed = 0;
    while (!stop && heap_n > 0) {
      const Ev evt = pop();
      stats.pop(evt.time);                             // counted in the time integration before the break (472-486)
      stats.checkpoint(total_customers, clock, qlen, dist, n_out, processed);
      if (total_customers > number_of_customers - 1) { reason = DES_STOP_CUSTOMERS; break; }
      clock = evt.time;
      stats.event();
      if (evt.type == 1) process_arrival(evt.server, evt.source, evt.id);
      else process_departure(evt.server, evt.id, evt.pad);
      if (++processed >= max_events && max_events > 0) { reason = DES_STOP_EVENTS; break; }   // (reference: wall clock)
    }
    stats.finish(is_source, qlen, dim, dist);
    return stop ? stop : reason;
  }
};

}  // namespace des
