// 'Music' logs of B simulations -> two tables per sample: one row per VISIT (a customer's stay at one node) and one row
// per CUSTOMER (an event_id), the walk of des_visits.h over every sample's records [rec_ptr[b], rec_ptr[b + 1]).
// include/gdm.h states the columns and the refusals.
//
// Host code only: this file holds no kernel and gdm_des_log_visits_host takes no stream.  A log that lives on the device
// is read back once by the caller (simulation_v3.log_visits).  The kernel is described, and not built, in DESIGN.md
// section 7.
//
// Every sample is walked twice: once without tables (checked and counted), and, when it is healthy and its rows fit
// behind those of the samples before it, once more writing them.  Bounds: a record index stays inside [rec_ptr[b],
// rec_ptr[b + 1]), which is checked against n_records; an event id is checked against the scratch table's length and a
// node against dim before either is used; a sample's rows are written only when all of them lie below the caps.
#include <vector>
#include "gdm_common.h"
#include "des_visits.h"

static_assert(DES_VISITS_ERECORD == GDM_DES_VISITS_ERECORD, "status codes");
static_assert(DES_VISIT_UNSERVED == GDM_DES_VISIT_UNSERVED && DES_VISIT_IN_SERVICE == GDM_DES_VISIT_IN_SERVICE &&
                  DES_VISIT_DEPARTED == GDM_DES_VISIT_DEPARTED,
              "visit outcomes");
static_assert(DES_CUST_ABSENT == GDM_DES_CUST_ABSENT && DES_CUST_UNSERVED == GDM_DES_CUST_UNSERVED &&
                  DES_CUST_IN_NET == GDM_DES_CUST_IN_NET && DES_CUST_EXITED == GDM_DES_CUST_EXITED,
              "customer outcomes");

extern "C" int gdm_des_log_visits_host(const double* value, const int64_t* event_id, const int32_t* node,
                                       const int32_t* kind, const int64_t* rec_ptr, int64_t n_records, int B, int dim,
                                       int64_t* visit_ptr, int64_t* cust_ptr, int32_t* status, int32_t* visit_i32,
                                       int64_t* visit_i64, double* visit_f64, int64_t n_visits_cap, int32_t* cust_i32,
                                       int64_t* cust_i64, double* cust_f64, int64_t n_customers_cap) {
  const char* who = "gdm_des_log_visits_host";
  GDM_REQUIRE(rec_ptr && visit_ptr && cust_ptr && status && (n_records == 0 || (value && event_id && node && kind)),
              "%s: null pointer", who);
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && dim >= 1 && dim <= GDM_DES_VISITS_MAX_DIM && n_records >= 0 &&
                  n_records <= GDM_DES_VISITS_MAX_RECORDS,
              "%s: 1 <= B <= 2^20, 1 <= dim <= %d, 0 <= n_records <= 2^40", who, GDM_DES_VISITS_MAX_DIM);
  GDM_REQUIRE(n_visits_cap >= 0 && n_customers_cap >= 0 && n_visits_cap <= GDM_DES_VISITS_MAX_RECORDS &&
                  n_customers_cap <= 2 * GDM_DES_VISITS_MAX_RECORDS,
              "%s: 0 <= n_visits_cap <= 2^40 and 0 <= n_customers_cap <= 2^41", who);
  const bool fill = visit_i32 && visit_i64 && visit_f64 && cust_i32 && cust_i64 && cust_f64;
  const bool counting = !visit_i32 && !visit_i64 && !visit_f64 && !cust_i32 && !cust_i64 && !cust_f64;
  GDM_REQUIRE(fill || (counting && n_visits_cap == 0 && n_customers_cap == 0),
              "%s: null pointer (the six tables are given together -- the customer sums are read off the visit rows -- "
              "or not at all, with both caps 0)", who);
  GDM_REQUIRE((((uintptr_t)node | (uintptr_t)kind | (uintptr_t)status | (uintptr_t)visit_i32 | (uintptr_t)cust_i32) & 3) == 0 &&
                  (((uintptr_t)value | (uintptr_t)event_id | (uintptr_t)rec_ptr | (uintptr_t)visit_ptr |
                    (uintptr_t)cust_ptr | (uintptr_t)visit_i64 | (uintptr_t)visit_f64 | (uintptr_t)cust_i64 |
                    (uintptr_t)cust_f64) & 7) == 0,
              "%s: an array is not aligned to its element size", who);
  std::vector<des_visits::Open> open;
  int64_t at_v = 0, at_c = 0;
  visit_ptr[0] = cust_ptr[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t lo = rec_ptr[b], hi = rec_ptr[b + 1];
    int64_t nv = 0, nc = 0;
    int st = GDM_DES_VISITS_EPTR;
    if (lo >= 0 && hi >= lo && hi <= n_records) {
      const int64_t n = hi - lo;
      open.resize((size_t)des_visits::scratch_entries(n, dim));
      des_visits::sample_walk(value, event_id, node, kind, lo, n, dim, open.data(), nullptr, nullptr, &nv, &nc, &st);
      if (st == 0 && fill && at_v + nv <= n_visits_cap && at_c + nc <= n_customers_cap) {
        const int64_t vc = n_visits_cap, cc = n_customers_cap;      // column k of a block starts at k * cap
        const des_visits::Visits vis{visit_i32 + at_v,          visit_i32 + vc + at_v,     visit_i32 + 2 * vc + at_v,
                                     visit_i64 + at_v,          visit_i64 + vc + at_v,     visit_i64 + 2 * vc + at_v,
                                     visit_i64 + 3 * vc + at_v, visit_i64 + 4 * vc + at_v, visit_i64 + 5 * vc + at_v,
                                     visit_i64 + 6 * vc + at_v, visit_f64 + at_v,          visit_f64 + vc + at_v,
                                     visit_f64 + 2 * vc + at_v, visit_f64 + 3 * vc + at_v, visit_f64 + 4 * vc + at_v};
        const des_visits::Customers cust{cust_i64 + at_c,          cust_i64 + cc + at_c,    cust_i32 + at_c,
                                         cust_i32 + cc + at_c,     cust_f64 + at_c,         cust_f64 + cc + at_c,
                                         cust_f64 + 2 * cc + at_c, cust_f64 + 3 * cc + at_c};
        des_visits::sample_walk(value, event_id, node, kind, lo, n, dim, open.data(), &vis, &cust, &nv, &nc, &st);
      }
    }
    at_v += nv;
    at_c += nc;
    status[b] = st;
    visit_ptr[b + 1] = at_v;
    cust_ptr[b + 1] = at_c;
  }
  if (fill && (at_v > n_visits_cap || at_c > n_customers_cap)) {
    gdm_set_error("%s: tables too small (%lld visit rows and %lld customer rows needed)", who, (long long)at_v,
                  (long long)at_c);
    return GDM_EWORKSPACE;
  }
  return GDM_OK;
}
