// The visit walk for ONE 'Music' log on the host, record by record: what gdm_des_log_visits_host runs per sample and
// tools/des_visits_host.cpp runs under the host sanitizers.  Plain C++, no HIP.
//
// An event_id is a customer and keeps its id from node to node.  Every 'arrival' record opens a VISIT (the customer's
// stay at one node); a customer's OPEN visit is its latest one.  A 'processing' record starts the open visit (its
// clock is the value of the latest arrival or departure record before it: the simulator writes the record inside the
// event that starts the service, and the processing record's own value is the service time), a 'departure' record
// ends it -- every one of them: a 'queue' node's delayed departures are several departure records of one visit, and
// the last one wins.  The walk copies doubles of the log into the visit table and does no arithmetic on them; the
// customer table's two sums are formed along the customer's chain of visits, in visit order.
//
// What the log cannot tell: an UNSERVED visit was turned away, or was still waiting when the log ended; a queue node's
// customer whose last logged departure was a delayed one reads as DEPARTED at that clock (at most one per queue node
// and log); a customer whose last visit DEPARTED reads as EXITED although its next arrival may lie behind the log's end.
#pragma once
#include <cstdint>
#include <limits>

#define DES_VISITS_ERECORD 1 /* a record the walk cannot place (include/gdm.h lists the cases) */

#define DES_VISIT_UNSERVED 0   /* never started */
#define DES_VISIT_IN_SERVICE 1 /* started, no departure logged */
#define DES_VISIT_DEPARTED 2   /* a departure was logged */
#define DES_CUST_ABSENT (-1)   /* an id below the largest one seen that has no record */
#define DES_CUST_UNSERVED 0    /* by the customer's last visit */
#define DES_CUST_IN_NET 1
#define DES_CUST_EXITED 2

namespace des_visits {

// The columns of a sample's visit rows and customer rows (the sample's first row at index 0).
struct Visits {
  int32_t *node, *n_departures, *outcome;
  int64_t *event_id, *rec_arrival, *rec_start, *rec_first_depart, *rec_depart, *prev_visit, *next_visit;
  double *t_arrival, *t_start, *service, *t_first_depart, *t_depart;
};
struct Customers {
  int64_t *first_visit, *last_visit;
  int32_t *n_visits, *outcome;
  double *t_enter, *t_exit, *service_sum, *wait_sum;
};

// A customer's open visit: its index (-1: none yet), its node, and how far it got (the DES_VISIT_* value).
struct Open {
  int64_t visit;
  int32_t node, phase;
};

// The number of `Open` entries a log of n records over dim nodes needs: no well-formed log names an id above n + dim
// (an id is handed out at the latest when an earlier arrival of its source is processed).
inline int64_t scratch_entries(int64_t n, int dim) { return n + dim + 1; }

// Records [lo, lo + n) of value / event_id / node / kind; open: scratch_entries(n, dim) entries.  vis and cust null:
// the sample is checked and counted only; both given: every row is written, and they must hold *n_visits and
// *n_customers rows (the counts of an earlier call).  *status = DES_VISITS_ERECORD and both counts 0 for a log the
// walk cannot place; the rows of such a sample are not defined.
inline void sample_walk(const double* value, const int64_t* event_id, const int32_t* node, const int32_t* kind,
                        int64_t lo, int64_t n, int dim, Open* open, const Visits* vis, const Customers* cust,
                        int64_t* n_visits, int64_t* n_customers, int* status) {
  const double none = std::numeric_limits<double>::quiet_NaN();
  const int64_t ids = scratch_entries(n, dim);
  for (int64_t e = 0; e < ids; ++e) open[e] = Open{-1, -1, DES_VISIT_UNSERVED};
  *n_visits = *n_customers = 0;
  *status = DES_VISITS_ERECORD;
  int64_t nv = 0, top = -1, clock_rec = -1;               // clock_rec: the latest arrival or departure record
  for (int64_t i = 0; i < n; ++i) {
    const int32_t k = kind[lo + i], nd = node[lo + i];
    const int64_t e = event_id[lo + i];
    if (k < 0 || k > 2 || nd < 0 || nd >= dim || e < 0 || e >= ids) return;
    Open& o = open[e];
    if (k == 0) {                                         // arrival: a new visit
      const int64_t v = nv++;
      if (vis) {
        vis->node[v] = nd;
        vis->n_departures[v] = 0;
        vis->outcome[v] = DES_VISIT_UNSERVED;
        vis->event_id[v] = e;
        vis->rec_arrival[v] = i;
        vis->rec_start[v] = vis->rec_first_depart[v] = vis->rec_depart[v] = vis->next_visit[v] = -1;
        vis->prev_visit[v] = o.visit;
        vis->t_arrival[v] = value[lo + i];
        vis->t_start[v] = vis->service[v] = vis->t_first_depart[v] = vis->t_depart[v] = none;
        if (o.visit >= 0) vis->next_visit[o.visit] = v;
      }
      if (cust) {
        for (; top < e; ++top) {                          // the rows up to this id, absent until seen
          const int64_t r = top + 1;
          cust->first_visit[r] = cust->last_visit[r] = -1;
          cust->n_visits[r] = 0;
          cust->outcome[r] = DES_CUST_ABSENT;
          cust->t_enter[r] = cust->t_exit[r] = none;
          cust->service_sum[r] = cust->wait_sum[r] = 0.0;
        }
        if (o.visit < 0) {
          cust->first_visit[e] = v;
          cust->t_enter[e] = value[lo + i];
        }
        cust->last_visit[e] = v;
        ++cust->n_visits[e];
      }
      top = e > top ? e : top;
      o = Open{v, nd, DES_VISIT_UNSERVED};
      clock_rec = i;
    } else if (k == 2) {                                  // processing: the open visit starts
      // (an open visit has an arrival record before it, so there is a clock record: clock_rec >= 0)
      if (o.visit < 0 || o.node != nd || o.phase != DES_VISIT_UNSERVED || clock_rec < 0) return;
      o.phase = DES_VISIT_IN_SERVICE;
      if (vis) {
        vis->rec_start[o.visit] = i;
        vis->service[o.visit] = value[lo + i];
        vis->t_start[o.visit] = value[lo + clock_rec];
        vis->outcome[o.visit] = DES_VISIT_IN_SERVICE;
      }
    } else {                                              // departure: the last one wins
      if (o.visit < 0 || o.node != nd || o.phase == DES_VISIT_UNSERVED) return;
      o.phase = DES_VISIT_DEPARTED;
      if (vis) {
        if (vis->n_departures[o.visit]++ == 0) {
          vis->rec_first_depart[o.visit] = i;
          vis->t_first_depart[o.visit] = value[lo + i];
        }
        vis->rec_depart[o.visit] = i;
        vis->t_depart[o.visit] = value[lo + i];
        vis->outcome[o.visit] = DES_VISIT_DEPARTED;
      }
      clock_rec = i;
    }
  }
  if (vis && cust) {
    for (int64_t e = 0; e <= top; ++e) {                  // the sums along the chain, the end by the last visit
      double service = 0.0, wait = 0.0;
      for (int64_t v = cust->first_visit[e]; v >= 0; v = vis->next_visit[v]) {
        if (vis->rec_start[v] < 0) continue;
        service += vis->service[v];
        wait += vis->t_start[v] - vis->t_arrival[v];
      }
      cust->service_sum[e] = service;
      cust->wait_sum[e] = wait;
      const int64_t last = cust->last_visit[e];
      if (last < 0) continue;
      const int32_t end = vis->outcome[last];
      cust->outcome[e] = end == DES_VISIT_DEPARTED ? DES_CUST_EXITED
                                                   : (end == DES_VISIT_IN_SERVICE ? DES_CUST_IN_NET : DES_CUST_UNSERVED);
      if (end == DES_VISIT_DEPARTED) cust->t_exit[e] = vis->t_depart[last];
    }
  }
  *n_visits = nv;
  *n_customers = top + 1;
  *status = 0;
}

}  // namespace des_visits
