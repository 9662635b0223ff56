"""The visit walk of csrc/des_visits.h once more, in plain Python over dicts and lists: the oracle of
tests/test_des_visits.py.  It shares no code with the C++ walk or with simulation_v3: it reads one sample's records
(value, event_id, node, kind) and returns the columns of simulation_v3.LogVisits for that sample as numpy arrays, or
None for a log the walk refuses.

``fault`` plants one named mistake, so that the tests can show that each of them changes a table:
  first_departure        keeps the FIRST departure of a visit as rec_depart / t_depart (a queue node's delayed
                         departures are several records of one visit; the last one is when the customer left)
  clock_from_processing  takes t_start from the processing record's own value (which is the service time) instead of
                         the clock record before it
  no_reopen              a customer's second visit to a node reuses its first visit there instead of opening a new one
"""
import numpy as np

FAULTS = ("first_departure", "clock_from_processing", "no_reopen")
UNSERVED, IN_SERVICE, DEPARTED = 0, 1, 2
CUST_ABSENT, CUST_UNSERVED, CUST_IN_NET, CUST_EXITED = -1, 0, 1, 2
NAN = float("nan")
VISIT_COLUMNS = (("node", np.int32), ("n_departures", np.int32), ("outcome", np.int32), ("event_id", np.int64),
                 ("rec_arrival", np.int64), ("rec_start", np.int64), ("rec_first_depart", np.int64),
                 ("rec_depart", np.int64), ("prev_visit", np.int64), ("next_visit", np.int64), ("t_arrival", np.float64),
                 ("t_start", np.float64), ("service", np.float64), ("t_first_depart", np.float64), ("t_depart", np.float64))
CUST_COLUMNS = (("cust_n_visits", np.int32), ("cust_outcome", np.int32), ("cust_first_visit", np.int64),
                ("cust_last_visit", np.int64), ("cust_t_enter", np.float64), ("cust_t_exit", np.float64),
                ("cust_service_sum", np.float64), ("cust_wait_sum", np.float64))


def walk(value, event_id, node, kind, dim, fault=None):
    """One sample's records -> {column: array} (VISIT_COLUMNS then CUST_COLUMNS), or None when the log is refused."""
    assert fault is None or fault in FAULTS, fault
    n = len(value)
    visits = []                                           # one dict per visit, in arrival order
    mine = {}                                             # event id -> the indices of its visits, in order
    at_node = {}                                          # (event id, node) -> its first visit there (no_reopen)
    clock = None
    for i in range(n):
        t, e, nd, k = float(value[i]), int(event_id[i]), int(node[i]), int(kind[i])
        if k not in (0, 1, 2) or not 0 <= nd < dim or not 0 <= e <= n + dim:
            return None
        chain = mine.setdefault(e, [])
        if k == 0:
            if fault == "no_reopen" and (e, nd) in at_node:
                chain.append(at_node[e, nd])              # the planted mistake: the old visit is the open one again
            else:
                visits.append(dict(node=nd, n_departures=0, outcome=UNSERVED, event_id=e, rec_arrival=i, rec_start=-1,
                                   rec_first_depart=-1, rec_depart=-1, prev_visit=chain[-1] if chain else -1,
                                   next_visit=-1, t_arrival=t, t_start=NAN, service=NAN, t_first_depart=NAN,
                                   t_depart=NAN))
                if chain:
                    visits[chain[-1]]["next_visit"] = len(visits) - 1
                chain.append(len(visits) - 1)
                at_node.setdefault((e, nd), len(visits) - 1)
            clock = t
            continue
        if not chain:
            return None
        v = visits[chain[-1]]
        if v["node"] != nd:
            return None
        if k == 2:
            if v["rec_start"] >= 0 and fault != "no_reopen":
                return None
            if clock is None:
                return None
            v.update(rec_start=i, service=t, t_start=t if fault == "clock_from_processing" else clock, outcome=IN_SERVICE)
        else:
            if v["rec_start"] < 0:
                return None
            v["n_departures"] += 1
            if v["n_departures"] == 1:
                v.update(rec_first_depart=i, t_first_depart=t)
            if v["n_departures"] == 1 or fault != "first_departure":
                v.update(rec_depart=i, t_depart=t)
            v["outcome"] = DEPARTED
            clock = t
    seen = [e for e, chain in mine.items() if chain]
    customers = []
    for e in range(max(seen) + 1 if seen else 0):
        chain = list(dict.fromkeys(mine.get(e, [])))      # (no_reopen may name a visit twice)
        row = dict(cust_n_visits=len(chain), cust_outcome=CUST_ABSENT, cust_first_visit=-1, cust_last_visit=-1,
                   cust_t_enter=NAN, cust_t_exit=NAN, cust_service_sum=0.0, cust_wait_sum=0.0)
        if chain:
            first, last = visits[chain[0]], visits[mine[e][-1]]
            row.update(cust_first_visit=chain[0], cust_last_visit=mine[e][-1], cust_t_enter=first["t_arrival"],
                       cust_outcome={DEPARTED: CUST_EXITED, IN_SERVICE: CUST_IN_NET, UNSERVED: CUST_UNSERVED}[last["outcome"]])
            if last["outcome"] == DEPARTED:
                row["cust_t_exit"] = last["t_depart"]
            for j in chain:
                if visits[j]["rec_start"] >= 0:
                    row["cust_service_sum"] += visits[j]["service"]
                    row["cust_wait_sum"] += visits[j]["t_start"] - visits[j]["t_arrival"]
        customers.append(row)
    out = {name: np.array([v[name] for v in visits], dtype=dt) for name, dt in VISIT_COLUMNS}
    out.update({name: np.array([c[name] for c in customers], dtype=dt) for name, dt in CUST_COLUMNS})
    return out


def walk_records(rec, dim, fault=None):
    """``walk`` on an EVENT_DTYPE record array."""
    return walk(rec["value"], rec["event_id"], rec["node"], rec["kind"], dim, fault)
