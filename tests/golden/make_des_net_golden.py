#!/usr/bin/env python3
"""Generate tests/golden/des_net.npz: the REFERENCE's own ``Sim`` on nets with its two node kinds that have no
distribution, ``['queue']`` (a waiting room in front of several servers) and ``['branch']`` (a zero-time router); needs
the reference checkout, like make_golden.py, whose ``load_reference``, ``_corpus_net`` and ``_corpus_random_net`` this
imports, and make_des_dist_golden.py's ``accumulators`` -- nothing of the reference's text is copied.

Run from the repo root:   python tests/golden/make_des_net_golden.py

1. A corpus (``names``): nets of at most 400 customers, each run in 'Music' mode from ``np.random.seed(np_seed)`` with
   one seed.  Stored per case: the inputs -- sim_matrix, kind (the index into simulation_v3.NODE_KINDS), loc, scale
   (0 for a queue or branch node), queue_list, seed, customers, np_seed --; the log (value, event_id, node, rec_kind);
   the fields des_stats.npz stores, read from the reference's objects after ``Sim.run`` (queue_time has one column more
   than the largest capacity + 1: a delayed departure counts as waiting); the whole final global generator state; and
   the witnesses, counted by wrapping the reference's own methods: ``delayed`` (calls of schedule_delayed_departure),
   ``redelayed`` (calls for an event of a node that was already delayed at the same time: it lost the tie against the
   departure it waits for and was delayed again) and ``popped`` (events taken off the list).

     mm2_cap2      source -> queue node (2 places) -> 2 exponential servers
     cap0          a station whose queue node has capacity 0: it still holds one customer, the delayed departure
     c1, c4        one server / four servers behind the queue node
     shared        the station's servers feed one downstream server with its own queue: the children are not sinks
     branch37      a branch node splitting 0.3 / 0.7
     branch_queue  a branch node in front of two stations
     mixed         a station whose servers are normal, uniform and exponential
     det_tie       deterministic (uniform with scale 0): delayed departures tie with arrivals and with the departure
                   they wait for, and some lose the tie
     sink_quirk    a queue node whose only child is node 0: a sink by the reference's ``sum(children) == 0``
     embed16, embed128   a queue node and a branch node put into a seeded random net of 16 / 128 nodes
     raises        a branch node that routes to a source: the reference raises KeyError; only the inputs and the name
                   of the exception are stored

2. The validation grid (``grid/...``): GRID, six M/M/c/N configurations (c 1..4, rho = lam / (c mu) from 0.5 to 1.5,
   capacities 0..3) x GRID_SEEDS x 4000 customers on the net source -> queue node -> c exponential sinks of capacity
   0, each run from the global stream ``RandomState([seed, 1])``.  Stored per run (configuration-major) the
   accumulators of the source, the queue node and the servers (rows padded to the largest dim).  The generator ASSERTS
   that for every compared quantity (blocked fraction at the queue node, mean server utilisation, LQ, WQ, the law of
   the number waiting) the reference's mean over the 16 seeds lies within 4 standard errors of
   ``queueing_theory.mmck`` with N = c + max(queue_cap, 1); the largest |z| is stored as ``grid/max_abs_z``.  A
   configuration that fails is to be REPLACED, never the bound.
"""
import logging
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg                      # noqa: E402
import make_des_dist_golden as mdd            # noqa: E402
from gan_des_midi_music_gen_amd import queueing_theory as qt   # noqa: E402

KINDS = ("normal", "exponential", "uniform", "queue", "branch")
REC_KINDS = ("arrival", "departure", "processing")
LINE = re.compile(r"INFO:root:(\S+) - (\S+) - (\S+) - (arrival|departure|processing)$")
GRID = ((1, 0.8, 1.0, 0), (2, 1.5, 1.0, 2), (2, 1.0, 1.0, 1), (3, 2.0, 1.0, 3), (4, 6.0, 1.0, 2), (3, 1.5, 1.0, 0))
GRID_SEEDS = tuple(101 + 7 * i for i in range(16))     # c, lam, mu, cap above
GRID_CUSTOMERS = 4000
Z_BOUND = 4.0
SIZE_BOUND = 400000


def station(c, lam, mu, cap):
    """source -> queue node -> c exponential sinks of capacity 0 (what simulation_v3.mmck_spec builds)."""
    dim = c + 2
    adj = np.zeros((dim, dim))
    adj[0, 0] = adj[0, 1] = 1.0
    adj[1, 2:] = 1.0
    return {"sim_matrix": adj, "queue_list": [0, cap] + [0] * c,
            "distributions": [["exponential", 1.0 / lam], ["queue"]] + [["exponential", 1.0 / mu] for _ in range(c)]}


def embed(S, dim, net_seed, seed, customers, np_seed):
    """_corpus_random_net with a station put in.  A source keeps the one destination it drew at the start, so which
    servers see customers at all depends on the run: the reference first runs the plain net under the case's seeds;
    the server with two or more server children that served most becomes a queue node, its children serve four times
    as long (so that they are busy when the next customer comes), and the busiest other server with a child, outside
    the station, becomes a branch node."""
    spec, sources = mg._corpus_random_net(dim, net_seed)
    adj = spec["sim_matrix"]
    kids = {i: [j for j in range(dim) if j != i and adj[i, j] > 0 and j not in sources] for i in range(dim)}
    np.random.seed(np_seed)
    plain, _recs, _w = run_reference(S, spec, seed, customers, False)
    busy = sorted(plain.servers, key=lambda i: -plain.servers[i].total_customers_served)
    q = next(i for i in busy if len(kids[i]) >= 2)
    b = next(i for i in busy if i != q and len(kids[i]) >= 1 and i not in kids[q])
    dist = [["normal", float(m), float(s)] for _n, m, s in spec["distributions"]]
    for j in kids[q]:
        dist[j][1] *= 4.0
    dist[q], dist[b] = ["queue"], ["branch"]
    return {"sim_matrix": adj, "distributions": dist, "queue_list": spec["queue_list"]}


def cases(S):
    """name -> (spec, seed, customers, np_seed); S: the reference's module (``embed`` runs it)."""
    C = {}
    C["mm2_cap2"] = (station(2, 1.5, 1.0, 2), 5301, 300, 51)
    C["cap0"] = (station(2, 2.0, 1.0, 0), 5302, 200, 52)
    C["c1"] = (station(1, 0.9, 1.0, 1), 5303, 200, 53)
    C["c4"] = (station(4, 5.0, 1.0, 3), 5304, 300, 54)
    sh = mg._corpus_net(5, [0], {(0, 1): 1.0, (1, 2): 1.0, (1, 3): 1.0, (2, 4): 1.0, (3, 4): 1.0}, {},
                        {1: 3, 2: 0, 3: 0, 4: 2})
    sh["distributions"] = [["exponential", 0.5], ["queue"], ["exponential", 1.0], ["exponential", 1.25],
                           ["exponential", 0.75]]
    C["shared"] = (sh, 5305, 300, 55)
    br = mg._corpus_net(4, [0], {(0, 1): 1.0, (1, 2): 0.3, (1, 3): 0.7}, {}, 2)
    br["distributions"] = [["exponential", 0.5], ["branch"], ["exponential", 0.75], ["uniform", 0.125, 0.5]]
    C["branch37"] = (br, 5306, 300, 56)
    bq = mg._corpus_net(7, [0], {(0, 1): 1.0, (1, 2): 0.5, (1, 3): 0.5, (2, 4): 1.0, (2, 5): 1.0, (3, 6): 1.0}, {},
                        {1: 2, 2: 2, 3: 1, 4: 0, 5: 0, 6: 0})
    bq["distributions"] = [["exponential", 0.4], ["branch"], ["queue"], ["queue"], ["exponential", 1.0],
                           ["exponential", 1.5], ["exponential", 0.6]]
    C["branch_queue"] = (bq, 5307, 300, 57)
    mx = mg._corpus_net(5, [0], {(0, 1): 1.0, (1, 2): 1.0, (1, 3): 1.0, (1, 4): 1.0}, {}, {1: 2, 2: 0, 3: 0, 4: 0})
    mx["distributions"] = [["uniform", 0.125, 0.5], ["queue"], ["normal", 1.0, 0.25], ["uniform", 0.5, 1.0],
                           ["exponential", 1.0]]
    C["mixed"] = (mx, 5308, 300, 58)
    dt = mg._corpus_net(4, [0], {(0, 1): 1.0, (1, 2): 1.0, (1, 3): 1.0}, {}, {1: 2, 2: 0, 3: 0})
    dt["distributions"] = [["uniform", 1.0, 0.0], ["queue"], ["uniform", 2.5, 0.0], ["uniform", 3.0, 0.0]]
    C["det_tie"] = (dt, 5309, 120, 59)
    sq = mg._corpus_net(3, [0], {(0, 1): 0.5, (0, 2): 0.5, (1, 0): 1.0}, {}, 2)
    sq["distributions"] = [["exponential", 0.5], ["queue"], ["exponential", 0.75]]
    C["sink_quirk"] = (sq, 5310, 150, 60)
    C["embed16"] = (embed(S, 16, 716, 5316, 300, 61), 5316, 300, 61)
    C["embed128"] = (embed(S, 128, 828, 5428, 250, 62), 5428, 250, 62)
    rz = mg._corpus_net(4, [0, 3], {(0, 1): 1.0, (1, 2): 0.5, (1, 3): 0.5, (3, 2): 1.0}, {}, 2)
    rz["distributions"] = [["exponential", 0.5], ["branch"], ["exponential", 0.25], ["exponential", 2.0]]
    C["raises"] = (rz, 5311, 100, 63)
    return C


def parse(dist):
    kind = [KINDS.index(d[0]) for d in dist]
    loc = [float(d[1]) if d[0] in ("normal", "uniform") else 0.0 for d in dist]
    scale = [float(d[1]) if d[0] == "exponential" else float(d[2]) if d[0] in ("normal", "uniform") else 0.0
             for d in dist]
    return np.array(kind, dtype=np.int32), np.array(loc), np.array(scale)


def run_reference(S, spec, seed, customers, log):
    """One Sim.run in a scratch directory with the witnesses counted around the reference's own methods -> (sim or the
    exception, records, witnesses)."""
    w = {"delayed": 0, "redelayed": 0, "popped": 0}
    cwd = os.getcwd()
    dequeue = S.EventList.dequeue

    def counting_dequeue(self):
        w["popped"] += 1
        return dequeue(self)

    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs("logs")
        S.EventList.dequeue = counting_dequeue
        try:
            for h in list(logging.root.handlers):
                logging.root.removeHandler(h)
            sim = S.Sim(spec["sim_matrix"].copy(), spec["distributions"], list(spec["queue_list"]), seeds=[seed],
                        log_path="logs/", generate_log=log, animation=False, record_history=False,
                        logging_mode='Music', max_sim_time=1e9)
            inner, last = sim.schedule_delayed_departure, {}

            def counting_delay(server_id, event_id, new_time):
                w["delayed"] += 1
                if last.get(server_id) == (event_id, sim.Clock):
                    w["redelayed"] += 1
                last[server_id] = (event_id, new_time)
                return inner(server_id, event_id, new_time)

            sim.schedule_delayed_departure = counting_delay
            try:
                sim.run(number_of_customers=customers)
                result = sim
            except Exception as e:      # noqa: BLE001 -- the recording is of whatever the reference raises
                result = e
            logging.shutdown()
            recs = []
            if log:
                for ln in open("logs/simulation.log"):
                    m = LINE.match(ln.strip())
                    if m:
                        recs.append((float(m.group(1)), int(m.group(2)), int(m.group(3)), REC_KINDS.index(m.group(4)),
                                     m.group(1)))
        finally:
            S.EventList.dequeue = dequeue
            os.chdir(cwd)
    return result, recs, w


def main():
    S = mg.load_reference("MMGAN_MIDI_DES", "simulation_v3")
    out, names = {}, []
    for name, (spec, seed, customers, np_seed) in cases(S).items():
        dim = len(spec["queue_list"])
        k = max(1, int(max(spec["queue_list"]))) + 1            # one column more: queue + delayed departure
        assert customers <= 400
        np.random.seed(np_seed)
        sim, recs, w = run_reference(S, spec, seed, customers, True)
        state = np.random.get_state()
        names.append(name)
        kind, loc, scale = parse(spec["distributions"])
        out[f"{name}/sim_matrix"], out[f"{name}/kind"] = spec["sim_matrix"], kind
        out[f"{name}/loc"], out[f"{name}/scale"] = loc, scale
        out[f"{name}/queue_list"] = np.array(spec["queue_list"], dtype=np.int32)
        out[f"{name}/seed"], out[f"{name}/customers"] = np.int64(seed), np.int64(customers)
        out[f"{name}/np_seed"] = np.int64(np_seed)
        if isinstance(sim, Exception):
            out[f"{name}/exception"] = np.array(type(sim).__name__)
            print(f"{name:12s} dim {dim:3d} raises {type(sim).__name__}({sim})")
            continue
        for key, v in mdd.accumulators(sim, dim, k).items():
            out[f"{name}/{key}"] = v
        assert all(len(o.queue_length_times) <= k + 1 and max(o.queue_length_times) <= k for o in sim.servers.values())
        out[f"{name}/value"] = np.array([r[0] for r in recs], dtype=np.float64)
        out[f"{name}/event_id"] = np.array([r[1] for r in recs], dtype=np.int64)
        out[f"{name}/node"] = np.array([r[2] for r in recs], dtype=np.int32)
        out[f"{name}/rec_kind"] = np.array([r[3] for r in recs], dtype=np.int32)
        # the reference writes the service time of a queue or branch node as the int 0
        assert all((r[4] == "0") == (kind[r[2]] >= 3) for r in recs if r[3] == 2), name
        out[f"{name}/final_key"] = np.asarray(state[1], dtype=np.uint32)
        out[f"{name}/final_pos"], out[f"{name}/final_has_gauss"] = np.int64(state[2]), np.int64(state[3])
        out[f"{name}/final_gauss"] = np.float64(state[4])
        for key, v in w.items():
            out[f"{name}/{key}"] = np.int64(v)
        print(f"{name:12s} dim {dim:3d} kinds {np.bincount(kind, minlength=5)} records {len(recs):5d} popped "
              f"{w['popped']:5d} delayed {w['delayed']:4d} redelayed {w['redelayed']:3d} clock {sim.Clock:9.4f} reneges "
              f"{int(out[f'{name}/reneges'].sum()):3d} max_queue {int(out[f'{name}/max_queue'].max())}")
    out["names"] = np.array(names)
    # witnesses of what the cases exist for
    for name in ("mm2_cap2", "cap0", "c1", "c4", "shared", "branch_queue", "mixed", "det_tie", "embed16", "embed128"):
        assert out[f"{name}/delayed"] > 0, name
    assert out["det_tie/redelayed"] > 0
    assert out["cap0/max_queue"].max() == 0 and out["cap0/queue_time"][1, 1] > 0 and out["cap0/reneges"][1] > 0
    assert out["sink_quirk/delayed"] == 0 and out["sink_quirk/served"][1] > 0
    assert out["branch37/delayed"] == 0 and out["branch37/served"][2] > 0 and out["branch37/served"][3] > 0
    assert out["shared/max_queue"][4] > 0
    assert str(out["raises/exception"]) == "KeyError"
    # simultaneous events exist in det_tie; elsewhere no two distinct times of a log are nearly equal
    t = out["det_tie/value"][out["det_tie/rec_kind"] == 0]
    assert len(np.unique(t)) < len(t)

    # ---- the validation grid
    cmax = max(g[0] for g in GRID)
    kmax = max(max(g[3], 1) for g in GRID)
    fields = ("served", "reneges", "max_queue", "generated", "time_in_service", "time_in_queue", "queue_area",
              "arrival_time", "clock", "end_time", "total_customers", "queue_time")
    grid = {f: [] for f in fields + ("popped",)}
    worst = 0.0
    for c, lam, mu, cap in GRID:
        spec = station(c, lam, mu, cap)
        runs = []
        for seed in GRID_SEEDS:
            np.random.set_state(np.random.RandomState([seed, 1]).get_state())
            sim, _recs, w = run_reference(S, spec, seed, GRID_CUSTOMERS, False)
            a = mdd.accumulators(sim, c + 2, kmax)
            runs.append(a)
            for f in fields:
                v = np.asarray(a[f])
                pad = np.zeros((cmax + 2,) + v.shape[1:], dtype=v.dtype) if v.ndim else v
                if v.ndim:
                    pad[:c + 2] = v
                grid[f].append(pad)
            grid["popped"].append(w["popped"])
        th = qt.mmck(lam, mu, c, max(cap, 1))
        sim_q = {"blocked_fraction": [a["reneges"][1] / (a["served"][1] + a["reneges"][1]) for a in runs],
                 "utilisation": [(a["time_in_service"][2:] / a["clock"]).mean() for a in runs],
                 "avg_queue_length": [a["queue_area"][1] / a["clock"] for a in runs],
                 "avg_queue_time": [a["time_in_queue"][1] / a["served"][1] for a in runs]}
        want = {"blocked_fraction": th["blocking"], "utilisation": th["utilisation"], "avg_queue_length": th["LQ"],
                "avg_queue_time": th["WQ"]}
        for j in range(max(cap, 1) + 1):
            sim_q[f"P(waiting={j})"] = [a["queue_time"][1, j] / a["clock"] for a in runs]
            want[f"P(waiting={j})"] = th["queue_length_probabilities"][j]
        for q, v in sim_q.items():
            v = np.array(v, dtype=np.float64)
            sem = v.std(ddof=1) / np.sqrt(len(v))
            z = (v.mean() - want[q]) / sem
            print(f"c {c} lam {lam} mu {mu} cap {cap} {q:18s} sim {v.mean():.5f} +- {sem:.5f} theory {want[q]:.5f} "
                  f"z {z:+.2f}")
            assert abs(z) <= Z_BOUND, ("replace this configuration", c, lam, mu, cap, q, z)
            worst = max(worst, abs(z))
    for f in grid:
        out[f"grid/{f}"] = np.array(grid[f])
    out["grid/config"] = np.array(GRID, dtype=np.float64)
    out["grid/seeds"] = np.array(GRID_SEEDS, dtype=np.int64)
    out["grid/customers"] = np.int64(GRID_CUSTOMERS)
    out["grid/max_abs_z"] = np.float64(worst)
    print("largest |z| on the grid:", worst)
    path = os.path.join(HERE, "des_net.npz")
    mg._write_npz_reproducibly(path, out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes,", len(names), "cases")
    assert size < SIZE_BOUND, "fewer customers per case"


if __name__ == "__main__":
    main()
