#!/usr/bin/env python3
"""Generate tests/golden/des_dist.npz: the REFERENCE's own ``Sim`` on nets whose nodes are 'normal', 'exponential' or
'uniform' (needs the reference checkout, like make_golden.py, whose ``load_reference``, ``_corpus_net`` and
``_corpus_random_net`` this imports, and make_des_stats_golden.py's ``reference_metrics`` -- nothing of the reference's
text is copied).

Run from the repo root:   python tests/golden/make_des_dist_golden.py

1. A corpus (``names``): small nets of at most 400 customers, each run in 'Music' mode from ``np.random.seed(np_seed)``
   with one seed.  Stored per case: the inputs -- sim_matrix, kind (the index into simulation_v3.DIST_KINDS), loc, scale
   (float64; an exponential's loc is 0), queue_list, seed, customers, np_seed -- and, read from the reference's objects
   after ``Sim.run``, exactly the fields des_stats.npz stores (make_des_stats_golden.py's docstring).

     exp2, uni2        all-exponential / all-uniform source -> server
     mix5, mix6        the three kinds in one net
     rand15 .. rand128 seeded random nets (_corpus_random_net) at dims 15, 16, 17, 64, 128, every node's kind a seeded
                       draw; a node keeps its mean: exponential(mean), uniform(mean - std, 2 std) clipped at 0.01
     uni_neg           uniforms whose support starts below zero: inter-arrival times that go BACK in time and service
                       times that are drawn again (``while service <= 0``)
     scale0_src        an exponential source with scale 0 (every customer at time 0, Clock stays 0) and a uniform
                       server with scale 0 (deterministic)
     scale0_srv        a uniform source with scale 0 (a fixed period) in front of an exponential server that fills and
                       reneges; a source keeps the one destination it drew at the start, so its other child, a
                       deterministic uniform server, stays idle in this run
     renege            arrivals three times as fast as service, one waiting place: the queue fills, customers renege

2. The validation grid (``grid/...``): GRID, six M/M/1/K configurations (rho 0.5, 0.8, 1.0, 1.5; capacities 1..5) x
   GRID_SEEDS x 4000 customers on the net source -> server, each run from the global stream
   ``RandomState([seed, 1])`` (simulation_v3.replication_states).  Stored per run (configuration-major) the
   accumulators of the server and the source.  The generator ASSERTS that for every compared quantity (blocked fraction
   = reneges / (served + reneges), utilisation, mean queue length, mean queue time, queue-length probabilities) the
   reference's mean over the 16 seeds lies within 4 standard errors of ``queueing_theory.mm1k``; the largest |z| is
   stored as ``grid/max_abs_z``.  A configuration that fails is to be REPLACED, never the bound.
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
import make_des_stats_golden as msg           # noqa: E402
from gan_des_midi_music_gen_amd import queueing_theory as qt   # noqa: E402

KINDS = ("normal", "exponential", "uniform")
GRID = ((0.5, 1.0, 1), (0.8, 1.0, 3), (1.0, 1.0, 5), (1.5, 1.0, 2), (1.6, 2.0, 4), (0.75, 0.5, 5))   # lam, mu, cap
GRID_SEEDS = tuple(101 + 7 * i for i in range(16))
GRID_CUSTOMERS = 4000
Z_BOUND = 4.0


def f32(x):
    return float(np.float32(x))


def with_kinds(spec, kinds):
    """A _corpus_net spec (all 'normal') with node i's distribution replaced by kind kinds[i] of the same mean."""
    dist = []
    for (_n, m, s), k in zip(spec["distributions"], kinds):
        m, s = float(m), float(s)
        if k == 0:
            dist.append(["normal", m, s])
        elif k == 1:
            dist.append(["exponential", m])
        else:
            lo = max(f32(m - s), 0.01)
            dist.append(["uniform", lo, f32(2 * s)])
    return {"sim_matrix": spec["sim_matrix"], "distributions": dist, "queue_list": spec["queue_list"]}


def cases():
    """name -> (spec, seed, customers, np_seed)."""
    C = {}
    two = {(0, 1): 1.0}
    C["exp2"] = (with_kinds(mg._corpus_net(2, [0], two, {0: (1.0, 0.0), 1: (0.8, 0.0)}, 3), [1, 1]), 4242, 300, 31)
    uni = mg._corpus_net(2, [0], two, {}, 2)
    uni["distributions"] = [["uniform", 0.5, 1.0], ["uniform", 0.25, 1.0]]
    C["uni2"] = (uni, 4243, 300, 32)
    f5 = {(0, 2): 0.5, (0, 3): 0.5, (1, 3): 1.0, (2, 4): 0.25, (2, 3): 0.75, (3, 4): 1.0}
    p5 = {0: (0.75, 0.25), 1: (1.0, 0.5), 2: (0.5, 0.125), 3: (0.25, 0.125), 4: (0.25, 0.0625)}
    C["mix5"] = (with_kinds(mg._corpus_net(5, [0, 1], f5, p5, {2: 2, 3: 3, 4: 1}), [1, 2, 0, 1, 2]), 4244, 300, 33)
    f6 = {(0, 3): 1.0, (1, 3): 0.5, (1, 4): 0.5, (2, 4): 1.0, (3, 5): 0.25, (3, 4): 0.75, (4, 5): 1.0}
    p6 = {0: (1.0, 0.25), 1: (1.5, 0.5), 2: (2.0, 0.5), 3: (0.25, 0.125), 4: (0.5, 0.25), 5: (0.25, 0.125)}
    C["mix6"] = (with_kinds(mg._corpus_net(6, [0, 1, 2], f6, p6, {3: 2, 4: 1, 5: 4}), [2, 0, 1, 1, 2, 0]), 4245, 300, 34)
    for dim in (15, 16, 17, 64, 128):
        spec, _src = mg._corpus_random_net(dim, 700 + dim)
        kinds = np.random.RandomState(900 + dim).randint(0, 3, size=dim)
        assert len(set(kinds.tolist())) == 3
        C[f"rand{dim}"] = (with_kinds(spec, kinds), 5000 + dim, 400 if dim < 64 else 300, 40 + dim % 7)
    neg = mg._corpus_net(3, [0], {(0, 1): 1.0, (1, 2): 1.0}, {}, 3)
    neg["distributions"] = [["uniform", -0.25, 1.5], ["uniform", -0.5, 1.25], ["uniform", -0.125, 0.5]]
    C["uni_neg"] = (neg, 4246, 300, 35)
    z1 = mg._corpus_net(3, [0], {(0, 1): 1.0, (1, 2): 1.0}, {}, 2)
    z1["distributions"] = [["exponential", 0.0], ["uniform", 0.5, 0.0], ["exponential", 0.25]]
    C["scale0_src"] = (z1, 4247, 60, 36)
    z2 = mg._corpus_net(3, [0], {(0, 1): 0.5, (0, 2): 0.5}, {}, 2)
    z2["distributions"] = [["uniform", 0.25, 0.0], ["uniform", 0.375, 0.0], ["exponential", 0.5]]
    C["scale0_srv"] = (z2, 4248, 200, 37)
    rn = mg._corpus_net(2, [0], two, {}, 1)
    rn["distributions"] = [["exponential", f32(1.0 / 3.0)], ["exponential", 1.0]]
    C["renege"] = (rn, 4249, 300, 38)
    return C


def parse(dist):
    kind = [KINDS.index(d[0]) for d in dist]
    loc = [0.0 if d[0] == "exponential" else float(d[1]) for d in dist]
    scale = [float(d[1]) if d[0] == "exponential" else float(d[2]) for d in dist]
    return np.array(kind, dtype=np.int32), np.array(loc), np.array(scale)


def accumulators(sim, dim, k):
    """The reference's objects after Sim.run as the arrays des_stats.npz stores."""
    sv, so = sim.servers, sim.sources

    def rows(objs, attr, dtype):
        a = np.zeros(dim, dtype=dtype)
        for i, o in objs.items():
            a[i] = getattr(o, attr)
        return a

    out = {"served": rows(sv, "total_customers_served", np.int64),
           "time_in_service": rows(sv, "total_time_in_service", np.float64),
           "reneges": rows(sv, "reneges", np.int64), "max_queue": rows(sv, "max_queue_length", np.int32),
           "time_in_queue": rows(sv, "total_time_in_queue", np.float64),
           "arrival_time": rows(so, "arrival_times", np.float64), "generated": rows(so, "customers_generated", np.int64),
           "is_source": np.array([i in so for i in range(dim)], dtype=np.bool_), "clock": np.float64(sim.Clock),
           "end_time": np.float64(sim.previous_time), "total_customers": np.int64(sim.total_customers)}
    qt_, area = np.zeros((dim, k + 1)), np.zeros(dim)
    for i, o in sv.items():
        for length, time in o.queue_length_times.items():
            qt_[i, length] = time
        area[i] = sum([length * time for length, time in o.queue_length_times.items()])
    out["queue_time"], out["queue_area"] = qt_, area
    return out


def run_reference(S, spec, seed, customers, log):
    """One Sim.run in a scratch directory -> (sim, number of 'Music' log lines or None)."""
    line_re = re.compile(r"INFO:root:(\S+) - (\S+) - (\S+) - (arrival|departure|processing)$")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs("logs")
        try:
            for h in list(logging.root.handlers):
                logging.root.removeHandler(h)
            sim = S.Sim(spec["sim_matrix"].copy(), spec["distributions"], list(spec["queue_list"]), seeds=[seed],
                        log_path="logs/", generate_log=log, animation=False, record_history=False,
                        logging_mode='Music', max_sim_time=1e9)
            sim.run(number_of_customers=customers)
            n = sum(1 for ln in open("logs/simulation.log") if line_re.match(ln.strip())) if log else None
        finally:
            os.chdir(cwd)
    return sim, n


def main():
    S = mg.load_reference("MMGAN_MIDI_DES", "simulation_v3")
    out, names = {}, []
    for name, (spec, seed, customers, np_seed) in cases().items():
        dim = len(spec["queue_list"])
        k = max(1, int(max(spec["queue_list"])))
        assert customers <= 400
        np.random.seed(np_seed)
        sim, n_records = run_reference(S, spec, seed, customers, True)
        names.append(name)
        kind, loc, scale = parse(spec["distributions"])
        out[f"{name}/sim_matrix"], out[f"{name}/kind"] = spec["sim_matrix"], kind
        out[f"{name}/loc"], out[f"{name}/scale"] = loc, scale
        out[f"{name}/queue_list"] = np.array(spec["queue_list"], dtype=np.int32)
        out[f"{name}/seed"], out[f"{name}/customers"] = np.int64(seed), np.int64(customers)
        out[f"{name}/np_seed"] = np.int64(np_seed)
        for key, v in accumulators(sim, dim, k).items():
            out[f"{name}/{key}"] = v
        out[f"{name}/n_records"] = np.int64(n_records)
        has = sim.Clock != 0
        out[f"{name}/has_metrics"] = np.bool_(has)
        if has:
            for key, v in msg.reference_metrics(sim, dim, k).items():
                out[f"{name}/m_{key}"] = v
        print(f"{name:12s} dim {dim:3d} kinds {np.bincount(kind, minlength=3)} records {n_records:5d} clock "
              f"{sim.Clock:9.4f} end {sim.previous_time:9.4f} served {int(out[f'{name}/served'].sum()):4d} reneges "
              f"{int(out[f'{name}/reneges'].sum()):3d} max_queue {int(out[f'{name}/max_queue'].max())}")
    out["names"] = np.array(names)
    # witnesses of what the cases exist for
    assert out["renege/reneges"].sum() > 50 and out["renege/max_queue"].max() == 1
    assert out["uni_neg/arrival_time"][0] > 0 and float(out["scale0_src/clock"]) == 0.0

    # ---- the validation grid
    kmax = max(c for _l, _m, c in GRID)
    fields = ("served", "reneges", "max_queue", "generated", "time_in_service", "time_in_queue", "queue_area",
              "arrival_time", "clock", "end_time", "total_customers", "queue_time")
    grid = {f: [] for f in fields}
    worst = 0.0
    for lam, mu, cap in GRID:
        spec = {"sim_matrix": np.array([[1.0, 1.0], [0.0, 0.0]]),
                "distributions": [["exponential", 1.0 / lam], ["exponential", 1.0 / mu]], "queue_list": [cap, cap]}
        runs = []
        for seed in GRID_SEEDS:
            np.random.set_state(np.random.RandomState([seed, 1]).get_state())
            sim, _ = run_reference(S, spec, seed, GRID_CUSTOMERS, False)
            a = accumulators(sim, 2, kmax)
            runs.append(a)
            for f in fields:
                grid[f].append(a[f])
        th = qt.mm1k(lam, mu, cap)
        sim_q = {"blocked_fraction": [a["reneges"][1] / (a["served"][1] + a["reneges"][1]) for a in runs],
                 "utilisation": [a["time_in_service"][1] / a["clock"] for a in runs],
                 "avg_queue_length": [a["queue_area"][1] / a["clock"] for a in runs],
                 "avg_queue_time": [a["time_in_queue"][1] / a["served"][1] for a in runs]}
        want = {"blocked_fraction": th["blocking"], "utilisation": th["utilisation"], "avg_queue_length": th["LQ"],
                "avg_queue_time": th["WQ"]}
        for j in range(cap + 1):
            sim_q[f"P(queue={j})"] = [a["queue_time"][1, j] / a["clock"] for a in runs]
            want[f"P(queue={j})"] = th["queue_length_probabilities"][j]
        for q, v in sim_q.items():
            v = np.array(v, dtype=np.float64)
            sem = v.std(ddof=1) / np.sqrt(len(v))
            z = (v.mean() - want[q]) / sem
            print(f"lam {lam} mu {mu} cap {cap} {q:18s} sim {v.mean():.5f} +- {sem:.5f} theory {want[q]:.5f} z {z:+.2f}")
            assert abs(z) <= Z_BOUND, ("replace this configuration", lam, mu, cap, q, z)
            worst = max(worst, abs(z))
    for f in fields:
        out[f"grid/{f}"] = np.array(grid[f])
    out["grid/config"] = np.array(GRID, dtype=np.float64)
    out["grid/seeds"] = np.array(GRID_SEEDS, dtype=np.int64)
    out["grid/customers"] = np.int64(GRID_CUSTOMERS)
    out["grid/max_abs_z"] = np.float64(worst)
    print("largest |z| on the grid:", worst)
    path = os.path.join(HERE, "des_dist.npz")
    mg._write_npz_reproducibly(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
