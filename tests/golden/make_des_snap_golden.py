#!/usr/bin/env python3
"""Generate tests/golden/des_snap.npz: the REFERENCE's own ``Sim`` run ONCE PER CHECKPOINT (needs the reference checkout,
like make_des_dist_golden.py, whose ``cases``, ``run_reference`` and ``accumulators`` this imports, and
make_des_net_golden.py's ``cases`` and ``parse`` -- nothing of the reference's text is copied).

Run from the repo root:   python tests/golden/make_des_snap_golden.py

``number_of_customers`` enters the reference only in its stop test, so its run of n1 customers is a prefix of its run of
n2 > n1 customers under the same seeds: what the simulator's snapshot at checkpoint n must hold is the final state of the
reference's run of n customers.

1. A corpus (``names``): six nets reused from des_dist.npz and des_net.npz -- mix5 (the three distribution kinds),
   rand17 (a seeded random net of 17 nodes), mm2_cap2 (a queue node in front of two servers), branch_queue (a branch node
   in front of two queue nodes), renege (the queue fills, customers renege) and uni_neg (time runs back) -- each run from
   ``np.random.seed(np_seed)`` with one seed at every checkpoint of CHECKPOINTS: values at or below the number of sources
   (all of them fire at the first pop), two consecutive values, and a last one of at most 400 customers.  Stored per
   case: the inputs (kind: the index into simulation_v3.NODE_KINDS) and the fields of des_dist.npz with a leading S.
   queue_time has one column more than the largest capacity asks for: a queue node's delayed departure counts.

2. The validation grid with a warm-up (``grid/...``): make_des_dist_golden.py's GRID x GRID_SEEDS on the net source ->
   server, each seed run twice from the global stream ``RandomState([seed, 1])``: GRID_WARMUP customers (``grid/w_*``)
   and GRID_CUSTOMERS customers (``grid/c_*``).  The statistics of the window between the two are the differences.  The
   generator ASSERTS that for every compared quantity the windowed mean over the 16 seeds lies within 4 standard errors
   of ``queueing_theory.mm1k``; the largest |z| with the warm-up is stored as ``grid/max_abs_z``, the one of the whole
   runs as ``grid/max_abs_z_full``.  A configuration that fails is to be REPLACED, never the bound.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg                      # noqa: E402
import make_des_dist_golden as mdd            # noqa: E402
import make_des_net_golden as mdn             # noqa: E402
from gan_des_midi_music_gen_amd import queueing_theory as qt   # noqa: E402

CHECKPOINTS = (1, 2, 50, 51, 137, 300)
FROM_DIST = ("mix5", "rand17", "renege", "uni_neg")
FROM_NET = ("mm2_cap2", "branch_queue")
GRID_WARMUP = 1000
FIELDS = ("served", "reneges", "max_queue", "generated", "time_in_service", "time_in_queue", "queue_area",
          "arrival_time", "clock", "end_time", "total_customers", "queue_time")


def window_quantities(lo, hi, cap):
    """The compared quantities of the server node between two recordings of one run (lo None: from the empty start)."""
    def d(f):
        return hi[f] - (lo[f] if lo is not None else 0)

    clock = d("clock")
    q = {"blocked_fraction": d("reneges")[1] / (d("served")[1] + d("reneges")[1]),
         "utilisation": d("time_in_service")[1] / clock, "avg_queue_length": d("queue_area")[1] / clock,
         "avg_queue_time": d("time_in_queue")[1] / d("served")[1]}
    for j in range(cap + 1):
        q[f"P(queue={j})"] = d("queue_time")[1, j] / clock
    return q


def main():
    S = mg.load_reference("MMGAN_MIDI_DES", "simulation_v3")
    dist_cases, net_cases = mdd.cases(), mdn.cases(S)
    out, names = {}, []
    for name in FROM_DIST + FROM_NET:
        spec, seed, customers, np_seed = (dist_cases if name in FROM_DIST else net_cases)[name]
        dim = len(spec["queue_list"])
        k = max(1, int(max(spec["queue_list"]))) + 1
        assert CHECKPOINTS[-1] <= customers <= 400
        n_sources = int((np.diagonal(spec["sim_matrix"]) > 0).sum())
        assert CHECKPOINTS[0] <= n_sources and any(b == a + 1 for a, b in zip(CHECKPOINTS, CHECKPOINTS[1:]))
        rows = []
        for n in CHECKPOINTS:
            np.random.seed(np_seed)
            sim, _ = mdd.run_reference(S, spec, seed, n, False)
            rows.append(mdd.accumulators(sim, dim, k))
        names.append(name)
        kind, loc, scale = mdn.parse(spec["distributions"])
        out[f"{name}/sim_matrix"], out[f"{name}/kind"] = spec["sim_matrix"], kind
        out[f"{name}/loc"], out[f"{name}/scale"] = loc, scale
        out[f"{name}/queue_list"] = np.array(spec["queue_list"], dtype=np.int32)
        out[f"{name}/seed"], out[f"{name}/np_seed"] = np.int64(seed), np.int64(np_seed)
        out[f"{name}/checkpoints"] = np.array(CHECKPOINTS, dtype=np.int64)
        for f in FIELDS + ("is_source",):
            out[f"{name}/{f}"] = np.stack([r[f] for r in rows])
        print(f"{name:13s} dim {dim:3d} sources {n_sources} clock " + " ".join(f"{float(r['clock']):8.3f}" for r in rows) +
              " served " + " ".join(f"{int(r['served'].sum()):4d}" for r in rows))
        # a prefix: nothing shrinks but where time runs back
        assert all((b["served"] >= a["served"]).all() for a, b in zip(rows, rows[1:])), name
    out["names"] = np.array(names)

    # ---- the validation grid, with and without the warm-up
    kmax = max(c for _l, _m, c in mdd.GRID)
    grid = {p + f: [] for p in ("w_", "c_") for f in FIELDS}
    worst = {"window": 0.0, "full": 0.0}
    for lam, mu, cap in mdd.GRID:
        spec = {"sim_matrix": np.array([[1.0, 1.0], [0.0, 0.0]]),
                "distributions": [["exponential", 1.0 / lam], ["exponential", 1.0 / mu]], "queue_list": [cap, cap]}
        runs = []
        for seed in mdd.GRID_SEEDS:
            pair = []
            for p, n in (("w_", GRID_WARMUP), ("c_", mdd.GRID_CUSTOMERS)):
                np.random.set_state(np.random.RandomState([seed, 1]).get_state())
                sim, _ = mdd.run_reference(S, spec, seed, n, False)
                a = mdd.accumulators(sim, 2, kmax)
                pair.append(a)
                for f in FIELDS:
                    grid[p + f].append(a[f])
            runs.append(pair)
        th = qt.mm1k(lam, mu, cap)
        want = {"blocked_fraction": th["blocking"], "utilisation": th["utilisation"], "avg_queue_length": th["LQ"],
                "avg_queue_time": th["WQ"]}
        for j in range(cap + 1):
            want[f"P(queue={j})"] = th["queue_length_probabilities"][j]
        for label in ("window", "full"):
            per_run = [window_quantities(w if label == "window" else None, c, cap) for w, c in runs]
            for q in want:
                v = np.array([r[q] for r in per_run], dtype=np.float64)
                sem = v.std(ddof=1) / np.sqrt(len(v))
                z = (v.mean() - want[q]) / sem
                print(f"lam {lam} mu {mu} cap {cap} {label:6s} {q:18s} sim {v.mean():.5f} +- {sem:.5f} theory "
                      f"{want[q]:.5f} z {z:+.2f}")
                assert abs(z) <= mdd.Z_BOUND, ("replace this configuration", lam, mu, cap, label, q, z)
                worst[label] = max(worst[label], abs(z))
    for f, v in grid.items():
        out[f"grid/{f}"] = np.array(v)
    out["grid/config"] = np.array(mdd.GRID, dtype=np.float64)
    out["grid/seeds"] = np.array(mdd.GRID_SEEDS, dtype=np.int64)
    out["grid/customers"], out["grid/warmup"] = np.int64(mdd.GRID_CUSTOMERS), np.int64(GRID_WARMUP)
    out["grid/max_abs_z"], out["grid/max_abs_z_full"] = np.float64(worst["window"]), np.float64(worst["full"])
    print("largest |z| on the grid: with the warm-up", worst["window"], "whole runs", worst["full"])
    path = os.path.join(HERE, "des_snap.npz")
    mg._write_npz_reproducibly(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
