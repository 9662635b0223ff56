#!/usr/bin/env python3
"""Generate tests/golden/des_stats.npz: the queueing statistics of the REFERENCE's own ``Sim`` on the corpus of
des_corpus.npz (build container only; needs /root/reference like make_golden.py, whose ``load_reference`` and
``_corpus_cases`` this imports -- nothing of the reference's text is copied).

Run from the repo root:   python tests/golden/make_des_stats_golden.py

Every good case of the catalogue is run ('Music' mode, as the corpus was recorded) from its recorded starting state of
numpy's global stream; a case with several seeds with its FIRST seed only (the convention of test_des_corpus.py's
``case_arrays``).  Stored per case, all read from the reference's objects after ``Sim.run``:

  served, time_in_service, reneges, max_queue, time_in_queue   (dim)  the Server attributes total_customers_served,
        total_time_in_service, reneges, max_queue_length, total_time_in_queue; 0 on a source row
  arrival_time, generated                                       (dim)  Source.arrival_times, customers_generated; 0 on a
        server row
  is_source (dim), clock = Sim.Clock, end_time = Sim.previous_time, total_customers, n_records = lines of the log
  queue_time (dim, K + 1), K = max(1, max(queue_list)): Server.queue_length_times as a dense array (a length the
        server never had: 0), and queue_area (dim) = sum(length * time) over its items in the dict's order
  m_<name> for the names of ``calculate_metrics`` (752-801), where Clock != 0 (the method raises ZeroDivisionError
        otherwise; has_metrics says which): the method stores nothing with record_history off, so its expressions are
        evaluated here on the reference's objects -- never on this project's code -- into (dim) arrays with NaN where
        the reference's dict has no key, queue_length_probabilities (dim, K + 1) with NaN rows for sources, and the
        five totals as scalars.

For single-seed cases the number of log lines must equal the corpus recording's.
"""
import logging
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg   # noqa: E402


def reference_metrics(sim, dim, k):
    """The expressions of calculate_metrics (756-771, 797-801) on the reference's objects."""
    sv, so, clock = sim.servers, sim.sources, sim.Clock
    d = {}
    d["avg_time_at_server"] = {s: (sv[s].total_time_in_service + sv[s].total_time_in_queue) / sv[s].total_customers_served
                               for s in sv if sv[s].total_customers_served > 0}
    d["avg_queue_time"] = {s: sv[s].total_time_in_queue / sv[s].total_customers_served
                           for s in sv if sv[s].total_customers_served > 0}
    d["server_utilizations"] = {s: sv[s].total_time_in_service / clock for s in sv}
    d["max_queue_lengths"] = {s: sv[s].max_queue_length for s in sv}
    d["renege_rate"] = {s: sv[s].reneges / sv[s].total_customers_served for s in sv if sv[s].total_customers_served > 0}
    d["service_times"] = {s: sv[s].total_time_in_service / sv[s].total_customers_served
                          for s in sv if sv[s].total_customers_served > 0}
    d["arrival_times"] = {s: so[s].arrival_times / so[s].customers_generated for s in so}
    d["customers_served_per_server"] = {s: sv[s].total_customers_served for s in sv}
    d["avg_queue_length"] = {s: sum([length * time for length, time in sv[s].queue_length_times.items()]) / clock
                             for s in sv}
    d["avg_server_length"] = {s: d["avg_queue_length"][s] + d["server_utilizations"][s] for s in sv}
    out = {}
    for name, values in d.items():
        a = np.full(dim, np.nan)
        for s, v in values.items():
            a[s] = float(v)
        out[name] = a
    prob = np.full((dim, k + 1), np.nan)
    for s in sv:
        prob[s] = 0.0
        for length, time in sv[s].queue_length_times.items():
            prob[s, length] = time / clock
    out["queue_length_probabilities"] = prob
    out["total_U"] = np.float64(sum(d["server_utilizations"].values()))
    out["total_L"] = np.float64(sum(d["avg_queue_length"].values()) + sum(d["server_utilizations"].values()))
    out["total_LQ"] = np.float64(sum(d["avg_queue_length"].values()))
    out["total_W"] = np.float64(sum(d["avg_time_at_server"].values()) + sum(d["avg_queue_time"].values()))
    out["total_WQ"] = np.float64(sum(d["avg_queue_time"].values()))
    return out


def main():
    S = mg.load_reference("MMGAN_MIDI_DES", "simulation_v3")
    corpus = np.load(os.path.join(HERE, "des_corpus.npz"))
    line_re = re.compile(r"INFO:root:(\S+) - (\S+) - (\S+) - (arrival|departure|processing)$")
    out, names = {}, []
    for name, (spec, seeds, customers, np_seed, pre_normal, _want) in mg._corpus_cases().items():
        if str(corpus[f"{name}/error"]):
            continue
        dim = len(spec["queue_list"])
        k = max(1, int(max(spec["queue_list"])))
        np.random.seed(np_seed)
        if pre_normal:
            np.random.standard_normal(pre_normal)
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            os.makedirs("logs")
            try:
                for h in list(logging.root.handlers):
                    logging.root.removeHandler(h)
                sim = S.Sim(spec["sim_matrix"].copy(), spec["distributions"], list(spec["queue_list"]), seeds=seeds[:1],
                            log_path="logs/", generate_log=True, animation=False, record_history=False,
                            logging_mode='Music', max_sim_time=1e9)
                sim.run(number_of_customers=customers)
                n_records = sum(1 for ln in open("logs/simulation.log") if line_re.match(ln.strip()))
            finally:
                os.chdir(cwd)
        if len(seeds) == 1:
            assert n_records == len(corpus[f"{name}/value"]), (name, n_records, len(corpus[f"{name}/value"]))
        names.append(name)
        sv, so = sim.servers, sim.sources

        def rows(objs, attr, dtype):
            a = np.zeros(dim, dtype=dtype)
            for i, o in objs.items():
                a[i] = getattr(o, attr)
            return a

        pre = name
        out[f"{pre}/served"] = rows(sv, "total_customers_served", np.int64)
        out[f"{pre}/time_in_service"] = rows(sv, "total_time_in_service", np.float64)
        out[f"{pre}/reneges"] = rows(sv, "reneges", np.int64)
        out[f"{pre}/max_queue"] = rows(sv, "max_queue_length", np.int32)
        out[f"{pre}/time_in_queue"] = rows(sv, "total_time_in_queue", np.float64)
        out[f"{pre}/arrival_time"] = rows(so, "arrival_times", np.float64)
        out[f"{pre}/generated"] = rows(so, "customers_generated", np.int64)
        out[f"{pre}/is_source"] = np.array([i in so for i in range(dim)], dtype=np.bool_)
        out[f"{pre}/clock"] = np.float64(sim.Clock)
        out[f"{pre}/end_time"] = np.float64(sim.previous_time)
        out[f"{pre}/total_customers"] = np.int64(sim.total_customers)
        out[f"{pre}/n_records"] = np.int64(n_records)
        qt, area = np.zeros((dim, k + 1)), np.zeros(dim)
        for i, o in sv.items():
            for length, time in o.queue_length_times.items():
                qt[i, length] = time
            area[i] = sum([length * time for length, time in o.queue_length_times.items()])
        out[f"{pre}/queue_time"], out[f"{pre}/queue_area"] = qt, area
        has = sim.Clock != 0
        out[f"{pre}/has_metrics"] = np.bool_(has)
        if has:
            for key, v in reference_metrics(sim, dim, k).items():
                out[f"{pre}/m_{key}"] = v
        print(f"{name:22s} dim {dim:3d} records {n_records:5d} clock {sim.Clock:9.4f} end {sim.previous_time:9.4f} "
              f"served {int(out[f'{pre}/served'].sum()):4d} reneges {int(out[f'{pre}/reneges'].sum()):3d} "
              f"metrics {bool(has)}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "des_stats.npz")
    mg._write_npz_reproducibly(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
