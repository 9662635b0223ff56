#!/usr/bin/env python3
"""Generate tests/golden/des_log_dist.npz: the 'Music' LOGS of the REFERENCE's own ``Sim`` on the nets of
make_des_dist_golden.py (nodes 'normal', 'exponential' or 'uniform'), and what the reference's notebook
MMGAN_MIDI_DES/simlog_to_vid.ipynb makes of them (needs the reference checkout, like the other generators; ``cases``
and ``parse`` are make_des_dist_golden.py's, ``load_reference`` make_golden.py's -- nothing of the reference's text is
copied: the notebook's cells are read from its JSON and executed).

Run from the repo root:   python tests/golden/make_des_log_dist_golden.py

Per case of ``cases()``, run exactly as make_des_dist_golden.py runs it ('Music' mode, ``np.random.seed(np_seed)``, one
seed; the line count is asserted to be des_dist.npz's ``n_records``):
  <name>/value f64, event_id i64, node i32, kind i32   the log's records (kind: the index into KIND_NAMES)
  <name>/final_pos, final_key_sha256                   numpy's global stream after the run: position, SHA-256 of the key
  <name>/servers, tracks          i32, i16             cell 0's ``process_adjsim_log(servers)`` on that log file for
                                                       servers = sorted(sim.servers)
  <name>/servers_perm, tracks_perm                     ... and for one seeded permutation of them
The inputs of a case are des_dist.npz's (same names).

``random_net`` recordings for RANDOM_NET_SEEDS: ``np.random.seed(seed)``, then cell 1's source up to, not including,
the line that imports ``Sim``:
  net<seed>/matrix, servers, sinks, distributions (dim, 2: the two numbers behind 'exponential'), seeds,
  net<seed>/final_pos, final_key_sha256
"""
import hashlib
import json
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
from make_des_dist_golden import cases, parse  # noqa: E402

KIND_NAMES = ("arrival", "departure", "processing")
RANDOM_NET_SEEDS = (0, 1, 2)
LINE = re.compile(r"INFO:root:(\S+) - (\S+) - (\S+) - (arrival|departure|processing)$")
SIZE_BOUND = 525657                           # des_corpus.npz


def notebook_cells():
    with open(os.path.join(mg.REF, "MMGAN_MIDI_DES", "simlog_to_vid.ipynb")) as f:
        nb = json.load(f)
    return ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]


def key_sha(state):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(state[1], dtype="<u4").tobytes()).digest(), dtype=np.uint8)


def run_case(S, cell0, spec, seed, customers, np_seed, perm_seed):
    """One Sim.run in a scratch directory, then the notebook's cell on the log it wrote."""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs("logs")
        try:
            for h in list(logging.root.handlers):
                logging.root.removeHandler(h)
            np.random.seed(np_seed)
            sim = S.Sim(spec["sim_matrix"].copy(), spec["distributions"], list(spec["queue_list"]), seeds=[seed],
                        log_path="logs/", generate_log=True, animation=False, record_history=False,
                        logging_mode='Music', max_sim_time=1e9)
            sim.run(number_of_customers=customers)
            state = np.random.get_state()
            logging.shutdown()
            recs = []
            for ln in open("logs/simulation.log"):
                m = LINE.match(ln.strip())
                if m:
                    recs.append((float(m.group(1)), int(m.group(2)), int(m.group(3)), KIND_NAMES.index(m.group(4))))
            ns = {}
            exec(compile(cell0, "simlog_to_vid.ipynb[0]", "exec"), ns)
            servers = sorted(int(s) for s in sim.servers)
            perm = [servers[i] for i in np.random.RandomState(perm_seed).permutation(len(servers))]
            tracks = ns["process_adjsim_log"](servers)
            tracks_perm = ns["process_adjsim_log"](perm)
        finally:
            os.chdir(cwd)
    return recs, state, servers, tracks, perm, tracks_perm


def main():
    S = mg.load_reference("MMGAN_MIDI_DES", "simulation_v3")
    cells = notebook_cells()
    dist = np.load(os.path.join(HERE, "des_dist.npz"))
    out, names, total = {}, [], 0
    for idx, (name, (spec, seed, customers, np_seed)) in enumerate(cases().items()):
        recs, state, servers, tracks, perm, tracks_perm = run_case(S, cells[0], spec, seed, customers, np_seed,
                                                                   1000 + idx)
        assert len(recs) == int(dist[f"{name}/n_records"]), (name, len(recs))
        kind, _loc, _scale = parse(spec["distributions"])
        assert np.array_equal(kind, dist[f"{name}/kind"]), name
        names.append(name)
        total += len(recs)
        out[f"{name}/value"] = np.array([r[0] for r in recs], dtype=np.float64)
        out[f"{name}/event_id"] = np.array([r[1] for r in recs], dtype=np.int64)
        out[f"{name}/node"] = np.array([r[2] for r in recs], dtype=np.int32)
        out[f"{name}/kind"] = np.array([r[3] for r in recs], dtype=np.int32)
        out[f"{name}/final_pos"] = np.int64(state[2])
        out[f"{name}/final_key_sha256"] = key_sha(state)
        for tag, sv_, tr in (("", servers, tracks), ("_perm", perm, tracks_perm)):
            tr = np.asarray(tr)
            assert tr.ndim == 2 and tr.shape[1] == len(sv_) and np.abs(tr).max() < 2 ** 15, (name, tr.shape)
            out[f"{name}/servers{tag}"] = np.array(sv_, dtype=np.int32)
            out[f"{name}/tracks{tag}"] = tr.astype(np.int16)
        # the clock of no line prints in exponent notation (the notebook's expression would drop it)
        assert not any("e" in repr(r[0]) for r in recs if r[3] != 2), name
        print(f"{name:12s} records {len(recs):5d} tracks {tracks.shape} max {int(tracks.max())}")
    out["names"] = np.array(names)
    print("records in total:", total)

    cut = cells[1].split("from simulation_v3 import Sim")[0]
    for seed in RANDOM_NET_SEEDS:
        np.random.seed(seed)
        ns = {"np": np}
        exec(compile(cut, "simlog_to_vid.ipynb[1]", "exec"), ns)
        state = np.random.get_state()
        out[f"net{seed}/matrix"] = np.asarray(ns["matrix"], dtype=np.float64)
        out[f"net{seed}/servers"] = np.asarray(ns["servers"], dtype=np.int64)
        out[f"net{seed}/sinks"] = np.asarray(ns["sinks"], dtype=np.int64)
        out[f"net{seed}/distributions"] = np.array([[d[1], d[2]] for d in ns["distributions"]], dtype=np.float64)
        out[f"net{seed}/seeds"] = np.asarray(ns["seeds"], dtype=np.int64)
        out[f"net{seed}/final_pos"] = np.int64(state[2])
        out[f"net{seed}/final_key_sha256"] = key_sha(state)
        assert all(d[0] == "exponential" for d in ns["distributions"]) and ns["queue_lengths"] == [330] * 20
    out["net_seeds"] = np.array(RANDOM_NET_SEEDS, dtype=np.int64)
    path = os.path.join(HERE, "des_log_dist.npz")
    mg._write_npz_reproducibly(path, out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes,", len(names), "cases")
    assert size < SIZE_BOUND, "keep the first 1500 records and a SHA-256 of all of them for the rand* cases"


if __name__ == "__main__":
    main()
