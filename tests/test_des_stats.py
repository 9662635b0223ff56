"""The log-free statistics mode of the batched simulator (gdm_des_stats_batch_host; csrc/des_sim.h with the null sink
and the NodeStats policy) against tests/golden/des_stats.npz: the accumulators of the REFERENCE's own Server / Source
objects after Sim.run on the 43 good cases of the corpus of des_corpus.npz, recorded by
tests/golden/make_des_stats_golden.py (a two-seed case with its first seed only).  Runs without a GPU.

  1. math=0 (libm, numpy's bits), cases of one dim stacked into one batch, in file order and shuffled: counts, stop
     reasons and total_customers equal; time_in_service, time_in_queue, arrival_time, clock and end_time -- the same
     operations in the reference's order -- equal bit for bit; queue_area and queue_time, integrated when a queue
     changes instead of on every event, within BOUND_LAZY * max(1, |x|).  Measured against the recording on this
     corpus: 4.79e-16 (queue_area, draw_backwards; queue_time: 2.15e-16, size_128), bound 10 x that = 4.79e-15.
  2. math=1 (portable, what the device runs): integers and stop reasons equal; the deterministic (tie) cases bit-equal
     in the event-order floats; the rest within 10 x the worst measured ratio: event-order floats 1.87e-16
     (time_in_service, size_17) -> 1.87e-15; lazily integrated ones 4.79e-16 (queue_area, draw_backwards; queue_time
     3.99e-16, route_interleave) -> 4.79e-15.  test_des_corpus.py's bound for the records is 2.13e-15.
  3. against the log of the same run (run_batch_host, math=1, uncapped): record counts, stop reasons, final states
     (of the samples that did not error: those keep their state here), served = the node's 'processing' records,
     time_in_service = their sequential sum, clock = the last arrival / departure record.
  4. invariants: the histogram's row sums are end_time, its first moment is queue_area; histogram=False changes no
     other output.
  5. metrics() against the recorded calculate_metrics values, same NaN pattern; Clock == 0 gives NaN, not an exception.
  6. the two error cases inside a batch: reason 3, zeros, generator state untouched, neighbours equal their recording.
  7. replicate() on a dim-5 net with 8 seeds.
  8. host validation of the device entry (no launch: safe without a GPU).
  9. tools/des_stats_host.cpp, the same header as a stand-alone program with exactly sized buffers, built with the
     host compiler's address and undefined-behaviour sanitizers and run as a child process."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import _lib, matrix_sim_process as msp, ops, simulation_v3 as sv
from helpers import load_golden
from test_des_corpus import (DETERMINISTIC, DIMS, ERRORS, G, GOOD, NAMES, case_arrays, names_of_dim, same_state, state0)

S = load_golden("des_stats.npz")
REL_LAZY = 4.79e-16             # max |lazy - recording| / max(1, |recording|), math=0 (queue_area, draw_backwards)
BOUND_LAZY = 10 * REL_LAZY
REL_PORTABLE = 1.87e-16         # math=1, the floats accumulated in event order (time_in_service, size_17)
BOUND_PORTABLE = 10 * REL_PORTABLE
REL_PORTABLE_LAZY = 4.79e-16    # math=1, queue_area / queue_time (queue_area, draw_backwards)
BOUND_PORTABLE_LAZY = 10 * REL_PORTABLE_LAZY
INTS = ("served", "reneges", "max_queue", "generated")
EVENT_ORDER = ("time_in_service", "time_in_queue", "arrival_time", "clock", "end_time")
ERROR = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ratio(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if want.size else 0.0


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def sample(st, b):
    """Sample b of a host BatchStats as a dict (the histogram cut to nothing when there is none)."""
    d = {f: np.asarray(getattr(st, f)[b]) for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("is_source",)}
    d["queue_time"] = None if st.queue_time is None else st.queue_time[b]
    d["state"] = sv.state_of(st, b)
    return d


def batches(math, shuffled):
    """name -> sample dict, the corpus stacked by dim (histogram on), in file order or shuffled."""
    out, rs = {}, np.random.RandomState(23)
    for dim in DIMS:
        names = names_of_dim(dim)
        if shuffled and len(names) > 1:
            names = [names[i] for i in rs.permutation(len(names))] + [names[0]]
        st = sv.run_stats_host(*case_arrays(names), math=math, histogram=True)
        for b, n in enumerate(names):
            out[n] = cut(sample(st, b), n)
    return out


def cut(d, name):
    """The histogram of a sample from a stacked batch (as wide as the batch's largest capacity) cut to the case's own
    K + 1 columns, K = max(1, its largest capacity): a queue cannot have been longer."""
    k = max(1, int(G[f"{name}/queue_list"].max())) + 1
    assert not d["queue_time"][:, k:].any(), name
    d["queue_time"] = d["queue_time"][:, :k]
    return d


@pytest.fixture(scope="module")
def runs():
    return {(m, sh): batches(m, sh) for m in (0, 1) for sh in (False, True)}


def check_structure(name, got):
    for f in INTS:
        assert np.array_equal(got[f], S[f"{name}/{f}"]), (name, f)
    assert got["total_customers"] == S[f"{name}/total_customers"] and got["n_records"] == S[f"{name}/n_records"], name
    assert np.array_equal(got["is_source"], S[f"{name}/is_source"]), name
    assert got["stop_reason"] == (1 if S[f"{name}/is_source"].any() else 0), name
    k = S[f"{name}/queue_time"].shape[1]
    assert got["queue_time"].shape[1] == k == max(1, int(G[f"{name}/queue_list"].max())) + 1


# ---- 1. libm: the reference's bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", GOOD)
def test_libm_statistics_are_the_recording(runs, name, shuffled):
    got = runs[0, shuffled][name]
    check_structure(name, got)
    for f in EVENT_ORDER:
        assert bits(got[f]) == bits(S[f"{name}/{f}"]), (name, f, got[f], S[f"{name}/{f}"])
    for f in ("queue_area", "queue_time"):
        r = ratio(got[f], S[f"{name}/{f}"])
        print(name, f, "max |lazy - recording| / max(1, |x|):", r)
        assert r <= BOUND_LAZY <= 1e-12, (name, f)


def test_the_measured_lazy_ratio_is_the_documented_one(runs):
    worst = max((ratio(runs[0, False][n][f], S[f"{n}/{f}"]), n, f) for n in GOOD for f in ("queue_area", "queue_time"))
    print("worst lazy / recording ratio:", worst)
    assert worst[0] <= 2 * REL_LAZY and BOUND_LAZY <= 1e-12


# ---- 2. portable math: what the device runs --------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", GOOD)
def test_portable_statistics(runs, name, shuffled):
    got = runs[1, shuffled][name]
    check_structure(name, got)
    assert same_state(got["state"], runs[0, shuffled][name]["state"])
    for f in EVENT_ORDER:
        r = ratio(got[f], S[f"{name}/{f}"])
        print(name, f, "max |portable - recording| / max(1, |x|):", r)
        if name in DETERMINISTIC:
            assert bits(got[f]) == bits(S[f"{name}/{f}"]), (name, f)
        else:
            assert r <= BOUND_PORTABLE, (name, f)
    for f in ("queue_area", "queue_time"):
        r = ratio(got[f], S[f"{name}/{f}"])
        print(name, f, "max |portable, lazy - recording| / max(1, |x|):", r)
        assert r <= BOUND_PORTABLE_LAZY <= 1e-12, (name, f)


def test_the_measured_portable_ratios_are_the_documented_ones(runs):
    worst = max((ratio(runs[1, False][n][f], S[f"{n}/{f}"]), n, f) for n in GOOD for f in EVENT_ORDER)
    lazy = max((ratio(runs[1, False][n][f], S[f"{n}/{f}"]), n, f) for n in GOOD for f in ("queue_area", "queue_time"))
    print("worst portable / recording ratios:", worst, lazy)
    assert len(DETERMINISTIC) >= 5 and worst[0] <= 2 * REL_PORTABLE and lazy[0] <= 2 * REL_PORTABLE_LAZY


# ---- 3. against the log of the same run ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_statistics_against_the_log_of_the_same_run(dim):
    names = names_of_dim(dim)
    a = case_arrays(names)
    st = sv.run_stats_host(*a, math=1)
    log = sv.run_batch_host(*a, math=1, max_records=0)
    assert np.array_equal(st.n_records, log.n_records) and np.array_equal(st.stop_reason, log.stop_reason)
    for b, n in enumerate(names):
        if n in ERRORS:                                   # (the logging entries hand back the advanced state)
            assert st.stop_reason[b] == ERROR and same_state(sv.state_of(st, b), state0(n))
            continue
        assert same_state(sv.state_of(st, b), sv.state_of(log, b)), n
        recs = sv.sample_log(log, b)
        proc = recs[recs["kind"] == sv.PROCESSING]
        for i in range(dim):
            mine = proc["value"][proc["node"] == i]
            assert st.served[b, i] == len(mine), (n, i)
            total = functools.reduce(lambda x, y: x + y, mine.tolist(), 0.0)
            assert bits(np.float64(total)) == bits(st.time_in_service[b, i]), (n, i)
        moves = recs[recs["kind"] != sv.PROCESSING]
        if len(moves):
            assert bits(st.clock[b]) == bits(moves["value"][-1]), n
        else:
            assert st.clock[b] == 0.0, n


# ---- 4. invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [0, 1])
def test_histogram_invariants(runs, math):
    for n in GOOD:
        got = runs[math, False][n]
        server = ~got["is_source"]
        qt = got["queue_time"]
        k = np.arange(qt.shape[1], dtype=np.float64)
        end = float(got["end_time"])
        assert (np.abs(qt[server].sum(axis=1) - end) <= BOUND_LAZY * max(1.0, abs(end))).all(), n
        assert not qt[~server].any() and not got["queue_area"][~server].any(), n
        area = got["queue_area"][server]
        assert (np.abs((qt[server] * k).sum(axis=1) - area) <= BOUND_LAZY * np.maximum(1.0, np.abs(area))).all(), n


@pytest.mark.parametrize("dim", [5, 17])
def test_histogram_off_changes_nothing_else(dim):
    a = case_arrays(names_of_dim(dim))
    on, off = sv.run_stats_host(*a, math=1, histogram=True), sv.run_stats_host(*a, math=1, histogram=False)
    assert off.queue_time is None and on.queue_time is not None
    for f in on._fields:
        if f != "queue_time":
            assert bits(getattr(on, f)) == bits(getattr(off, f)), f


# ---- 5. derived metrics ----------------------------------------------------------------------------------------------
RATIO_NAMES = ("avg_time_at_server", "avg_queue_time", "server_utilizations", "renege_rate", "service_times",
               "arrival_times", "avg_queue_length", "avg_server_length")


TOTAL_TERMS = {"total_U": ("server_utilizations",), "total_L": ("avg_queue_length", "server_utilizations"),
               "total_LQ": ("avg_queue_length",), "total_W": ("avg_time_at_server", "avg_queue_time"),
               "total_WQ": ("avg_queue_time",)}                    # simulation_v3.py:797-801


@pytest.mark.parametrize("math,bound", [(0, BOUND_LAZY), (1, BOUND_PORTABLE_LAZY)])
def test_metrics_against_the_recorded_calculate_metrics(math, bound):
    """One division (or one sum of two quotients) after the accumulators: a quotient moves by its operands' relative
    deviations (at most `bound` each, numerator and denominator) plus one rounding, so 3 x bound relative to
    max(1, |x|).  A total is a sum of n such terms, added here in another order than the reference's left-to-right
    sum(): 3 x bound x sum(max(1, |term|)) for the terms plus n x 2^-52 x sum(|term|) for the order."""
    assert sorted(sv.METRIC_NAMES) == sorted(RATIO_NAMES + ("max_queue_lengths", "customers_served_per_server"))
    seen = 0
    for dim in DIMS:
        names = [n for n in names_of_dim(dim) if n in GOOD]
        m = sv.metrics(sv.run_stats_host(*case_arrays(names), math=math, histogram=True))
        for b, n in enumerate(names):
            if not bool(S[f"{n}/has_metrics"]):
                continue
            seen += 1
            for name in sv.METRIC_NAMES + ("queue_length_probabilities",):
                got, want = m[name][b], S[f"{n}/m_{name}"]
                if name == "queue_length_probabilities":          # (the batch's histogram is as wide as its widest case)
                    assert not np.nan_to_num(got[:, want.shape[1]:]).any(), n
                    got = got[:, :want.shape[1]]
                assert got.dtype == np.float64 and got.shape == want.shape, (n, name)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (n, name)
                ok = ~np.isnan(want)
                if name in ("max_queue_lengths", "customers_served_per_server"):
                    assert np.array_equal(got[ok], want[ok]), (n, name)
                else:
                    assert ratio(got[ok], want[ok]) <= 3 * bound, (n, name, ratio(got[ok], want[ok]))
            for name, parts in TOTAL_TERMS.items():
                got, want = float(m[name][b]), float(S[f"{n}/m_{name}"])
                terms = np.concatenate([S[f"{n}/m_{p}"] for p in parts])
                terms = np.abs(terms[~np.isnan(terms)])
                tol = 3 * bound * np.maximum(1.0, terms).sum() + len(terms) * 2.3e-16 * terms.sum()
                assert abs(got - want) <= tol, (n, name, got, want, tol)
    assert seen == 38


def test_metrics_where_the_clock_never_moved():
    """stop_n0, stop_n1, stop_n2: customers were generated, nothing was processed -- calculate_metrics divides by
    Clock == 0 (ZeroDivisionError upstream); stop_nosrc, size_1: no customers at all (it returns early)."""
    zero = [n for n in GOOD if not bool(S[f"{n}/has_metrics"])]
    assert sorted(zero) == ["size_1", "stop_n0", "stop_n1", "stop_n2", "stop_nosrc"]
    raising = [n for n in zero if int(S[f"{n}/total_customers"]) > 0]
    assert raising == ["stop_n0", "stop_n1", "stop_n2"] and all(float(S[f"{n}/clock"]) == 0.0 for n in zero)
    st = sv.run_stats_host(*case_arrays(raising), math=1, histogram=True)
    m = sv.metrics(st)
    assert (st.clock == 0).all() and (st.end_time > 0).all()
    for name in ("server_utilizations", "avg_queue_length", "avg_server_length", "total_U", "total_L", "total_LQ"):
        assert np.isnan(m[name]).all(), name
    assert np.isnan(m["queue_length_probabilities"]).all()
    src = st.is_source
    assert not np.isnan(m["arrival_times"][src]).any() and np.isnan(m["arrival_times"][~src]).all()
    assert np.isnan(m["avg_queue_time"]).all() and (m["total_W"] == 0).all() and (m["total_WQ"] == 0).all()
    assert (m["max_queue_lengths"][~src] == 0).all() and (m["customers_served_per_server"][~src] == 0).all()


# ---- 6. errors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [0, 1])
def test_error_cases_inside_a_batch(runs, math):
    names = ["q_cap1", "err_to_source", "stop_n4", "err_source_childless", "tie_a"]
    assert set(names[1::2]) == set(ERRORS) <= set(NAMES)
    st = sv.run_stats_host(*case_arrays(names), math=math, histogram=True)
    assert st.stop_reason.tolist() == [1, ERROR, 1, ERROR, 1]
    for b in (1, 3):
        for f in sv.STATS_NODE_FIELDS + ("clock", "end_time", "total_customers", "events", "n_records"):
            assert not np.asarray(getattr(st, f)[b]).any(), (names[b], f)
        assert not st.queue_time[b].any()
        assert same_state(sv.state_of(st, b), state0(names[b])), names[b]
    for b in (0, 2, 4):
        want = runs[math, False][names[b]]
        got = cut(sample(st, b), names[b])
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("queue_time",):
            assert bits(got[f]) == bits(want[f]), (names[b], f)
        assert same_state(got["state"], want["state"])


# ---- 7. replications -------------------------------------------------------------------------------------------------
def corpus_spec(n):
    dim = len(G[f"{n}/queue_list"])
    return msp.DesSpec(G[f"{n}/sim_matrix"], [["normal", a, b] for a, b in G[f"{n}/dist"]], list(G[f"{n}/queue_list"]),
                       np.array([0]), int(G[f"{n}/customers"]), 1.0, np.zeros(dim), np.zeros(dim))


def test_replicate_is_r_single_runs_summarised():
    n, seeds = "q_wrap3", [11, 12, 13, 14, 15, 16, 17, 2 ** 32 - 1]
    rep = sv.replicate(corpus_spec(n), seeds)
    assert rep.valid.all() and len(seeds) == 8
    one = case_arrays([n])
    for r, seed in enumerate(seeds):
        state = np.random.RandomState([seed, 1]).get_state()
        single = sv.run_stats_host(*one[:4], [seed], one[5], [state], math=1)
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
            assert bits(getattr(single, f)[0]) == bits(getattr(rep.stats, f)[r]), (r, f)
        assert same_state(sv.state_of(single, 0), sv.state_of(rep.stats, r))
    assert len({float(c) for c in rep.stats.clock}) == 8
    m = sv.metrics(rep.stats)
    for name in sv.METRIC_NAMES + sv.TOTAL_NAMES:
        a = m[name]
        count = (~np.isnan(a)).sum(axis=0)
        assert np.array_equal(rep.n[name], count), name
        full = count == 8
        cols = a[:, full] if a.ndim == 2 else a
        want_mean, want_std = cols.mean(axis=0), cols.std(axis=0, ddof=1)
        pick = (lambda x: x[full]) if a.ndim == 2 else (lambda x: x)
        np.testing.assert_allclose(pick(rep.mean[name]), want_mean, rtol=1e-13, atol=0)
        np.testing.assert_allclose(pick(rep.std[name]), want_std, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(pick(rep.sem[name]), want_std / np.sqrt(8), rtol=1e-9, atol=1e-15)
        if a.ndim == 2:
            assert np.isnan(rep.mean[name][count == 0]).all() and np.isnan(rep.std[name][count < 2]).all()
    # a replication that errors is left out of every summary
    bad = sv.replicate(corpus_spec("err_to_source"), [1, 2, 3])
    assert not bad.valid.any() and (bad.n["server_utilizations"] == 0).all() and np.isnan(bad.mean["total_U"])


def test_run_stats_takes_specs():
    specs = [corpus_spec("q_wrap3"), corpus_spec("q_cap0")]
    states = [state0("q_wrap3"), state0("q_cap0")]
    for sp, n in zip(specs, ("q_wrap3", "q_cap0")):
        sp.seeds = G[f"{n}/seeds"][:1]
    st = sv.run_stats(specs, states=states)
    want = sv.run_stats_host(*case_arrays(["q_wrap3", "q_cap0"]), math=1)
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert bits(getattr(st, f)) == bits(getattr(want, f)), f


# ---- 8. host validation of the device entry --------------------------------------------------------------------------
def test_device_entry_validates_on_the_host():
    lib = _lib.load()
    b, dim, cap = 2, 5, 4
    need = lib.gdm_des_stats_workspace_bytes(b, dim, cap)
    assert need == lib.gdm_des_batch_workspace_bytes(b, dim, cap) + b * ((dim * cap * 8 + 15) // 16 * 16)
    assert lib.gdm_des_stats_workspace_bytes(b, 129, cap) == -1 and lib.gdm_des_stats_workspace_bytes(b, dim, 0) == -1
    assert lib.gdm_des_stats_workspace_bytes(0, dim, cap) == -1 and lib.gdm_des_stats_workspace_bytes(b, dim, 65537) == -1
    # host memory stands in for the arrays: every call below is refused before anything is launched
    buf = np.zeros(need + 64, dtype=np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    arrays = [np.zeros(4096, dtype=np.float64) for _ in range(27)]
    ptrs = [a.ctypes.data for a in arrays]

    def call(dim=dim, cap=cap, ptrs=ptrs, hist=None, ws=base, ws_bytes=need, max_events=1000):
        args = [ptrs[0], b, dim, *ptrs[1:6], cap, max_events, *ptrs[6:24], hist, ws, ws_bytes, None]
        return lib.gdm_des_stats_batch(*args), lib.gdm_last_error()

    for missing in (0, 3, 9, 10, 17, 23):
        rc, msg = call(ptrs=[None if i == missing else p for i, p in enumerate(ptrs)])
        assert rc == -1 and b"null pointer" in msg, missing
    rc, msg = call(ws=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc == -1 and b"workspace" in msg
    rc, msg = call(ws=base + 8)
    assert rc == -1 and b"workspace" in msg
    rc, msg = call(dim=129)
    assert rc == -1 and b"dim" in msg
    rc, msg = call(cap=0)
    assert rc == -1 and b"max_queue_cap" in msg
    rc, msg = call(max_events=0)
    assert rc == -1 and b"max_events" in msg
    rc, msg = call(ptrs=[ptrs[0] + 4] + ptrs[1:])
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(hist=ptrs[24] + 2)
    assert rc == -1 and b"aligned" in msg
    # the host entry: the same checks, no workspace
    rc = lib.gdm_des_stats_batch_host(*([None] * 1), b, dim, *ptrs[1:6], cap, 1, 1000, *ptrs[6:24], None)
    assert rc == -1 and b"null pointer" in lib.gdm_last_error()
    rc = lib.gdm_des_stats_batch_host(ptrs[0], b, dim, *ptrs[1:6], cap, 2, 1000, *ptrs[6:24], None)
    assert rc == -1 and b"math" in lib.gdm_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    z = torch.zeros
    with pytest.raises(ops.GdmError):
        ops.des_run_stats(z(1, 2, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64),
                          z(1, 2, dtype=torch.int32), z(1, dtype=torch.int64), z(1, dtype=torch.int64),
                          z(1, 624, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.int32),
                          z(1, dtype=torch.float64), max_queue_cap=4)


def test_existing_refusals_stay():
    with pytest.raises(NotImplementedError):
        sv.Sim(np.eye(2), [["normal", 1, 1]] * 2, [1, 1], seeds=[1], logging_mode='Music', record_history=True)


# ---- 9. the same header as a stand-alone program under the host sanitizers -------------------------------------------
def stand_alone_cases():
    """(label, adj, loc, scale, qcap, seed, customers, state): a wrapping ring, capacity 0, a run-time error, and a spec
    the batch entries refuse before anything runs (a negative scale)."""
    out = []
    for n in ("q_wrap3", "q_cap0", "err_to_source", "q_cap1"):
        adj, loc, scale, qcap, seed, cust, states = case_arrays([n])
        if n == "q_cap1":
            scale = scale.copy()
            scale[0, 3] = -1.0
            n = "refused"
        out.append((n, adj[0], loc[0], scale[0], qcap[0].astype(np.int32), int(seed[0]), int(cust[0]), states[0]))
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of tools/des_stats_host.cpp "
                    "did not run")
    cases = stand_alone_cases()
    exe, cases_bin, stats_bin = str(tmp_path / "des_stats_host"), str(tmp_path / "cases.bin"), str(tmp_path / "stats.bin")
    with open(cases_bin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _n, adj, loc, scale, qcap, seed, cust, st in cases:
            f.write(struct.pack("<iiiiqqqd", adj.shape[0], int(st[3]), int(st[2]), 0, seed, cust, 200000, float(st[4])))
            for a, dt in ((adj, "<f8"), (loc, "<f8"), (scale, "<f8"), (qcap, "<i4"), (st[1], "<u4")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            *static, "-I", os.path.join(ROOT, "gan_des_midi_music_gen_amd", "csrc"),
                            os.path.join(ROOT, "tools", "des_stats_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases_bin, stats_bin], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    with open(stats_bin, "rb") as f:
        for n, adj, loc, scale, qcap, seed, cust, st in cases:
            dim = adj.shape[0]
            want = sv.run_stats_host(adj[None], loc[None], scale[None], qcap[None], [seed], [cust], [st], math=1,
                                     histogram=True)
            reason, has, pos, stride, total, events, n_rec, gauss, clock, end = struct.unpack("<iiiiqqqddd", f.read(64))
            assert stride == int(qcap.max()) and reason == want.stop_reason[0], n
            assert (total, events, n_rec) == (want.total_customers[0], want.events[0], want.n_records[0]), n
            assert bits(np.float64(clock)) == bits(want.clock[0]) and bits(np.float64(end)) == bits(want.end_time[0]), n
            for field, dt in (("served", "<i8"), ("reneges", "<i8"), ("generated", "<i8"), ("max_queue", "<i4"),
                              ("time_in_service", "<f8"), ("time_in_queue", "<f8"), ("queue_area", "<f8"),
                              ("arrival_time", "<f8")):
                got = np.frombuffer(f.read(np.dtype(dt).itemsize * dim), dtype=dt)
                assert bits(got) == bits(getattr(want, field)[0]), (n, field)
            qt = np.frombuffer(f.read(8 * dim * (stride + 1)), dtype="<f8").reshape(dim, stride + 1)
            assert bits(qt) == bits(want.queue_time[0][:, :stride + 1]) and not want.queue_time[0][:, stride + 1:].any(), n
            key = np.frombuffer(f.read(4 * 624), dtype="<u4")
            assert same_state(("MT19937", key, pos, has, gauss), sv.state_of(want, 0)), n
            if n in ("refused", "err_to_source"):
                assert reason == ERROR and same_state(sv.state_of(want, 0), st) and not want.served.any(), n
            else:
                assert reason == 1 and want.served.sum() > 50, n
        assert f.read() == b""
    assert int(cases[0][4].max()) == 3 and int(G["q_wrap3/w_from_queue"].max()) >= 20 and cases[1][4][3] == 0
