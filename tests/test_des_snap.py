"""Snapshots of the statistics run at customer counts (des::SnapStats in csrc/des_sim.h, behind
gdm_des_stats_batch_snap_host) and what is built on them: snapshot, window, convergence, batch_means and warmup=.
Runs without a GPU.

  1. against the REFERENCE (tests/golden/des_snap.npz, recorded by tests/golden/make_des_snap_golden.py: the reference's
     own Sim run once per checkpoint from the same seeds, six nets): with math=0 snapshot s is the reference's run of n_s
     customers -- counts, stop reasons and total_customers equal; time_in_service, time_in_queue, arrival_time, clock and
     end_time bit-equal; queue_area and queue_time within test_des_stats.py's BOUND_LAZY.
  2. the invariant: every snapshot is run_stats_host(customers = n_s) byte for byte, every field and the histogram,
     both maths, on the corpora of des_dist.npz and des_net.npz stacked per dim (the net the reference raises on among
     them: the checkpoints before the error are the shorter runs', the rest zeros and reason 3); a batch cut by a small
     max_events, refused samples, a sample that ends on the draw budget; per-sample rows that differ.  The generator
     state after the run is that of the run to the last checkpoint.
  3. the surface: window, convergence and batch_means against float64 numpy restatements; warmup=0 returns the arrays
     of today's functions through today's entries; warmup > 0 is the window; the argument checks of the entry; with a
     device nothing falls back to the host quietly.
  4. warm-up beside theory: mm1k_sweep(warmup=, math=0) reproduces the recorded reference runs (two per seed: warmup and
     customers) to the equalities of 1. (BOUND_LAZY; measured 4.40e-15, queue_area), and every |z| <= 4 -- the
     recording's own largest |z|, 1.67 with the warm-up beside 1.64 without.
  5. tools/des_snap_host.cpp, the policy as a stand-alone program under the host compiler's sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import _lib, simulation_v3 as sv
from helpers import load_golden
from test_des_corpus import same_state
from test_des_dist import DIMS as DIST_DIMS, Z_BOUND, check_z, dist_case_arrays, dist_names_of_dim
from test_des_net import DIMS as NET_DIMS, names_of_dim as net_names_of_dim, net_case_arrays, refused_dist_batch
from test_des_stats import BOUND_LAZY, EVENT_ORDER, INTS, ROOT, bits, ratio

G = load_golden("des_snap.npz")
NAMES = [str(n) for n in G["names"]]
ERROR, BUDGET, EVENTS, CUSTOMERS = 3, 5, 2, 1
CHECKPOINTS = (1, 2, 3, 50, 51, 137, 300)               # the invariant's: fire together, consecutive, a long way apart
FIELDS = sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("queue_time",)
STATE = ("mt_key", "mt_pos", "has_gauss", "gauss")


def golden_arrays(name):
    return ((G[f"{name}/sim_matrix"][None], G[f"{name}/loc"][None], G[f"{name}/scale"][None],
             G[f"{name}/queue_list"][None], [int(G[f"{name}/seed"])]), G[f"{name}/kind"][None],
            [np.random.RandomState(int(G[f"{name}/np_seed"])).get_state()])


# ---- 1. against the reference ----------------------------------------------------------------------------------------
def test_the_recording_covers_what_it_was_made_for():
    assert NAMES == ["mix5", "rand17", "renege", "uni_neg", "mm2_cap2", "branch_queue"]
    for n in NAMES:
        cp = G[f"{n}/checkpoints"].tolist()
        sources = int(G[f"{n}/is_source"][0].sum())
        assert cp == [1, 2, 50, 51, 137, 300] and cp[0] <= sources and cp[-1] <= 400, n
        assert not G[f"{n}/clock"][0] and G[f"{n}/served"][-1].sum() > 50, n       # nothing processed at the first pop
    assert G["mix5/is_source"][0].sum() == 2 and not G["mix5/clock"][1]            # two checkpoints at one pop
    assert G["rand17/sim_matrix"].shape == (17, 17) and set(G["mix5/kind"].tolist()) == {0, 1, 2}
    assert 3 in G["mm2_cap2/kind"] and {3, 4} <= set(G["branch_queue/kind"].tolist())
    assert G["renege/reneges"][-1].sum() > 50 and (np.diff(G["uni_neg/end_time"]) != 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_libm_snapshots_are_the_references_shorter_runs(name):
    a, kind, states = golden_arrays(name)
    sn = sv.run_stats_snapshots_host(*a, G[f"{name}/checkpoints"], states, math=0, histogram=True, kind=kind)
    assert sn.stop.tolist() == [[CUSTOMERS] * 6] and sn.checkpoints.tolist() == [G[f"{name}/checkpoints"].tolist()]
    k = sn.snaps.queue_time.shape[-1]
    assert not G[f"{name}/queue_time"][:, :, k:].any(), name
    for s in range(6):
        got = sv.snapshot(sn, s)
        for f in INTS + ("total_customers",):
            assert np.array_equal(getattr(got, f)[0], G[f"{name}/{f}"][s]), (name, s, f)
        assert np.array_equal(got.is_source[0], G[f"{name}/is_source"][s]), (name, s)
        for f in EVENT_ORDER:
            assert bits(getattr(got, f)[0]) == bits(G[f"{name}/{f}"][s]), (name, s, f)
        for f, want in (("queue_area", G[f"{name}/queue_area"][s]), ("queue_time", G[f"{name}/queue_time"][s][:, :k])):
            r = ratio(getattr(got, f)[0], want)
            print(name, s, f, "max |lazy - recording| / max(1, |x|):", r)
            assert r <= BOUND_LAZY <= 1e-12, (name, s, f)


# ---- 2. the invariant ------------------------------------------------------------------------------------------------
def assert_invariant(a, kind, cp, *, math, max_events=200000, net=True):
    """a = (adj, loc, scale, queue_cap, seed, customers, states); cp (S,) or (B,S).  -> (snapshots, the shorter runs)."""
    adj, loc, scale, qcap, seed, _customers, states = a
    kw = dict(math=math, max_events=max_events, histogram=True, kind=kind)
    sn = sv.run_stats_snapshots_host(adj, loc, scale, qcap, seed, cp, states, **kw)
    runs = []
    for s in range(sn.checkpoints.shape[1]):
        want = sv.run_stats_host(adj, loc, scale, qcap, seed, sn.checkpoints[:, s], states, net=net, **kw)
        got = sv.snapshot(sn, s)
        for f in FIELDS + ("is_source",):
            assert bits(getattr(got, f)) == bits(getattr(want, f)), (s, f, getattr(got, f), getattr(want, f))
        assert bits(sn.stop[:, s]) == bits(want.stop_reason)
        runs.append(want)
    for f in STATE:                                       # the run to the last checkpoint
        assert bits(getattr(sn, f)) == bits(getattr(runs[-1], f)) == bits(getattr(sn.snaps, f)), f
    return sn, runs


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("dim", DIST_DIMS)
def test_every_snapshot_is_the_shorter_run_dist_corpus(dim, math):
    a, kind = dist_case_arrays(dist_names_of_dim(dim))
    sn, _ = assert_invariant(a, kind, CHECKPOINTS, math=math)
    assert (sn.stop == CUSTOMERS).all() and (np.diff(sn.snaps.events, axis=1) >= 0).all()


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("dim", NET_DIMS)
def test_every_snapshot_is_the_shorter_run_net_corpus(dim, math):
    names = net_names_of_dim(dim)
    a, kind = net_case_arrays(names)
    sn, _ = assert_invariant(a, kind, CHECKPOINTS, math=math)
    for b, n in enumerate(names):
        if n != "raises":
            assert (sn.stop[b] == CUSTOMERS).all(), n
            continue
        # the reference raises in this run: the checkpoints it passed before are healthy shorter runs, the rest zeros
        first = sn.stop[b].tolist().index(ERROR)
        assert first >= 3 and sn.stop[b].tolist() == [CUSTOMERS] * first + [ERROR] * (7 - first)
        assert sn.snaps.events[b, first - 1] > 0 and not sn.snaps.queue_time[b, first:].any()
        for f in sv.STATS_NODE_FIELDS + ("clock", "end_time", "total_customers", "events", "n_records"):
            assert not getattr(sn.snaps, f)[b, first:].any(), f
        assert same_state(sv.state_of(sn, b), a[6][b])


@pytest.mark.parametrize("math", [0, 1])
def test_runs_that_end_for_another_reason(math):
    # cut by max_events: the checkpoints not reached hold the final state and reason 2
    a, kind = dist_case_arrays(dist_names_of_dim(5))
    sn, runs = assert_invariant(a, kind, CHECKPOINTS, math=math, max_events=60)
    assert sn.stop[0].tolist() == [CUSTOMERS] * 3 + [EVENTS] * 4 and (sn.snaps.events[0, 3:] == 60).all()
    assert bits(sn.snaps.queue_time[0, 3]) == bits(sn.snaps.queue_time[0, 6]) and sn.snaps.queue_time[0, 6].any()
    # refused samples (a negative scale, servers that never turn positive) between healthy ones
    a, kind = refused_dist_batch()
    sn, _ = assert_invariant(a, kind, CHECKPOINTS, math=math)
    assert [r[-1] for r in sn.stop.tolist()] == [CUSTOMERS, ERROR, ERROR, CUSTOMERS, ERROR, CUSTOMERS]
    assert (sn.stop[1] == ERROR).all() and not sn.snaps.queue_time[1].any() and not sn.snaps.served[1].any()
    for b in (1, 2, 4):
        assert same_state(sv.state_of(sn, b), a[6][b]), b
    # the draw budget: a uniform server on [-2, -1]
    a, kind = dist_case_arrays(["uni2"])
    loc = a[1].copy()
    loc[0, 1] = -2.0
    sn, _ = assert_invariant((a[0], loc, *a[2:]), kind, (1, 2, 5, 40), math=math, max_events=40)
    assert sn.stop.tolist() == [[CUSTOMERS, BUDGET, BUDGET, BUDGET]]


def test_rows_of_checkpoints_that_differ_and_the_all_normal_default():
    a, kind = dist_case_arrays(["mix5"] * 3)
    cp = np.array([[1, 2, 3, 4], [7, 70, 71, 300], [2, 9, 10, 11]])
    sn, _ = assert_invariant(a, kind, cp, math=1)
    assert bits(sn.snaps.served[0, 1]) == bits(sn.snaps.served[2, 0]) and sn.checkpoints.dtype == np.int64
    one, _ = assert_invariant(a, kind, [137], math=1)                       # S = 1: the statistics run itself
    assert one.snaps.served.shape == (3, 1, 5)
    # kind=None is every node normal: the entry without kinds, byte for byte
    from test_des_corpus import case_arrays, names_of_dim
    arrays = case_arrays(names_of_dim(5))
    sn = sv.run_stats_snapshots_host(*arrays[:5], (3, 40, 41), arrays[6], math=1, histogram=True)
    for s, n in enumerate((3, 40, 41)):
        want = sv.run_stats_host(*arrays[:5], np.full(len(arrays[4]), n), arrays[6], math=1, histogram=True)
        for f in FIELDS:
            assert bits(getattr(sv.snapshot(sn, s), f)) == bits(getattr(want, f)), (s, f)


# ---- 3. the surface --------------------------------------------------------------------------------------------------
SPEC = sv.mm1k_spec(0.8, 1.0, 3, 400, seed=7)


def test_window_against_numpy():
    sn = sv.run_stats_snapshots([SPEC, sv.mm1k_spec(1.5, 1.0, 2, 1)], (50, 200, 400), histogram=True)
    w = sv.window(sn, 0, 2)
    st = sn.snaps
    for f in ("served", "reneges", "generated", "time_in_service", "time_in_queue", "queue_area", "arrival_time", "clock",
              "end_time", "events", "n_records", "queue_time"):
        a = np.asarray(getattr(st, f))
        assert bits(getattr(w, f)) == bits(a[:, 2] - a[:, 0]) and getattr(w, f).dtype == a.dtype, f
    for f in ("max_queue", "total_customers", "stop_reason"):
        assert bits(getattr(w, f)) == bits(getattr(st, f)[:, 2]), f
    assert np.array_equal(w.is_source, st.is_source) and bits(w.mt_key) == bits(sn.mt_key)
    whole = sv.window(sn, None, 1)
    for f in FIELDS:
        assert bits(getattr(whole, f)) == bits(getattr(st, f)[:, 1]), f
    m = sv.metrics(w)
    clock = (st.clock[:, 2] - st.clock[:, 0]).astype(np.float64)
    assert bits(m["server_utilizations"][:, 1]) == bits((st.time_in_service[:, 2, 1] - st.time_in_service[:, 0, 1]) / clock)
    assert bits(m["avg_queue_length"][:, 1]) == bits((st.queue_area[:, 2, 1] - st.queue_area[:, 0, 1]) / clock)
    assert bits(m["queue_length_probabilities"][:, 1]) == bits((st.queue_time[:, 2, 1] - st.queue_time[:, 0, 1])
                                                               / clock[:, None])
    assert "one service" in sv.window.__doc__ and "606" in sv.window.__doc__


def summary(v):
    """float64 restatement: mean, sem (ddof 1) and n over axis 0 of the values that are not NaN."""
    v = np.asarray(v, dtype=np.float64)
    have = ~np.isnan(v)
    n = have.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(have, v, 0.0).sum(axis=0) / n
        var = np.where(have, (v - mean) ** 2, 0.0).sum(axis=0) / (n - 1)
        sem = np.where(n > 1, np.sqrt(var) / np.sqrt(n), np.nan)
    return np.where(n > 0, mean, np.nan), sem, n


def test_convergence_is_replicate_at_every_checkpoint():
    seeds, cp = [11, 12, 13, 14, 15], (20, 100, 400)
    c = sv.convergence(SPEC, seeds, cp)
    assert c.checkpoints.tolist() == list(cp) and c.valid.shape == (5, 3) and c.valid.all()
    for s, n in enumerate(cp):
        rep = sv.replicate(sv.mm1k_spec(0.8, 1.0, 3, n), seeds)
        for f in FIELDS:
            assert bits(getattr(sv.snapshot(c.snaps, s), f)) == bits(getattr(rep.stats, f)), (n, f)
        for name in sv.METRIC_NAMES + sv.TOTAL_NAMES:
            mean, sem, count = summary(rep.metrics[name])
            assert np.array_equal(c.mean[name][s], mean, equal_nan=True), (n, name)
            assert np.allclose(c.sem[name][s], sem, rtol=1e-13, atol=0, equal_nan=True), (n, name)
            assert np.array_equal(c.n[name][s], count) and np.array_equal(c.mean[name][s], rep.mean[name], equal_nan=True)
    assert c.mean["server_utilizations"].shape == (3, 2) and c.mean["total_L"].shape == (3,)
    assert (c.sem["server_utilizations"][1:, 1] < c.sem["server_utilizations"][0, 1]).all()      # the band narrows
    with pytest.raises(ValueError, match="ascending"):
        sv.convergence(SPEC, seeds, (100, 100))
    with pytest.raises(ValueError, match="no seeds"):
        sv.convergence(SPEC, [], cp)


@pytest.mark.parametrize("warmup", [0, 150])
def test_batch_means_against_numpy(warmup):
    bm = sv.batch_means(SPEC, 21, n_batches=6, batch_customers=250, warmup=warmup)
    cp = [warmup + j * 250 for j in range(0 if warmup else 1, 7)]
    assert bm.checkpoints.tolist() == cp and (bm.snaps.stop == CUSTOMERS).all()
    adj, kind, loc, scale, qcap, _seed, _cust = sv.net_arrays([SPEC])
    sn = sv.run_stats_snapshots_host(adj, loc, scale, qcap, [21], cp, sv.replication_states([21]), math=1, kind=kind)
    tis, clock = sn.snaps.time_in_service[0, :, 1], sn.snaps.clock[0]
    tiq, served = sn.snaps.time_in_queue[0, :, 1], sn.snaps.served[0, :, 1]
    if not warmup:
        tis, clock, tiq, served = (np.concatenate([[0], x]) for x in (tis, clock, tiq, served))
    util = np.diff(tis) / np.diff(clock)
    wq = np.diff(tiq) / np.diff(served)
    for name, v in (("server_utilizations", util), ("avg_queue_time", wq)):
        assert bits(bm.values[name][:, 1]) == bits(v), name
        mean, sem, n = summary(v)
        assert bm.mean[name][1] == mean and np.isclose(bm.sem[name][1], sem, rtol=1e-13, atol=0) and bm.n[name][1] == 6
        d = v - v.mean()
        assert np.isclose(bm.lag1[name][1], (d[:-1] * d[1:]).sum() / (d * d).sum(), rtol=1e-12, atol=0), name
        assert -1.0 <= bm.lag1[name][1] <= 1.0
    assert bm.values["server_utilizations"].shape == (6, 2) and np.isnan(bm.mean["server_utilizations"][0])
    assert bm.values["total_U"].shape == (6,)
    with pytest.raises(ValueError, match="before its last checkpoint"):
        sv.batch_means(SPEC, 21, n_batches=6, batch_customers=250, warmup=warmup, max_events=500)
    with pytest.raises(ValueError, match="n_batches"):
        sv.batch_means(SPEC, 21, n_batches=1, batch_customers=250)


def test_warmup_zero_is_todays_path_and_warmup_is_the_window(monkeypatch):
    lib = _lib.load()
    called = []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("gdm_des_"):
                called.append(name)
            return getattr(lib, name)

    today = sv.replicate(SPEC, [1, 2, 3])
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    rep = sv.replicate(SPEC, [1, 2, 3], warmup=0)
    sw = sv.mm1k_sweep([0.8], [1.0], [3], [1, 2], customers=300, warmup=0)
    mc = sv.mmck_sweep([2], [1.5], [1.0], [2], [1, 2], customers=300, warmup=0)
    assert called == ["gdm_des_stats_batch_dist_host", "gdm_des_stats_batch_dist_host", "gdm_des_stats_batch_net_host"]
    for f in today.stats._fields:
        assert bits(getattr(rep.stats, f)) == bits(getattr(today.stats, f)), f
    for name in today.mean:
        assert np.array_equal(rep.mean[name], today.mean[name], equal_nan=True), name
    for got, want in ((sw, sv.mm1k_sweep([0.8], [1.0], [3], [1, 2], customers=300)),
                      (mc, sv.mmck_sweep([2], [1.5], [1.0], [2], [1, 2], customers=300))):
        for f in want.stats._fields:
            assert bits(getattr(got.stats, f)) == bits(getattr(want.stats, f)), f
        for name in sv.SWEEP_NAMES:
            assert np.array_equal(got.values[name], want.values[name], equal_nan=True), name
    del called[:]
    # warmup > 0: the window between the two checkpoints of the same runs
    rep = sv.replicate(SPEC, [1, 2, 3], warmup=100)
    assert called == ["gdm_des_stats_batch_snap_host"]
    arrays, kind, _net = sv._replication_inputs("test", SPEC, [1, 2, 3], None)
    sn = sv.run_stats_snapshots_host(*arrays[:5], (100, 400), arrays[6], math=1, kind=kind)
    want = sv.window(sn, 0, 1)
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert bits(getattr(rep.stats, f)) == bits(getattr(want, f)), f
    assert (rep.stats.served[:, 1] < today.stats.served[:, 1]).all() and rep.valid.all()
    for f in (lambda: sv.replicate(SPEC, [1], warmup=400), lambda: sv.replicate(SPEC, [1], warmup=-1),
              lambda: sv.mm1k_sweep([0.8], [1.0], [3], [1], customers=300, warmup=300)):
        with pytest.raises(ValueError, match="warmup"):
            f()
    mc = sv.mmck_sweep([2, 1], [1.5, 0.8], [1.0, 1.0], [2, 0], [1, 2], customers=300, warmup=100)
    full = sv.mmck_sweep([2, 1], [1.5, 0.8], [1.0, 1.0], [2, 0], [1, 2], customers=300)
    assert mc.stats.served.shape == (4, 3) and (mc.stats.served[:, 1] < full.stats.served[:, 1]).all()
    assert np.array_equal(mc.stats.total_customers, full.stats.total_customers)


def test_spec_level_snapshots_and_their_refusals():
    sn = sv.run_stats_snapshots([SPEC], (5, 50))
    adj, kind, loc, scale, qcap, seed, _cust = sv.net_arrays([SPEC])
    want = sv.run_stats_snapshots_host(adj, loc, scale, qcap, seed, (5, 50), None, math=1, kind=kind)
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert bits(getattr(sn.snaps, f)) == bits(getattr(want.snaps, f)), f
    assert sn.snaps.queue_time is None and sv.snapshot(sn, 1).queue_time is None
    for bad in ((0, 5), (5, 5), (6, 5), (), ((1, 2), (3, 3))):
        with pytest.raises(ValueError, match="ascending"):
            sv.run_stats_snapshots([SPEC], bad)
    with pytest.raises(ValueError, match="checkpoints must be"):
        sv.run_stats_snapshots_host(adj, loc, scale, qcap, seed, np.ones((2, 2), dtype=np.int64), None, kind=kind)
    gamma = sv.mm1k_spec(0.8, 1.0, 3, 100)
    gamma.distributions = [["gamma", 2.0, 0.0, 1.0], ["normal", 0.5, 0.1]]
    with pytest.raises(NotImplementedError, match="gamma"):
        sv.run_stats_snapshots([gamma], (5, 50))
    # nothing falls back quietly: with a device none of these returns host results (no GPU is touched here)
    for f in (lambda: sv.replicate(SPEC, [1], warmup=10, device="cuda"),
              lambda: sv.mm1k_sweep([0.8], [1.0], [3], [1], customers=300, warmup=10, device="cuda"),
              lambda: sv.mmck_sweep([2], [1.5], [1.0], [2], [1], customers=300, warmup=10, device="cuda"),
              lambda: sv.run_stats_snapshots([SPEC], (5, 50), device="cuda"),
              lambda: sv.convergence(SPEC, [1, 2], (5, 50), device="cuda"),
              lambda: sv.batch_means(SPEC, 1, n_batches=2, batch_customers=50, device="cuda")):
        with pytest.raises(Exception):
            f()


def test_the_entry_validates_its_arguments():
    lib = _lib.load()
    b, dim, cap, s = 2, 5, 4, 3
    arrays = [np.zeros(4096, dtype=np.float64) for _ in range(27)]
    ptrs = [a.ctypes.data for a in arrays]
    kind = np.zeros(b * dim + 1, dtype=np.int32)
    snap = np.array([[1, 2, 3], [4, 5, 9]], dtype=np.int64)

    def host(kind=kind.ctypes.data, ptrs=ptrs, snap=snap, s=s, math=1, max_events=1000, dim=dim):
        args = [ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:5], None if snap is None else snap.ctypes.data, s, cap, math,
                max_events, *ptrs[6:24], None]
        return lib.gdm_des_stats_batch_snap_host(*args), lib.gdm_last_error()

    for kw, word in ((dict(kind=None), b"null pointer"), (dict(ptrs=[None] + ptrs[1:]), b"null pointer"),
                     (dict(snap=None), b"null pointer"), (dict(math=2), b"math"), (dict(max_events=0), b"max_events"),
                     (dict(s=0), b"<= S <="), (dict(s=257), b"<= S <="), (dict(dim=0), b"dim")):
        rc, msg = host(**kw)
        assert rc == -1 and b"gdm_des_stats_batch_snap_host" in msg and word in msg, (kw, msg)
    kind[7] = 5
    rc, msg = host()
    kind[7] = 0
    assert rc == -1 and b"gdm_des_stats_batch_snap_host: kind 5 at sample 1, node 2" in msg, msg
    for rows, sample, entry in (([[1, 2, 3], [4, 4, 9]], 1, 1), ([[0, 2, 3], [4, 5, 9]], 0, 0), ([[1, 2, 3], [4, 5, 3]], 1, 2),
                                ([[-1, 2, 3], [4, 5, 9]], 0, 0)):
        rc, msg = host(snap=np.array(rows, dtype=np.int64))
        assert rc == -1 and f"snap_customers of sample {sample} must be strictly ascending".encode() in msg, msg
        assert f"(entry {entry})".encode() in msg, msg
        with pytest.raises(_lib.GdmError, match="strictly ascending"):
            sv.run_stats_snapshots_host(np.zeros((2, 2, 2)), np.ones((2, 2)), np.ones((2, 2)), np.ones((2, 2)), [1, 2],
                                        rows, [np.random.RandomState(1).get_state()] * 2)


# ---- 4. warm-up beside theory ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warm_sweep():
    cfg = G["grid/config"]
    return sv.mm1k_sweep(cfg[:, 0], cfg[:, 1], cfg[:, 2].astype(int), G["grid/seeds"], customers=int(G["grid/customers"]),
                         math=0, warmup=int(G["grid/warmup"]))


def test_warm_sweep_runs_are_the_recorded_reference_runs(warm_sweep):
    cfg, seeds = G["grid/config"], G["grid/seeds"]
    assert cfg.shape == (6, 3) and len(seeds) == 16 and int(G["grid/warmup"]) == 1000 and int(G["grid/customers"]) == 4000
    states = sv.replication_states(seeds) * 6
    specs = [sv.mm1k_spec(lam, mu, int(cap), 4000, s) for lam, mu, cap in cfg for s in seeds]
    adj, kind, loc, scale, qcap, seed, _cust = sv.dist_arrays(specs)
    sn = sv.run_stats_snapshots_host(adj, loc, scale, qcap, seed, (1000, 4000), states, math=0, max_events=4 * 4000 + 64,
                                     histogram=True, kind=kind)
    assert (sn.stop == CUSTOMERS).all()
    for s, p in enumerate(("w_", "c_")):
        got = sv.snapshot(sn, s)
        for f in INTS + ("total_customers",):
            assert np.array_equal(getattr(got, f), G[f"grid/{p}{f}"]), (p, f)
        for f in EVENT_ORDER:
            assert bits(getattr(got, f)) == bits(G[f"grid/{p}{f}"]), (p, f)
        for f in ("queue_area", "queue_time"):
            r = ratio(getattr(got, f), G[f"grid/{p}{f}"])
            print(p, f, "max |lazy - recording| / max(1, |x|):", r)
            assert r <= BOUND_LAZY <= 1e-12, (p, f)
    want = sv.window(sn, 0, 1)
    for f in FIELDS:
        assert bits(getattr(warm_sweep.stats, f)) == bits(getattr(want, f)), f
    # the window of the RECORDED runs, bit for bit in the sums the reference accumulates in event order
    for f in INTS[:2] + ("generated",) + EVENT_ORDER:
        assert bits(getattr(warm_sweep.stats, f)) == bits(G[f"grid/c_{f}"] - G[f"grid/w_{f}"]), f


def test_warm_sweep_agrees_with_theory(warm_sweep):
    worst, count = check_z(warm_sweep, 16)
    assert count == 6 * 4 + sum(int(c) + 1 for c in G["grid/config"][:, 2]) == 50
    assert worst <= Z_BOUND and abs(worst - float(G["grid/max_abs_z"])) <= 1e-9     # the recording's own largest |z|
    assert float(G["grid/max_abs_z"]) <= Z_BOUND and float(G["grid/max_abs_z_full"]) <= Z_BOUND


# ---- 5. the policy as a stand-alone program under the host sanitizers ------------------------------------------------
def stand_alone_cases():
    """(label, adj, loc, scale, kind, qcap, seed, checkpoints, max_events, state): the tie case, the cap-0 station, a
    station behind a branch node, the net the reference raises on, a run cut by max_events, and S = 1."""
    out = []
    for n, cp, max_events in (("det_tie", (1, 2, 30, 31, 120), 200000), ("cap0", (1, 50, 200), 200000),
                              ("branch_queue", (1, 2, 3, 150, 300), 200000), ("raises", (1, 3, 100), 200000),
                              ("mixed", (1, 20, 21, 300), 70), ("mm2_cap2", (300,), 200000)):
        (adj, loc, scale, qcap, seed, _cust, states), kind = net_case_arrays([n])
        out.append((n, adj[0], loc[0], scale[0], kind[0].astype(np.int32), qcap[0].astype(np.int32), int(seed[0]),
                    np.array(cp, dtype=np.int64), max_events, states[0]))
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of tools/des_snap_host.cpp "
                    "did not run")
    cases = stand_alone_cases()
    exe, cases_bin, snaps_bin = str(tmp_path / "des_snap_host"), str(tmp_path / "cases.bin"), str(tmp_path / "snaps.bin")
    with open(cases_bin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _n, adj, loc, scale, kind, qcap, seed, cp, max_events, st in cases:
            f.write(struct.pack("<iiiiqqd", adj.shape[0], int(st[3]), int(st[2]), len(cp), seed, max_events, float(st[4])))
            for a, dt in ((adj, "<f8"), (loc, "<f8"), (scale, "<f8"), (kind, "<i4"), (qcap, "<i4"), (st[1], "<u4"),
                          (cp, "<i8")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            *static, "-I", os.path.join(ROOT, "gan_des_midi_music_gen_amd", "csrc"),
                            os.path.join(ROOT, "tools", "des_snap_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases_bin, snaps_bin], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    with open(snaps_bin, "rb") as f:
        for n, adj, loc, scale, kind, qcap, seed, cp, max_events, st in cases:
            dim, s = adj.shape[0], len(cp)
            reason, has, pos, stride, gauss = struct.unpack("<iiiid", f.read(24))

            def rows(dt, *shape):
                return np.frombuffer(f.read(np.dtype(dt).itemsize * int(np.prod(shape))), dtype=dt).reshape(shape)

            got = {"stop_reason": rows("<i4", s), "total_customers": rows("<i8", s), "events": rows("<i8", s),
                   "n_records": rows("<i8", s), "clock": rows("<f8", s), "end_time": rows("<f8", s),
                   "served": rows("<i8", s, dim), "reneges": rows("<i8", s, dim), "generated": rows("<i8", s, dim),
                   "max_queue": rows("<i4", s, dim), "time_in_service": rows("<f8", s, dim),
                   "time_in_queue": rows("<f8", s, dim), "queue_area": rows("<f8", s, dim),
                   "arrival_time": rows("<f8", s, dim), "queue_time": rows("<f8", s, dim, stride + 1)}
            key = rows("<u4", 624)
            assert stride == int(qcap.max()), n
            want = sv.run_stats_snapshots_host(adj[None], loc[None], scale[None], qcap[None], [seed], cp, [st], math=1,
                                               max_events=max_events, histogram=True, kind=kind[None])
            assert reason == want.stop[0, -1] == {"raises": ERROR, "mixed": EVENTS}.get(n, CUSTOMERS), n
            for k in got:
                w = getattr(want.snaps, k)[0]
                # (the program's histogram follows the largest capacity exactly; the library's floor for it is 1)
                assert bits(got[k]) == bits(w[..., :stride + 1] if k == "queue_time" else w), (n, k)
            assert same_state(("MT19937", key, pos, has, gauss), sv.state_of(want, 0)), n
            assert n != "raises" or got["stop_reason"].tolist() == [CUSTOMERS, CUSTOMERS, ERROR]
            assert n != "mixed" or got["stop_reason"].tolist() == [CUSTOMERS, CUSTOMERS, CUSTOMERS, EVENTS]
        assert f.read() == b""
