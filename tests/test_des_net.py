"""The reference's 'queue' and 'branch' nodes (des::AnyNode in csrc/des_sim.h, behind gdm_des_stats_batch_net_host and
gdm_des_run_batch_net_host) against tests/golden/des_net.npz: logs and accumulators of the REFERENCE's own Sim on 12 nets
with such nodes, one net it raises on, and a grid of M/M/c/N stations, recorded by tests/golden/make_des_net_golden.py.
Runs without a GPU.

  1. math=0 (libm, numpy's bits), cases of one dim stacked into one batch (the raising net among the healthy ones of
     dim 4), in file order and shuffled: the log is the recording record for record and bit for bit, with the same
     stop reason and final generator state; the statistics' counts and `events` (the recorded pops minus the one that
     ends the run) are equal; the sums in event order are bit-equal; queue_area / queue_time within
     lazy_bound(popped) * max(1, |x|) -- GRID_LAZY's argument on the RECORDED number of popped events, which the re-pops
     of delayed departures add to.  Measured worst: 7.07e-16 on the corpus (queue_area, c4; bound 4.2e-13 there),
     1.32e-15 on the grid (queue_area; bound 5.6e-12).
  2. math=1 against math=0: the same counts, stop reasons, record structure and generator states, values within 1e-12.
  3. kinds 0..2 through the _net entries give the bytes of the _dist entries on des_dist.npz's corpus, log and
     statistics, both maths, refused samples included.
  4. refusals: kinds 5 and -1 refuse the host calls by message; the raising net, a source that is a queue node and a
     queue node whose only children are sources stop with 3 -- an empty log, zeros, the state kept --, neighbours
     untouched.
  5. the argument checks of the two device entries (no launch: safe without a GPU).
  6. queueing_theory.mmck.
  7. mmck_sweep(math=0) on the recorded grid is the reference's runs, every |z| <= 4, the worst the recorded one.
  8. the public surface: run_stats, replicate, run_batch_dist and net_arrays take such specs, write_music_log(kind=)
     writes the reference's text, what refused keeps refusing.
  9. tools/des_net_host.cpp, the policy as a stand-alone program under the host compiler's sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import _lib, ops, queueing_theory as qt, simulation_v3 as sv
from gan_des_midi_music_gen_amd.matrix_sim_process import DesSpec
from helpers import load_golden
from test_des_corpus import same_state
from test_des_dist import DIMS as DIST_DIMS, Z_BOUND, check_z, dist_case_arrays, dist_names_of_dim
from test_des_stats import EVENT_ORDER, INTS, ROOT, bits, ratio, sample

N = load_golden("des_net.npz")
NAMES = [str(n) for n in N["names"]]
GOOD = [n for n in NAMES if n != "raises"]
DIMS = sorted({int(N[f"{n}/sim_matrix"].shape[0]) for n in NAMES})
ERROR = 3
QUEUE, BRANCH = 3, 4
FIELDS = ("value", "event_id", "node", "kind")
PORTABLE_BOUND = 1e-12                                   # test_des_dist.py::test_portable_math_has_the_same_structure
ZERO_FIELDS = sv.STATS_NODE_FIELDS + ("clock", "end_time", "total_customers", "events", "n_records")


def lazy_bound(popped):
    """queue_area / queue_time against the recording: the reference adds (dt * length) once per popped event, the lazy
    integration fewer terms; every term costs either sum at most two roundings (the product, the addition) of 2^-53
    relative to a partial sum that stays below the final one where time does not run back (and within the max(1, .)
    floor of the comparison where a normal source of the embed nets steps back)."""
    return 2 * 2 * int(popped) * 2.0 ** -53


def names_of_dim(dim):
    return [n for n in NAMES if N[f"{n}/sim_matrix"].shape[0] == dim]


def net_state0(name):
    return np.random.RandomState(int(N[f"{name}/np_seed"])).get_state()


def final_state(name):
    return ("MT19937", N[f"{name}/final_key"], int(N[f"{name}/final_pos"]), int(N[f"{name}/final_has_gauss"]),
            float(N[f"{name}/final_gauss"]))


def net_case_arrays(names):
    """((adj, loc, scale, queue_cap, seed, customers, states), kind) of recorded cases of one dim."""
    return ((np.stack([N[f"{n}/sim_matrix"] for n in names]), np.stack([N[f"{n}/loc"] for n in names]),
             np.stack([N[f"{n}/scale"] for n in names]), np.stack([N[f"{n}/queue_list"] for n in names]),
             np.array([int(N[f"{n}/seed"]) for n in names]), np.array([int(N[f"{n}/customers"]) for n in names]),
             [net_state0(n) for n in names]), np.stack([N[f"{n}/kind"] for n in names]))


def cut(d, name):
    """The histogram cut to the case's own K + 1 columns, K = max(1, its largest capacity): queue + delayed departure
    was never longer (the recording's further column is empty)."""
    k = max(1, int(N[f"{name}/queue_list"].max())) + 1
    assert not d["queue_time"][:, k:].any(), name
    d["queue_time"] = d["queue_time"][:, :k]
    return d


def batches(math, shuffled):
    """name -> (records, stop reason, final state, statistics dict), the cases of one dim in one call each."""
    out, rs = {}, np.random.RandomState(37)
    for dim in DIMS:
        names = names_of_dim(dim)
        if shuffled and len(names) > 1:
            names = [names[i] for i in rs.permutation(len(names))] + [names[0]]
        a, kind = net_case_arrays(names)
        log = sv.run_batch_host(*a, math=math, max_records=0, kind=kind, net=True)
        st = sv.run_stats_host(*a, math=math, histogram=True, kind=kind, net=True)
        for b, n in enumerate(names):
            out[n] = (sv.sample_log(log, b), int(log.stop_reason[b]), sv.state_of(log, b), cut(sample(st, b), n))
    return out


@pytest.fixture(scope="module")
def runs():
    return {(m, sh): batches(m, sh) for m in (0, 1) for sh in (False, True)}


def test_the_recording_covers_what_it_was_made_for():
    assert DIMS == [3, 4, 5, 6, 7, 16, 128] and len(NAMES) == 13 and names_of_dim(4)[-1] == "raises"
    for n in GOOD:
        assert int(N[f"{n}/customers"]) <= 400 and set(N[f"{n}/kind"].tolist()) <= {0, 1, 2, 3, 4}, n
    for n in ("mm2_cap2", "cap0", "c1", "c4", "shared", "branch_queue", "mixed", "det_tie", "embed16", "embed128"):
        assert QUEUE in N[f"{n}/kind"] and int(N[f"{n}/delayed"]) > 0, n
    assert int(N["det_tie/redelayed"]) > 0 and (N["det_tie/scale"] == 0).all()
    arrivals = N["det_tie/value"][N["det_tie/rec_kind"] == 0]
    assert len(np.unique(arrivals)) < len(arrivals)                     # simultaneous events
    assert N["cap0/queue_list"][1] == 0 and N["cap0/max_queue"].max() == 0 and N["cap0/queue_time"][1, 1] > 0
    assert [int((N[f"{n}/kind"] == 1).sum()) for n in ("c1", "c4")] == [2, 5]
    assert N["shared/sim_matrix"][2, 4] > 0 and N["shared/max_queue"][4] > 0
    assert N["branch37/kind"][1] == BRANCH and N["branch37/sim_matrix"][1, 2:].tolist() == [0.3, 0.7]
    assert N["branch_queue/kind"].tolist()[:4] == [1, BRANCH, QUEUE, QUEUE]
    assert sorted(N["mixed/kind"].tolist()[2:]) == [0, 1, 2]
    assert N["sink_quirk/sim_matrix"][1, 0] > 0 and not N["sink_quirk/sim_matrix"][1, 2:].any()
    for n in ("embed16", "embed128"):
        assert sorted(set(N[f"{n}/kind"].tolist())) == [0, QUEUE, BRANCH], n
    assert str(N["raises/exception"]) == "KeyError"


# ---- 1. libm: the reference's log and accumulators -------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", GOOD)
def test_libm_log_and_statistics_are_the_recording(runs, name, shuffled):
    rec, reason, state, got = runs[0, shuffled][name]
    assert reason == 1 and len(rec) == len(N[f"{name}/value"]), name
    for f in FIELDS:
        want = N[f"{name}/{'rec_kind' if f == 'kind' else f}"]
        assert rec[f].dtype == want.dtype and bits(rec[f]) == bits(want), (name, f)
    assert same_state(state, final_state(name)) and same_state(got["state"], final_state(name)), name
    for f in INTS:
        assert np.array_equal(got[f], N[f"{name}/{f}"]), (name, f)
    assert got["total_customers"] == N[f"{name}/total_customers"] and got["n_records"] == len(rec), name
    assert got["events"] == int(N[f"{name}/popped"]) - 1 and got["stop_reason"] == 1, name
    assert np.array_equal(got["is_source"], N[f"{name}/is_source"]), name
    for f in EVENT_ORDER:
        assert bits(got[f]) == bits(N[f"{name}/{f}"]), (name, f, got[f], N[f"{name}/{f}"])
    k = got["queue_time"].shape[1]
    assert not N[f"{name}/queue_time"][:, k:].any(), name
    for f, want in (("queue_area", N[f"{name}/queue_area"]), ("queue_time", N[f"{name}/queue_time"][:, :k])):
        r = ratio(got[f], want)
        print(name, f, "max |lazy - recording| / max(1, |x|):", r, "bound", lazy_bound(N[f"{name}/popped"]))
        assert r <= lazy_bound(N[f"{name}/popped"]) <= 1e-12, (name, f)


# ---- 2. portable math against libm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_portable_math_has_the_same_structure(runs, name):
    got, want = runs[1, False][name], runs[0, False][name]
    assert got[1] == want[1] and len(got[0]) == len(want[0]), name
    for f in ("event_id", "node", "kind"):
        assert np.array_equal(got[0][f], want[0][f]), (name, f)
    assert same_state(got[2], want[2]) and same_state(got[3]["state"], want[3]["state"]), name
    assert ratio(got[0]["value"], want[0]["value"]) <= PORTABLE_BOUND, name
    for f in INTS + ("total_customers", "n_records", "events", "stop_reason"):
        assert np.array_equal(got[3][f], want[3][f]), (name, f)
    for f in EVENT_ORDER + ("queue_area",):
        assert ratio(got[3][f], want[3][f]) <= PORTABLE_BOUND, (name, f)
    shuffled = runs[1, True][name]
    assert bits(shuffled[0]) == bits(got[0]) and same_state(shuffled[2], got[2]), name


# ---- 3. kinds 0..2 are the _dist entries -----------------------------------------------------------------------------
def refused_dist_batch():
    """test_des_dist.py's batch of healthy and refused samples (a negative scale, servers that never turn positive)."""
    names = ["uni_neg", "uni_neg", "uni_neg", "scale0_srv", "uni_neg", "scale0_src"]
    a, kind = dist_case_arrays(names)
    loc, scale = a[1].copy(), a[2].copy()
    scale[1, 2] = -0.5
    kind[2, 1], scale[2, 1] = 1, 0.0
    kind[4, 2], scale[4, 2], loc[4, 2] = 2, 0.0, 0.0
    return (a[0], loc, scale, *a[3:]), kind


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("dim", DIST_DIMS + ["refused"])
def test_kinds_without_nodes_are_the_dist_entries(dim, math):
    a, kind = refused_dist_batch() if dim == "refused" else dist_case_arrays(dist_names_of_dim(dim))
    old = sv.run_batch_host(*a, math=math, max_records=0, kind=kind)
    new = sv.run_batch_host(*a, math=math, max_records=0, kind=kind, net=True)
    assert len(old.value) > 0 and (dim != "refused" or old.stop_reason.tolist() == [1, ERROR, ERROR, 1, ERROR, 1])
    for f in old._fields:
        assert bits(getattr(new, f)) == bits(getattr(old, f)), f
    old = sv.run_stats_host(*a, math=math, histogram=True, kind=kind)
    new = sv.run_stats_host(*a, math=math, histogram=True, kind=kind, net=True)
    for f in old._fields:
        assert bits(getattr(new, f)) == bits(getattr(old, f)), f


def test_net_selects_the_entries_not_the_kinds(monkeypatch):
    lib = _lib.load()
    called = []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("gdm_des_"):
                called.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    a, kind = net_case_arrays(["c1"])
    sv.run_batch_host(*a, math=1, kind=kind, net=True)
    sv.run_stats_host(*a, math=1, kind=kind, net=True)
    with pytest.raises(_lib.GdmError, match="kind 3 at sample 0, node 1"):      # the _dist entries refuse as ever
        sv.run_stats_host(*a, math=1, kind=kind)
    with pytest.raises(_lib.GdmError, match="kind 3 at sample 0, node 1"):
        sv.run_batch_host(*a, math=1, kind=kind)
    assert called == ["gdm_des_run_batch_net_host", "gdm_des_stats_batch_net_host", "gdm_des_stats_batch_dist_host",
                      "gdm_des_run_batch_dist_host"]
    with pytest.raises(ValueError, match="net=True needs kind"):
        sv.run_stats_host(*a, math=1, net=True)
    with pytest.raises(ValueError, match="net=True needs kind"):
        sv.run_batch_host(*a, math=1, net=True)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_kind_out_of_range_refuses_the_host_calls():
    a, kind = net_case_arrays(["mixed"])
    for bad in (5, -1):
        k = kind.copy()
        k[0, 4] = bad
        with pytest.raises(_lib.GdmError, match=f"gdm_des_stats_batch_net_host: kind {bad} at sample 0, node 4"):
            sv.run_stats_host(*a, math=1, kind=k, net=True)
        with pytest.raises(_lib.GdmError, match=f"gdm_des_run_batch_net_host: kind {bad} at sample 0, node 4"):
            sv.run_batch_host(*a, math=1, kind=k, net=True)


def assert_refused(log, st, b, state):
    assert log.stop_reason[b] == ERROR == st.stop_reason[b], b
    assert log.n_records[b] == 0 and log.rec_ptr[b] == log.rec_ptr[b + 1], b
    for f in ZERO_FIELDS:
        assert not np.asarray(getattr(st, f)[b]).any(), (b, f)
    assert not st.queue_time[b].any(), b
    assert same_state(sv.state_of(log, b), state) and same_state(sv.state_of(st, b), state), b


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("shuffled", [False, True])
def test_the_raising_net_among_healthy_ones(runs, math, shuffled):
    rec, reason, state, got = runs[math, shuffled]["raises"]
    assert reason == ERROR == got["stop_reason"] and len(rec) == 0
    for f in ZERO_FIELDS:
        assert not np.asarray(got[f]).any(), f
    assert not got["queue_time"].any()
    assert same_state(state, net_state0("raises")) and same_state(got["state"], net_state0("raises"))
    for n in names_of_dim(4)[:-1]:                                     # its neighbours: a run of their own
        a, kind = net_case_arrays([n])
        log = sv.run_batch_host(*a, math=math, max_records=0, kind=kind, net=True)
        assert bits(sv.sample_log(log, 0)) == bits(runs[math, shuffled][n][0]), n
        assert same_state(sv.state_of(log, 0), runs[math, shuffled][n][2]), n
        alone = cut(sample(sv.run_stats_host(*a, math=math, histogram=True, kind=kind, net=True), 0), n)
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("queue_time",):
            assert bits(alone[f]) == bits(runs[math, shuffled][n][3][f]), (n, f)


@pytest.mark.parametrize("math", [0, 1])
def test_nets_without_a_defined_run_stop_with_an_error(runs, math):
    names = ["mm2_cap2", "mm2_cap2", "mm2_cap2", "mm2_cap2", "cap0"]
    a, kind = net_case_arrays(names)
    adj = a[0].copy()
    kind[1, 0] = QUEUE                          # sample 1: a SOURCE that is a queue node (Source.__init__ raises)
    kind[2, 0] = BRANCH                         # sample 2: ... a branch node
    adj[3, 2, 2] = adj[3, 3, 3] = 1.0           # sample 3: the queue node's children are sources: it waits until +inf
    adj[3, 2, 1] = adj[3, 3, 1] = 1.0
    log = sv.run_batch_host(adj, *a[1:], math=math, max_records=0, kind=kind, net=True)
    st = sv.run_stats_host(adj, *a[1:], math=math, histogram=True, kind=kind, net=True)
    assert log.stop_reason.tolist() == [1, ERROR, ERROR, ERROR, 1]
    for b in (1, 2, 3):
        assert_refused(log, st, b, net_state0(names[b]))
    for b in (0, 4):
        want = runs[math, False][names[b]]
        assert bits(sv.sample_log(log, b)) == bits(want[0]) and same_state(sv.state_of(log, b), want[2]), b
        got = cut(sample(st, b), names[b])
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("queue_time",):
            assert bits(got[f]) == bits(want[3][f]), (b, f)


# ---- 5. argument checks ----------------------------------------------------------------------------------------------
def test_device_entries_validate_on_the_host():
    lib = _lib.load()
    b, dim, cap = 2, 5, 4
    arrays = [np.zeros(4096, dtype=np.float64) for _ in range(27)]
    ptrs = [a.ctypes.data for a in arrays]
    kind = np.zeros(b * dim + 1, dtype=np.int32)
    need = lib.gdm_des_stats_workspace_bytes(b, dim, cap)
    buf = np.zeros(need + 64, dtype=np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16

    def stats(dim=dim, cap=cap, ptrs=ptrs, kind=kind.ctypes.data, hist=None, ws=base, ws_bytes=need, max_events=1000):
        args = [ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:6], cap, max_events, *ptrs[6:24], hist, ws, ws_bytes, None]
        return lib.gdm_des_stats_batch_net(*args), lib.gdm_last_error()

    for missing in (0, 2, 3, 9, 10, 17, 23):
        rc, msg = stats(ptrs=[None if i == missing else p for i, p in enumerate(ptrs)])
        assert rc == -1 and b"gdm_des_stats_batch_net: null pointer" in msg, missing
    for kw, word in ((dict(kind=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=base + 8), b"workspace"), (dict(dim=129), b"dim"),
                     (dict(cap=0), b"max_queue_cap"), (dict(max_events=0), b"max_events"),
                     (dict(ptrs=[ptrs[0] + 4] + ptrs[1:]), b"aligned"), (dict(kind=kind.ctypes.data + 2), b"aligned"),
                     (dict(hist=ptrs[24] + 2), b"aligned")):
        rc, msg = stats(**kw)
        assert rc == -1 and b"gdm_des_stats_batch_net:" in msg and word in msg, (kw, msg)

    need_log = lib.gdm_des_batch_workspace_bytes(b, dim, cap)
    assert need_log <= need
    records = 16

    def run(dim=dim, cap=cap, ptrs=ptrs, kind=kind.ctypes.data, ws=base, ws_bytes=need_log, max_events=1000,
            max_records=records, n_cap=b * records):
        args = [ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:6], cap, max_events, max_records, *ptrs[6:14], n_cap,
                *ptrs[14:17], ws, ws_bytes, None]
        return lib.gdm_des_run_batch_net(*args), lib.gdm_last_error()

    for missing in (0, 2, 3, 6, 10, 13, 14, 16):
        rc, msg = run(ptrs=[None if i == missing else p for i, p in enumerate(ptrs)])
        assert rc == -1 and b"gdm_des_run_batch_net: null pointer" in msg, missing
    for kw, word, code in ((dict(kind=None), b"null pointer", -1), (dict(ws=None), b"null pointer", -1),
                           (dict(ws_bytes=need_log - 1), b"workspace", -3), (dict(ws=base + 8), b"workspace", -3),
                           (dict(dim=129), b"dim", -1), (dict(cap=0), b"max_queue_cap", -1),
                           (dict(max_events=0), b"max_events", -1), (dict(max_records=0), b"max_records", -1),
                           (dict(n_cap=b * records - 1), b"B * max_records", -1),
                           (dict(kind=kind.ctypes.data + 2), b"aligned", -1)):
        rc, msg = run(**kw)
        assert rc == code and b"gdm_des_run_batch_net:" in msg and word in msg, (kw, rc, msg)

    def host(name, tail, kind=kind.ctypes.data, ptrs=ptrs, math=1, max_events=1000):
        return (getattr(lib, name)(ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:6], cap, math, max_events, *tail(ptrs)),
                lib.gdm_last_error())

    tails = {"gdm_des_stats_batch_net_host": lambda p: (*p[6:24], None),
             "gdm_des_run_batch_net_host": lambda p: (0, *p[6:14], 4096, *p[14:17])}
    for name, tail in tails.items():
        for kw, word in ((dict(kind=None), b"null pointer"), (dict(ptrs=[None] + ptrs[1:]), b"null pointer"),
                         (dict(math=2), b"math"), (dict(max_events=0), b"max_events")):
            rc, msg = host(name, tail, **kw)
            assert rc == -1 and name.encode() in msg and word in msg, (name, kw, msg)
        kind[7] = 5
        rc, msg = host(name, tail)
        kind[7] = 0
        assert rc == -1 and name.encode() + b": kind 5 at sample 1, node 2" in msg, msg


def test_ops_refuse_cpu_tensors():
    import torch
    z = torch.zeros
    for entry in (ops.des_run_stats_net, ops.des_run_batch_net):
        with pytest.raises(ops.GdmError):
            entry(z(1, 2, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64),
                  z(1, 2, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, dtype=torch.int64),
                  z(1, dtype=torch.int64), z(1, 624, dtype=torch.int32), z(1, dtype=torch.int32),
                  z(1, dtype=torch.int32), z(1, dtype=torch.float64), max_queue_cap=4)
    assert (ops.DES_DIST_QUEUE, ops.DES_DIST_BRANCH) == (QUEUE, BRANCH)


# ---- 6. the closed form ----------------------------------------------------------------------------------------------
def test_mmck():
    for lam, mu, cap in ((0.8, 1.0, 3), (1.5, 1.0, 2), (1.0, 1.0, 5), (0.3, 2.0, 0), (2.0, 0.5, 7)):
        one, t = qt.mm1k(lam, mu, cap), qt.mmck(lam, mu, 1, cap)
        assert sorted(one) == sorted(t)
        for key in one:                                   # the same weights; the utilisation is summed, not 1 - p[0]
            assert np.asarray(t[key]).shape == np.asarray(one[key]).shape, key
            assert np.allclose(t[key], one[key], rtol=4e-16, atol=0) or key == "utilisation", key
        assert abs(t["utilisation"] - one["utilisation"]) <= 4e-16
    for lam, mu, c, cap in ((1.5, 1.0, 2, 2), (6.0, 1.0, 4, 2), (2.0, 1.0, 3, 0), (0.5, 1.0, 3, 4), (3.0, 1.0, 3, 6)):
        t = qt.mmck(lam, mu, c, cap)
        n = c + cap
        assert t["p"].shape == (n + 1,) and abs(t["p"].sum() - 1) <= 4e-16 and (t["p"] > 0).all()
        assert t["blocking"] == t["p"][n] and abs(t["blocking"] - qt.mmck_blocking(lam, mu, c, cap)) <= 1e-15
        assert t["queue_length_probabilities"].shape == (cap + 1,)
        assert abs(t["queue_length_probabilities"].sum() - 1) <= 4e-16
        # flow balance: accepted arrivals leave through the c servers; Little's law on the queue; L = LQ + busy servers
        assert abs(lam * (1 - t["blocking"]) - c * mu * t["utilisation"]) <= 4e-15 * max(lam, c * mu)
        assert abs(t["WQ"] * lam * (1 - t["blocking"]) - t["LQ"]) <= 1e-14 * max(1.0, t["LQ"])
        assert abs(t["L"] - (t["LQ"] + c * t["utilisation"])) <= 1e-14 * max(1.0, t["L"])
        assert abs(t["W"] - (t["WQ"] + 1 / mu)) <= 1e-14 * max(1.0, t["W"])
    # Erlang B (no waiting room): c = 2, a = 1: (1/2) / (1 + 1 + 1/2); c = 3, a = 2: (8/6) / (1 + 2 + 2 + 8/6)
    assert abs(qt.mmck(1.0, 1.0, 2, 0)["blocking"] - 0.2) <= 1e-16
    assert abs(qt.mmck(2.0, 1.0, 3, 0)["blocking"] - (8 / 6) / (5 + 8 / 6)) <= 1e-16
    assert qt.mmck(2.0, 1.0, 3, 0)["LQ"] == 0.0 and qt.mmck(2.0, 1.0, 3, 0)["queue_length_probabilities"].tolist() == [1.0]
    for bad in ((0.0, 1.0, 1, 1), (1.0, 1.0, 0, 1), (1.0, 1.0, 1, -1)):
        with pytest.raises(ValueError):
            qt.mmck(*bad)


# ---- 7. the sweep beside theory --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_sweep():
    cfg = N["grid/config"]
    return sv.mmck_sweep(cfg[:, 0].astype(int), cfg[:, 1], cfg[:, 2], cfg[:, 3].astype(int), N["grid/seeds"],
                         customers=int(N["grid/customers"]), math=0)


def together(a, largest=False):
    """The recording's padded node rows as mmck_sweep's three: source, queue node, the servers together."""
    rest = a[:, 2:].max(axis=1) if largest else a[:, 2:].sum(axis=1)
    return np.stack([a[:, 0], a[:, 1], rest], axis=1)


def test_sweep_runs_are_the_recorded_reference_runs(grid_sweep):
    st, cfg = grid_sweep.stats, N["grid/config"]
    assert cfg.shape == (6, 4) and len(N["grid/seeds"]) == 16 and st.served.shape == (96, 3)
    assert sorted(set(cfg[:, 0].tolist())) == [1, 2, 3, 4] and sorted(set(cfg[:, 3].tolist())) == [0, 1, 2, 3]
    rho = cfg[:, 1] / (cfg[:, 0] * cfg[:, 2])
    assert rho.min() == 0.5 and rho.max() == 1.5
    assert (st.stop_reason == 1).all() and np.array_equal(st.events, N["grid/popped"] - 1)
    for f in INTS:
        assert np.array_equal(getattr(st, f), together(N[f"grid/{f}"], f == "max_queue")), f
    assert np.array_equal(st.total_customers, N["grid/total_customers"])
    for f in EVENT_ORDER:
        want = N[f"grid/{f}"]
        assert bits(getattr(st, f)) == bits(want if want.ndim == 1 else together(want)), f
    bound = lazy_bound(N["grid/popped"].max())
    for f in ("queue_area", "queue_time"):
        r = ratio(getattr(st, f), together(N[f"grid/{f}"]))
        print(f, "max |lazy - recording| / max(1, |x|):", r, "bound", bound)
        assert r <= bound <= 1e-11, f
    for i, (c, lam, mu, cap) in enumerate(cfg):
        spec = sv.mmck_spec(int(c), lam, mu, int(cap), 4000, seed=3)
        assert spec.distributions[1] == ["queue"] and list(spec.queue_list) == [0, int(cap)] + [0] * int(c)
        assert spec.sim_matrix.shape == (c + 2, c + 2) and spec.sim_matrix[1, 2:].tolist() == [1.0] * int(c)


def test_sweep_agrees_with_theory(grid_sweep):
    worst, count = check_z(grid_sweep, 16)
    assert count == 6 * 4 + sum(max(int(c), 1) + 1 for c in N["grid/config"][:, 3]) == 40
    assert worst <= Z_BOUND and abs(worst - float(N["grid/max_abs_z"])) <= 1e-9     # the recording's own largest |z|


# ---- 8. the public surface -------------------------------------------------------------------------------------------
def spec_of(name):
    dist = []
    for k, loc, scale in zip(N[f"{name}/kind"], N[f"{name}/loc"], N[f"{name}/scale"]):
        kind = sv.NODE_KINDS[k]
        dist.append([kind] if k >= QUEUE else [kind, float(scale)] if k == 1 else [kind, float(loc), float(scale)])
    dim = len(dist)
    return DesSpec(N[f"{name}/sim_matrix"], dist, N[f"{name}/queue_list"].tolist(), np.array([int(N[f"{name}/seed"])]),
                   int(N[f"{name}/customers"]), 1.0, np.zeros(dim), np.zeros(dim))


def test_spec_level_functions_take_queue_and_branch_nodes(runs, monkeypatch):
    assert sv.NODE_KINDS == ("normal", "exponential", "uniform", "queue", "branch") == sv.DIST_KINDS + ("queue", "branch")
    spec = spec_of("branch_queue")
    adj, kind, loc, scale, qcap, seed, customers = sv.net_arrays([spec])
    assert kind.tolist() == [N["branch_queue/kind"].tolist()] and kind.dtype == np.int32
    assert loc[0, 1:4].tolist() == [0.0] * 3 and scale[0, 1:4].tolist() == [0.0] * 3
    assert np.array_equal(scale[0], N["branch_queue/scale"]) and np.array_equal(qcap[0], N["branch_queue/queue_list"])
    used = []
    real_stats, real_log = sv.run_stats_host, sv.run_batch_host
    monkeypatch.setattr(sv, "run_stats_host", lambda *a, **k: (used.append(k.get("net")), real_stats(*a, **k))[1])
    monkeypatch.setattr(sv, "run_batch_host", lambda *a, **k: (used.append(k.get("net")), real_log(*a, **k))[1])
    state = net_state0("branch_queue")
    st = sv.run_stats([spec], states=[state], histogram=True)
    want = runs[1, False]["branch_queue"]
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert bits(np.asarray(getattr(st, f)[0])) == bits(want[3][f]), f
    log = sv.run_batch_dist([spec], states=[state], max_records=0)
    assert bits(sv.sample_log(log, 0)) == bits(want[0])
    log0 = sv.run_batch_dist([spec], states=[state], max_records=0, math=0)
    assert bits(sv.sample_log(log0, 0)) == bits(runs[0, False]["branch_queue"][0])
    rep = sv.replicate(spec_of("mm2_cap2"), [1, 2, 3, 4])
    assert rep.valid.all() and rep.n["server_utilizations"][2] == 4 and 0.3 < rep.mean["server_utilizations"][2] < 0.95
    assert rep.mean["avg_queue_length"][1] > 0 and np.isnan(rep.mean["server_utilizations"][0])
    sv.run_stats([sv.mm1k_spec(0.8, 1.0, 3, 50)])               # no queue or branch node: the _dist entry as ever
    assert used == [True, True, True, True, False]


def test_what_refused_keeps_refusing():
    spec = spec_of("c1")
    for f in (lambda: sv.dist_arrays([spec]), lambda: sv.spec_arrays([spec]), lambda: sv.run_batch([spec]),
              lambda: sv.Sim(spec.sim_matrix, spec.distributions, spec.queue_list, seeds=[1], logging_mode='Music')):
        with pytest.raises(NotImplementedError):
            f()
    with pytest.raises(NotImplementedError, match="queue"):
        sv.dist_arrays([spec])
    spec.distributions = [["gamma", 2.0, 0.0, 1.0], ["queue"], ["exponential", 1.0]]
    for f in (lambda: sv.net_arrays([spec]), lambda: sv.run_stats([spec]), lambda: sv.run_batch_dist([spec]),
              lambda: sv.replicate(spec, [1])):
        with pytest.raises(NotImplementedError, match="gamma"):
            f()
    with pytest.raises(ValueError):
        sv.mmck_sweep([1], [1.0], [1.0], [-1], [1], customers=10)
    with pytest.raises(ValueError):
        sv.mmck_sweep([0], [1.0], [1.0], [1], [1], customers=10)
    with pytest.raises(ValueError):
        sv.mmck_sweep([1, 2], [1.0], [1.0], [1], [1], customers=10)


def test_write_music_log_is_the_references_text(tmp_path, runs):
    """The reference writes the service time of a queue or branch node as the int 0 ("0 - 5 - 1 - processing")."""
    rec = runs[0, False]["branch_queue"][0]
    path = str(tmp_path / "simulation.log")
    sv.write_music_log(rec, path, kind=N["branch_queue/kind"])
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == len(rec) + 1
    kind, zeros = N["branch_queue/kind"], 0
    for i, line in enumerate(lines[:-1]):
        v, node, k = float(N["branch_queue/value"][i]), int(N["branch_queue/node"][i]), int(N["branch_queue/rec_kind"][i])
        timeless = k == 2 and kind[node] >= QUEUE
        zeros += timeless
        assert not timeless or v == 0.0
        want = "INFO:root:%s - %s - %s - %s" % (0 if timeless else v, int(N["branch_queue/event_id"][i]), node,
                                                sv.KIND_NAMES[k])
        assert line == want, i
    assert zeros > 300
    sv.write_music_log(rec, path)                                       # without the kinds: floats throughout
    assert sum(ln.startswith("INFO:root:0.0 - ") and ln.endswith("processing\n") for ln in open(path)) == zeros


# ---- 9. the policy as a stand-alone program under the host sanitizers ------------------------------------------------
def stand_alone_cases():
    """(label, adj, loc, scale, kind, qcap, seed, customers, state): the tie case, the cap-0 station, a station behind a
    branch node, the net the reference raises on, and a spec refused before anything runs (kind 5)."""
    out = []
    for n in ("det_tie", "cap0", "branch_queue", "raises", "mixed"):
        (adj, loc, scale, qcap, seed, cust, states), kind = net_case_arrays([n])
        if n == "mixed":
            kind = kind.copy()
            kind[0, 4] = 5
            n = "refused"
        out.append((n, adj[0], loc[0], scale[0], kind[0].astype(np.int32), qcap[0].astype(np.int32), int(seed[0]),
                    int(cust[0]), states[0]))
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of tools/des_net_host.cpp "
                    "did not run")
    cases = stand_alone_cases()
    exe, cases_bin, stats_bin = str(tmp_path / "des_net_host"), str(tmp_path / "cases.bin"), str(tmp_path / "stats.bin")
    with open(cases_bin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _n, adj, loc, scale, kind, qcap, seed, cust, st in cases:
            f.write(struct.pack("<iiiiqqqd", adj.shape[0], int(st[3]), int(st[2]), 0, seed, cust, 200000, float(st[4])))
            for a, dt in ((adj, "<f8"), (loc, "<f8"), (scale, "<f8"), (kind, "<i4"), (qcap, "<i4"), (st[1], "<u4")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            *static, "-I", os.path.join(ROOT, "gan_des_midi_music_gen_amd", "csrc"),
                            os.path.join(ROOT, "tools", "des_net_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases_bin, stats_bin], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    with open(stats_bin, "rb") as f:
        for n, adj, loc, scale, kind, qcap, seed, cust, st in cases:
            dim = adj.shape[0]
            want = None
            if n != "refused":                            # (the host ENTRY refuses the call for kind 5)
                want = sv.run_stats_host(adj[None], loc[None], scale[None], qcap[None], [seed], [cust], [st], math=1,
                                         histogram=True, kind=kind[None], net=True)
            reason, has, pos, stride, total, events, n_rec, gauss, clock, end = struct.unpack("<iiiiqqqddd", f.read(64))
            rows = {}
            for field, dt in (("served", "<i8"), ("reneges", "<i8"), ("generated", "<i8"), ("max_queue", "<i4"),
                              ("time_in_service", "<f8"), ("time_in_queue", "<f8"), ("queue_area", "<f8"),
                              ("arrival_time", "<f8")):
                rows[field] = np.frombuffer(f.read(np.dtype(dt).itemsize * dim), dtype=dt)
            qtime = np.frombuffer(f.read(8 * dim * (stride + 1)), dtype="<f8").reshape(dim, stride + 1)
            key = np.frombuffer(f.read(4 * 624), dtype="<u4")
            assert stride == int(qcap.max()), n
            if want is None or n == "raises":
                assert reason == ERROR and (total, events, n_rec) == (0, 0, 0) and clock == 0 and end == 0, n
                assert not any(r.any() for r in rows.values()) and not qtime.any(), n
                assert same_state(("MT19937", key, pos, has, gauss), st), n
                assert want is None or want.stop_reason[0] == ERROR, n
                continue
            assert reason == want.stop_reason[0] == 1 and want.served.sum() > 50, n
            assert (total, events, n_rec) == (want.total_customers[0], want.events[0], want.n_records[0]), n
            assert bits(np.float64(clock)) == bits(want.clock[0]) and bits(np.float64(end)) == bits(want.end_time[0]), n
            for field, got in rows.items():
                assert bits(got) == bits(getattr(want, field)[0]), (n, field)
            # (the program's rings and histogram follow the largest capacity exactly: none at all for the cap-0 station,
            # whose delayed departure then has no column; the library's floor for max_queue_cap is 1)
            assert bits(qtime[:, :stride + 1]) == bits(want.queue_time[0][:, :stride + 1]), n
            assert same_state(("MT19937", key, pos, has, gauss), sv.state_of(want, 0)), n
        assert f.read() == b""
