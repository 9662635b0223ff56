"""Exponential and uniform nodes in the log-free statistics run (des::AnyDist in csrc/des_sim.h, behind
gdm_des_stats_batch_dist_host) against tests/golden/des_dist.npz: the accumulators of the REFERENCE's own Server / Source
objects after Sim.run on 13 nets with 'normal', 'exponential' and 'uniform' nodes, and 6 M/M/1/K configurations x 16
seeds x 4000 customers, recorded by tests/golden/make_des_dist_golden.py.  Runs without a GPU.

  1. math=0 (libm, numpy's bits), cases of one dim stacked into one batch, in file order and shuffled: counts, stop
     reasons, total_customers and n_records equal; time_in_service, time_in_queue, arrival_time, clock and end_time
     bit-equal; queue_area and queue_time within test_des_stats.py's BOUND_LAZY = 10 x 4.79e-16 (f15: the corpus'
     worst relative difference, 400-record runs).  Measured on THESE cases, up to 4667 records: 9.60e-16
     (queue_area, rand17; queue_time 2.17e-16, rand15), beside f15's 4.79e-16.
  2. math=1 (portable, what the device runs) against math=0: same counts, stop reasons and final generator states.
  3. all-normal specs through the _dist entry with kind = 0: the bytes of gdm_des_stats_batch_host on the corpus of
     des_corpus.npz, both maths, error cases included.
  4. refusals: kind 3 refuses the host call; a negative scale, an exponential server with scale 0 and a uniform server
     with scale 0 and loc <= 0 stop that sample with reason 3, zeros, state kept, neighbours untouched; a uniform
     server whose support is <= 0 draws and ends on the draw budget.
  5. the argument checks of both _dist entries (no launch: safe without a GPU).
  6. queueing_theory's closed forms.
  7. mm1k_sweep on the recorded grid: with math=0 the accumulators are the reference's runs -- counts equal, the sums
     in event order bit-equal, queue_area / queue_time within GRID_LAZY (these runs are 8000 events long, twenty times
     the corpus': the bound is the worst case of the two summations, see there; measured 4.40e-15 queue_area,
     1.89e-16 queue_time) -- and every |z| <= 4 (the bound the recording was made under: its largest |z| is 1.64 over
     50 comparisons).
  8. run_stats / replicate take specs with the new kinds (NotImplementedError before).
  9. tools/des_dist_host.cpp, the policy as a stand-alone program under the host compiler's sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import _lib, ops, queueing_theory as qt, simulation_v3 as sv
from helpers import load_golden
from test_des_corpus import DIMS as CORPUS_DIMS, case_arrays, names_of_dim, same_state
from test_des_stats import BOUND_LAZY, EVENT_ORDER, INTS, ROOT, bits, ratio, sample

D = load_golden("des_dist.npz")
NAMES = [str(n) for n in D["names"]]
DIMS = sorted({int(D[f"{n}/sim_matrix"].shape[0]) for n in NAMES})
ERROR, BUDGET = 3, 5
Z_BOUND = 4.0
# queue_area / queue_time of a grid run: the reference adds (dt * length) once per popped event, at most 2 * customers +
# 2 of them, the lazy integration fewer; every term costs either sum at most two roundings (the product, the addition)
# of 2^-53 relative to a partial sum that never exceeds the final one (all terms >= 0 on this net: time never runs back)
GRID_LAZY = 2 * 2 * (2 * 4000 + 2) * 2.0 ** -53


def dist_names_of_dim(dim):
    return [n for n in NAMES if D[f"{n}/sim_matrix"].shape[0] == dim]


def dist_state0(name):
    return np.random.RandomState(int(D[f"{name}/np_seed"])).get_state()


def dist_case_arrays(names):
    """((adj, loc, scale, queue_cap, seed, customers, states), kind) of recorded cases of one dim."""
    return ((np.stack([D[f"{n}/sim_matrix"] for n in names]), np.stack([D[f"{n}/loc"] for n in names]),
             np.stack([D[f"{n}/scale"] for n in names]), np.stack([D[f"{n}/queue_list"] for n in names]),
             np.array([int(D[f"{n}/seed"]) for n in names]), np.array([int(D[f"{n}/customers"]) for n in names]),
             [dist_state0(n) for n in names]), np.stack([D[f"{n}/kind"] for n in names]))


def cut(d, name):
    k = max(1, int(D[f"{name}/queue_list"].max())) + 1
    assert not d["queue_time"][:, k:].any(), name
    d["queue_time"] = d["queue_time"][:, :k]
    return d


def batches(math, shuffled):
    out, rs = {}, np.random.RandomState(29)
    for dim in DIMS:
        names = dist_names_of_dim(dim)
        if shuffled and len(names) > 1:
            names = [names[i] for i in rs.permutation(len(names))] + [names[0]]
        a, kind = dist_case_arrays(names)
        st = sv.run_stats_host(*a, math=math, histogram=True, kind=kind)
        for b, n in enumerate(names):
            out[n] = cut(sample(st, b), n)
    return out


@pytest.fixture(scope="module")
def runs():
    return {(m, sh): batches(m, sh) for m in (0, 1) for sh in (False, True)}


def test_the_recording_covers_what_it_was_made_for():
    assert DIMS == [2, 3, 5, 6, 15, 16, 17, 64, 128] and len(NAMES) == 13
    for n in NAMES:
        assert int(D[f"{n}/customers"]) <= 400 and set(D[f"{n}/kind"].tolist()) <= {0, 1, 2}, n
    assert set(D["exp2/kind"].tolist()) == {1} and set(D["uni2/kind"].tolist()) == {2}
    for n in ("mix5", "mix6", "rand15", "rand16", "rand17", "rand64", "rand128"):
        assert set(D[f"{n}/kind"].tolist()) == {0, 1, 2}, n
    assert (D["uni_neg/loc"] < 0).all() and float(D["uni_neg/end_time"]) < float(D["uni_neg/clock"])   # time ran back
    assert D["scale0_src/kind"][0] == 1 and D["scale0_src/scale"][0] == 0 and float(D["scale0_src/clock"]) == 0
    assert D["scale0_srv/kind"][1] == 2 and D["scale0_srv/scale"][1] == 0
    assert D["renege/reneges"].sum() > 50 and D["renege/max_queue"].max() == 1 == D["renege/queue_list"].max()


# ---- 1. libm: the reference's bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_libm_statistics_are_the_recording(runs, name, shuffled):
    got = runs[0, shuffled][name]
    for f in INTS:
        assert np.array_equal(got[f], D[f"{name}/{f}"]), (name, f)
    assert got["total_customers"] == D[f"{name}/total_customers"] and got["n_records"] == D[f"{name}/n_records"], name
    assert np.array_equal(got["is_source"], D[f"{name}/is_source"]) and got["stop_reason"] == 1, name
    for f in EVENT_ORDER:
        assert bits(got[f]) == bits(D[f"{name}/{f}"]), (name, f, got[f], D[f"{name}/{f}"])
    for f in ("queue_area", "queue_time"):
        r = ratio(got[f], D[f"{name}/{f}"])
        print(name, f, "max |lazy - recording| / max(1, |x|):", r)
        assert r <= BOUND_LAZY <= 1e-12, (name, f)


def test_metrics_of_the_recording(runs):
    """One division after the accumulators, as test_des_stats.py's metrics test: 3 x BOUND_LAZY."""
    seen = 0
    for dim in DIMS:
        names = dist_names_of_dim(dim)
        a, kind = dist_case_arrays(names)
        m = sv.metrics(sv.run_stats_host(*a, math=0, histogram=True, kind=kind))
        for b, n in enumerate(names):
            if not bool(D[f"{n}/has_metrics"]):
                continue
            seen += 1
            for name in sv.METRIC_NAMES:
                got, want = m[name][b], D[f"{n}/m_{name}"]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (n, name)
                ok = ~np.isnan(want)
                assert ratio(got[ok], want[ok]) <= 3 * BOUND_LAZY, (n, name)
    assert seen == 12


# ---- 2. portable math against libm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_portable_math_has_the_same_structure(runs, name):
    got, want = runs[1, False][name], runs[0, False][name]
    for f in INTS + ("total_customers", "n_records", "events", "stop_reason"):
        assert np.array_equal(got[f], want[f]), (name, f)
    assert same_state(got["state"], want["state"]), name
    for f in EVENT_ORDER + ("queue_area",):
        assert ratio(got[f], want[f]) <= 1e-12, (name, f)


# ---- 3. kind 0 is the existing entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("dim", CORPUS_DIMS)
def test_all_normal_kinds_are_the_existing_entry(dim, math):
    a = case_arrays(names_of_dim(dim))
    old = sv.run_stats_host(*a, math=math, histogram=True)
    new = sv.run_stats_host(*a, math=math, histogram=True, kind=np.zeros(a[1].shape, dtype=np.int32))
    for f in old._fields:
        assert bits(getattr(new, f)) == bits(getattr(old, f)), f


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_kind_out_of_range_refuses_the_host_call():
    a, kind = dist_case_arrays(["mix5"])
    for bad in (3, -1):
        k = kind.copy()
        k[0, 4] = bad
        with pytest.raises(_lib.GdmError, match="kind"):
            sv.run_stats_host(*a, math=1, kind=k)


@pytest.mark.parametrize("math", [0, 1])
def test_refused_samples_inside_a_batch(runs, math):
    names = ["uni_neg", "uni_neg", "uni_neg", "scale0_srv", "uni_neg", "scale0_src"]      # uni_neg: 0 -> 1 -> 2
    a, kind = dist_case_arrays(names)
    loc, scale = a[1].copy(), a[2].copy()
    scale[1, 2] = -0.5                                    # sample 1: scipy's "Domain error"
    kind[2, 1], scale[2, 1] = 1, 0.0                      # sample 2: an exponential server that only ever gives 0.0
    kind[4, 2], scale[4, 2], loc[4, 2] = 2, 0.0, 0.0      # sample 4: a uniform server that only ever gives loc = 0
    st = sv.run_stats_host(a[0], loc, scale, *a[3:], math=math, histogram=True, kind=kind)
    assert st.stop_reason.tolist() == [1, ERROR, ERROR, 1, ERROR, 1]
    for b in (1, 2, 4):
        for f in sv.STATS_NODE_FIELDS + ("clock", "end_time", "total_customers", "events", "n_records"):
            assert not np.asarray(getattr(st, f)[b]).any(), (b, f)
        assert not st.queue_time[b].any() and same_state(sv.state_of(st, b), dist_state0(names[b])), b
    for b in (0, 3, 5):
        want = runs[math, False][names[b]]
        got = cut(sample(st, b), names[b])
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("queue_time",):
            assert bits(got[f]) == bits(want[f]), (b, f)
        assert same_state(got["state"], want["state"])


def test_a_uniform_that_is_never_positive_ends_on_the_draw_budget():
    a, kind = dist_case_arrays(["uni2"])
    loc = a[1].copy()
    loc[0, 1] = -2.0                                      # the server: uniform on [-2, -1]
    st = sv.run_stats_host(a[0], loc, *a[2:], math=1, max_events=40, kind=kind)
    assert st.stop_reason.tolist() == [BUDGET] and st.served[0, 1] == 0 and st.events[0] >= 1


# ---- 5. argument checks ----------------------------------------------------------------------------------------------
def test_dist_entries_validate_on_the_host():
    lib = _lib.load()
    b, dim, cap = 2, 5, 4
    need = lib.gdm_des_stats_workspace_bytes(b, dim, cap)
    buf = np.zeros(need + 64, dtype=np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    arrays = [np.zeros(4096, dtype=np.float64) for _ in range(27)]
    ptrs = [a.ctypes.data for a in arrays]
    kind = np.zeros(b * dim + 1, dtype=np.int32)

    def call(dim=dim, cap=cap, ptrs=ptrs, kind=kind.ctypes.data, hist=None, ws=base, ws_bytes=need, max_events=1000):
        args = [ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:6], cap, max_events, *ptrs[6:24], hist, ws, ws_bytes, None]
        return lib.gdm_des_stats_batch_dist(*args), lib.gdm_last_error()

    for missing in (0, 2, 3, 9, 10, 17, 23):
        rc, msg = call(ptrs=[None if i == missing else p for i, p in enumerate(ptrs)])
        assert rc == -1 and b"gdm_des_stats_batch_dist: null pointer" in msg, missing
    for kw, word in ((dict(kind=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=base + 8), b"workspace"), (dict(dim=129), b"dim"),
                     (dict(cap=0), b"max_queue_cap"), (dict(max_events=0), b"max_events"),
                     (dict(ptrs=[ptrs[0] + 4] + ptrs[1:]), b"aligned"), (dict(kind=kind.ctypes.data + 2), b"aligned"),
                     (dict(hist=ptrs[24] + 2), b"aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)

    def host(ptrs=ptrs, kind=kind.ctypes.data, math=1, max_events=1000):
        return (lib.gdm_des_stats_batch_dist_host(ptrs[0], b, dim, *ptrs[1:3], kind, *ptrs[3:6], cap, math, max_events,
                                                  *ptrs[6:24], None), lib.gdm_last_error())

    for kw, word in ((dict(kind=None), b"null pointer"), (dict(ptrs=[None] + ptrs[1:]), b"null pointer"),
                     (dict(math=2), b"math"), (dict(max_events=0), b"max_events")):
        rc, msg = host(**kw)
        assert rc == -1 and b"gdm_des_stats_batch_dist_host" in msg and word in msg, (kw, msg)
    kind[7] = 3
    rc, msg = host()
    assert rc == -1 and b"kind 3 at sample 1, node 2" in msg


def test_ops_refuse_cpu_tensors():
    import torch
    z = torch.zeros
    with pytest.raises(ops.GdmError):
        ops.des_run_stats_dist(z(1, 2, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64),
                               z(1, 2, dtype=torch.float64), z(1, 2, dtype=torch.int32), z(1, 2, dtype=torch.int32),
                               z(1, dtype=torch.int64), z(1, dtype=torch.int64), z(1, 624, dtype=torch.int32),
                               z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.float64),
                               max_queue_cap=4)


# ---- 6. closed forms -------------------------------------------------------------------------------------------------
def test_mm1k():
    for lam, mu, cap in ((0.8, 1.0, 3), (1.5, 1.0, 2), (1.0, 1.0, 5), (0.3, 2.0, 0), (2.0, 0.5, 7)):
        t = qt.mm1k(lam, mu, cap)
        k = cap + 1
        assert t["p"].shape == (k + 1,) and abs(t["p"].sum() - 1) <= 4e-16 and (t["p"] > 0).all()
        assert t["blocking"] == t["p"][k] and abs(t["utilisation"] - (1 - t["p"][0])) <= 1e-16
        assert t["queue_length_probabilities"].shape == (cap + 1,) and abs(t["queue_length_probabilities"].sum() - 1) <= 4e-16
        # balance: accepted arrivals leave through the server; Little's law on the queue
        assert abs(lam * (1 - t["blocking"]) - mu * t["utilisation"]) <= 1e-15 * max(lam, mu)
        assert abs(t["L"] - (t["LQ"] + t["utilisation"])) <= 1e-14 * max(1.0, t["L"])
        assert abs(t["WQ"] * lam * (1 - t["blocking"]) - t["LQ"]) <= 1e-14 * max(1.0, t["LQ"])
        assert abs(qt.mmck_blocking(lam, mu, 1, cap) - t["blocking"]) <= 1e-15
    t = qt.mm1k(1.0, 1.0, 4)
    assert np.array_equal(t["p"], np.full(6, 1 / 6)) and t["L"] == 2.5                       # rho == 1: uniform
    assert abs(qt.mm1k(0.8, 1.0, 3)["blocking"] - 0.8 ** 4 * 0.2 / (1 - 0.8 ** 5)) <= 1e-16   # the textbook form
    # Erlang B (no waiting room), c = 2, a = 1: (1/2) / (1 + 1 + 1/2)
    assert abs(qt.mmck_blocking(1.0, 1.0, 2, 0) - 0.2) <= 1e-16
    with pytest.raises(ValueError):
        qt.mm1k(0.0, 1.0, 1)


def test_traffic_rates():
    from gan_des_midi_music_gen_amd.matrix_sim_process import DesSpec

    def spec(adj, dist):
        n = len(dist)
        return DesSpec(np.array(adj, dtype=np.float64), dist, [3] * n, np.array([1]), 10, 1.0, np.zeros(n), np.zeros(n))

    # a tandem: source (rate 2) -> 1 -> 2
    tandem = spec([[1, 1, 0], [0, -1, 1], [0, 0, 0]], [["exponential", 0.5], ["exponential", 0.1], ["uniform", 0.0, 0.2]])
    assert np.allclose(qt.traffic_rates(tandem), [2.0, 2.0, 2.0], rtol=1e-15)
    # a feedback loop: source (mean 4: rate 1/4) -> 1; 1 -> 2 w.p. 1/2, back to 1 w.p. 1/2 over 3: lam1 = 1/4 + lam3,
    # lam3 = lam1 / 2 -> lam1 = 1/2, lam2 = lam3 = 1/4
    loop = spec([[1, 1, 0, 0], [0, -1, 0.5, 0.5], [0, 0, 0, 0], [0, 1, 0, -1]],
                [["normal", 4.0, 1.0], ["exponential", 1.0], ["exponential", 1.0], ["uniform", 0.5, 1.0]])
    assert np.allclose(qt.traffic_rates(loop), [0.25, 0.5, 0.25, 0.25], rtol=1e-15)
    closed = spec([[1, 1, 0], [0, -1, 1], [0, 1, -1]], [["exponential", 1.0]] * 3)
    with pytest.raises(ValueError, match="singular"):
        qt.traffic_rates(closed)
    assert qt.mean_of(["uniform", 0.5, 1.0]) == 1.0
    with pytest.raises(NotImplementedError):
        qt.mean_of(["gamma", 1.0, 0.0, 1.0])


# ---- 7. the sweep beside theory --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_sweep():
    cfg = D["grid/config"]
    return sv.mm1k_sweep(cfg[:, 0], cfg[:, 1], cfg[:, 2].astype(int), D["grid/seeds"], customers=int(D["grid/customers"]),
                         math=0)


def test_sweep_runs_are_the_recorded_reference_runs(grid_sweep):
    st = grid_sweep.stats
    assert D["grid/config"].shape == (6, 3) and len(D["grid/seeds"]) == 16 and st.served.shape == (96, 2)
    assert (st.stop_reason == 1).all()
    for f in INTS + ("total_customers",):
        assert np.array_equal(getattr(st, f), D[f"grid/{f}"]), f
    for f in EVENT_ORDER:
        assert bits(getattr(st, f)) == bits(D[f"grid/{f}"]), f
    for f in ("queue_area", "queue_time"):
        r = ratio(getattr(st, f), D[f"grid/{f}"])
        print(f, "max |lazy - recording| / max(1, |x|):", r)
        assert int(D["grid/customers"]) == 4000 and r <= GRID_LAZY <= 4e-12, f


def check_z(sweep, n_runs):
    worst, count = 0.0, 0
    for name in sv.SWEEP_NAMES:
        z, th = sweep.z[name], sweep.theory[name]
        assert (sweep.n[name][~np.isnan(th)] == n_runs).all(), name
        assert np.array_equal(np.isnan(z), np.isnan(th)), name
        for c in np.argwhere(~np.isnan(th)):
            c = tuple(c)
            print(f"config {c[0]} {name}{[int(j) for j in c[1:]]} mean {sweep.mean[name][c]:.5f} sem {sweep.sem[name][c]:.5f} "
                  f"theory {th[c]:.5f} z {z[c]:+.2f}")
        worst, count = max(worst, float(np.nanmax(np.abs(z)))), count + int((~np.isnan(th)).sum())
        assert (np.abs(z[~np.isnan(th)]) <= Z_BOUND).all(), (name, z)
    return worst, count


def test_sweep_agrees_with_theory(grid_sweep):
    worst, count = check_z(grid_sweep, 16)
    assert count == 6 * 4 + sum(int(c) + 1 for c in D["grid/config"][:, 2]) == 50
    assert abs(worst - float(D["grid/max_abs_z"])) <= 1e-9          # the same runs: the recording's own largest |z|


# ---- 8. the public surface -------------------------------------------------------------------------------------------
def test_run_stats_and_replicate_take_the_new_kinds():
    assert sv.DIST_KINDS == ("normal", "exponential", "uniform")
    spec = sv.mm1k_spec(0.8, 1.0, 3, 300, seed=7)
    adj, kind, loc, scale, qcap, seed, customers = sv.dist_arrays([spec])
    assert kind.tolist() == [[1, 1]] and loc.tolist() == [[0.0, 0.0]] and scale.tolist() == [[1.25, 1.0]]
    state = np.random.RandomState(5).get_state()
    st = sv.run_stats([spec], states=[state], histogram=True)
    want = sv.run_stats_host(adj, loc, scale, qcap, seed, customers, [state], math=1, histogram=True, kind=kind)
    for f in st._fields:
        assert bits(getattr(st, f)) == bits(getattr(want, f)), f
    assert st.stop_reason[0] == 1 and st.served[0, 1] > 200 and st.reneges[0, 1] > 0
    rep = sv.replicate(spec, [1, 2, 3, 4])
    assert rep.valid.all() and rep.n["server_utilizations"][1] == 4 and 0.4 < rep.mean["server_utilizations"][1] < 0.95
    uni = sv.mm1k_spec(0.8, 1.0, 3, 100)
    uni.distributions = [["uniform", 0.5, 1.0], ["normal", 0.5, 0.1]]
    assert sv.dist_arrays([uni])[1].tolist() == [[2, 0]] and sv.dist_arrays([uni])[2].tolist() == [[0.5, 0.5]]
    uni.distributions = [["gamma", 2.0, 0.0, 1.0], ["normal", 0.5, 0.1]]
    for f in (lambda: sv.dist_arrays([uni]), lambda: sv.run_stats([uni]), lambda: sv.replicate(uni, [1])):
        with pytest.raises(NotImplementedError, match="gamma"):
            f()
    # the logging surface keeps refusing
    with pytest.raises(NotImplementedError):
        sv.spec_arrays([spec])
    with pytest.raises(NotImplementedError):
        sv.run_batch([spec])
    with pytest.raises(NotImplementedError):
        sv.Sim(spec.sim_matrix, spec.distributions, spec.queue_list, seeds=[1], logging_mode='Music')


def test_all_normal_specs_take_the_existing_entries(monkeypatch):
    """run_stats routes to the _dist entries only when some node is not normal."""
    from test_des_stats import corpus_spec
    called = []
    real = sv.run_stats_host
    monkeypatch.setattr(sv, "run_stats_host", lambda *a, **k: (called.append(k.get("kind")), real(*a, **k))[1])
    sv.run_stats([corpus_spec("q_wrap3")])
    sv.replicate(corpus_spec("q_wrap3"), [1, 2])
    sv.run_stats([sv.mm1k_spec(0.8, 1.0, 3, 50)])
    assert called[0] is None and called[1] is None and called[2] is not None


# ---- 9. the policy as a stand-alone program under the host sanitizers ------------------------------------------------
def stand_alone_cases():
    """(label, adj, loc, scale, kind, qcap, seed, customers, state): the three kinds in one net, service times drawn
    again and time running backwards, scale 0, and a spec refused before anything runs (kind 3)."""
    out = []
    for n in ("mix5", "uni_neg", "scale0_srv", "mix6"):
        (adj, loc, scale, qcap, seed, cust, states), kind = dist_case_arrays([n])
        if n == "mix6":
            kind = kind.copy()
            kind[0, 5] = 3
            n = "refused"
        out.append((n, adj[0], loc[0], scale[0], kind[0].astype(np.int32), qcap[0].astype(np.int32), int(seed[0]),
                    int(cust[0]), states[0]))
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of tools/des_dist_host.cpp "
                    "did not run")
    cases = stand_alone_cases()
    exe, cases_bin, stats_bin = str(tmp_path / "des_dist_host"), str(tmp_path / "cases.bin"), str(tmp_path / "stats.bin")
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
                            os.path.join(ROOT, "tools", "des_dist_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases_bin, stats_bin], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    with open(stats_bin, "rb") as f:
        for n, adj, loc, scale, kind, qcap, seed, cust, st in cases:
            dim = adj.shape[0]
            if n == "refused":                            # the host ENTRY refuses the call: the device's rule is the header's
                want = None
            else:
                want = sv.run_stats_host(adj[None], loc[None], scale[None], qcap[None], [seed], [cust], [st], math=1,
                                         histogram=True, kind=kind[None])
            reason, has, pos, stride, total, events, n_rec, gauss, clock, end = struct.unpack("<iiiiqqqddd", f.read(64))
            rows = {}
            for field, dt in (("served", "<i8"), ("reneges", "<i8"), ("generated", "<i8"), ("max_queue", "<i4"),
                              ("time_in_service", "<f8"), ("time_in_queue", "<f8"), ("queue_area", "<f8"),
                              ("arrival_time", "<f8")):
                rows[field] = np.frombuffer(f.read(np.dtype(dt).itemsize * dim), dtype=dt)
            qtime = np.frombuffer(f.read(8 * dim * (stride + 1)), dtype="<f8").reshape(dim, stride + 1)
            key = np.frombuffer(f.read(4 * 624), dtype="<u4")
            assert stride == int(qcap.max()), n
            if want is None:
                assert reason == ERROR and (total, events, n_rec) == (0, 0, 0) and clock == 0 and end == 0
                assert not any(r.any() for r in rows.values()) and not qtime.any()
                assert same_state(("MT19937", key, pos, has, gauss), st)
                continue
            assert reason == want.stop_reason[0] == 1 and want.served.sum() > 50, n
            assert (total, events, n_rec) == (want.total_customers[0], want.events[0], want.n_records[0]), n
            assert bits(np.float64(clock)) == bits(want.clock[0]) and bits(np.float64(end)) == bits(want.end_time[0]), n
            for field, got in rows.items():
                assert bits(got) == bits(getattr(want, field)[0]), (n, field)
            assert bits(qtime) == bits(want.queue_time[0][:, :stride + 1]), n
            assert same_state(("MT19937", key, pos, has, gauss), sv.state_of(want, 0)), n
        assert f.read() == b""
