"""The discrete-event simulator's three host builds of csrc/des_sim.h against tests/golden/des_corpus.npz: the REFERENCE's
own Sim ('Music' mode) recorded by tests/golden/make_golden.py des_corpus on 45 small nets, each built for one branch of
the event logic -- ties between distinct events (Python's heapq order), queue capacities 0..3 and a wrapping ring, both
routing branches with 1..7 children, the three kinds of sink, redrawn services, a clock that runs backwards, a cached
gauss, every way a run stops, dims 1..128 -- with the witnesses, taken from the reference's objects and its log, that
the branch was reached.  Runs without a GPU.

  * simulation_v3.Sim (gdm_des_run, libm): records and the WHOLE final global generator state equal the recording;
  * run_batch_host(math=0, max_records=0): the same, cases of one dim stacked into one batch, in file order and shuffled;
  * run_batch_host(math=1), what the device runs: same kinds, nodes, event ids, counts, stop reasons, final states; the
    deterministic (tie) cases equal in value bit for bit; the rest within |d| <= BOUND * max(1, |t|), BOUND = 10 x the
    worst ratio measured against the recording on this corpus: 2.13e-16 measured (route_u7), bound 2.13e-15 (the
    runs are short: des_core.npz's, 5000 to 90 000 records long, reach 7.7e-14 relative);
  * the stored witnesses cover the catalogue, one assertion per branch naming the case that provides it;
  * the two error cases: the reference raises KeyError for both (recorded), Sim.run raises ValueError here, a batch
    sample ends with stop reason 3 and no records, its neighbours equal their recordings;
  * tools/des_corpus_host.cpp, the same header as a stand-alone program with exactly sized buffers, built with the host
    compiler's address and undefined-behaviour sanitizers and run as a child process, gives run_batch_host(math=1)'s
    records (2.3 s to build, 0.03 s to run where this was written)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import simulation_v3 as sv
from helpers import load_golden

G = load_golden("des_corpus.npz")
NAMES = [str(n) for n in G["names"]]
ERRORS = {"err_to_source": "KeyError",          # reference: self.servers[evt.get_server_id()] in Sim.run (line 473)
          "err_source_childless": "KeyError"}   # reference: the source's destination is None -> self.servers[None]
GOOD = [n for n in NAMES if str(G[f"{n}/error"]) == ""]
DETERMINISTIC = [n for n in GOOD if (G[f"{n}/dist"][:, 1] == 0).all()]
DIMS = sorted({int(G[f"{n}/sim_matrix"].shape[0]) for n in NAMES})
REL_MEASURED = 2.13e-16         # max |portable - recording| / max(1, |recording|) over the corpus (route_u7)
BOUND = 10 * REL_MEASURED
ERROR = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def names_of_dim(dim, names=NAMES):
    return [n for n in names if G[f"{n}/sim_matrix"].shape[0] == dim]


def state0(name):
    """The global generator state the recording started from."""
    if f"{name}/state0_key" in G.files:
        pos, has = (int(x) for x in G[f"{name}/state0_rest"])
        return ("MT19937", G[f"{name}/state0_key"].copy(), pos, has, float(G[f"{name}/state0_gauss"]))
    return np.random.RandomState(int(G[f"{name}/np_seed"])).get_state()


def final_state(name):
    pos, has = (int(x) for x in G[f"{name}/final_rest"])
    return ("MT19937", G[f"{name}/final_key"], pos, has, float(G[f"{name}/final_gauss"]))


def same_state(a, b):
    return (np.array_equal(np.asarray(a[1], dtype=np.uint32), np.asarray(b[1], dtype=np.uint32))
            and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3])
            and np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes())


def case_arrays(names, states=None, seed_index=0):
    """(adj, loc, scale, queue_cap, seed, customers, states) of corpus cases of one dim, as run_batch_host takes them."""
    return (np.stack([G[f"{n}/sim_matrix"] for n in names]), np.stack([G[f"{n}/dist"][:, 0] for n in names]),
            np.stack([G[f"{n}/dist"][:, 1] for n in names]), np.stack([G[f"{n}/queue_list"] for n in names]),
            np.array([int(G[f"{n}/seeds"][seed_index if len(G[f"{n}/seeds"]) > 1 else 0]) for n in names]),
            np.array([int(G[f"{n}/customers"]) for n in names]),
            [state0(n) for n in names] if states is None else states)


def recording(name):
    out = np.empty(len(G[f"{name}/value"]), dtype=sv.EVENT_DTYPE)
    for f in ("value", "event_id", "node", "kind"):
        out[f] = G[f"{name}/{f}"]
    return out


def n_seeds(name):
    return len(G[f"{name}/seeds"])


@pytest.fixture(scope="module")
def stacked():
    """math -> name -> (records, stop reason, final state) of the corpus batched by dim in file order (computed once).
    A case with two seeds is two runs: the second starts from the state the first left."""
    out = {0: {}, 1: {}}
    for m in (0, 1):
        for dim in DIMS:
            names = names_of_dim(dim)
            log = sv.run_batch_host(*case_arrays(names), math=m, max_records=0)
            assert log.rec_ptr.tolist() == [0] + np.cumsum(log.n_records).tolist()
            for b, n in enumerate(names):
                recs, reason, state = sv.sample_log(log, b), int(log.stop_reason[b]), sv.state_of(log, b)
                if n_seeds(n) > 1:
                    more = sv.run_batch_host(*case_arrays([n], [state], seed_index=1), math=m, max_records=0)
                    recs = np.concatenate([recs, sv.sample_log(more, 0)])
                    reason, state = int(more.stop_reason[0]), sv.state_of(more, 0)
                out[m][n] = (recs, reason, state)
    return out


# ---- the three host builds against the recording ---------------------------------------------------------------------
@pytest.mark.parametrize("name", GOOD)
def test_sim_is_the_recording(name):
    d = G[f"{name}/dist"]
    dist = [["normal", np.float32(a), np.float32(b)] for a, b in d]
    assert all(float(x[1]) == a and float(x[2]) == b for x, (a, b) in zip(dist, d))
    sim = sv.Sim(G[f"{name}/sim_matrix"], dist, list(G[f"{name}/queue_list"]), seeds=G[f"{name}/seeds"],
                 generate_log=False, animation=False, record_history=False, logging_mode='Music', max_sim_time=1.0)
    keep = np.random.get_state()
    try:
        np.random.set_state(state0(name))
        log = sim.run(number_of_customers=int(G[f"{name}/customers"]))
        after = np.random.get_state()
    finally:
        np.random.set_state(keep)
    want = recording(name)
    assert len(log) == len(want)
    for f in ("kind", "node", "event_id"):
        assert np.array_equal(log[f], want[f]), f
    assert np.array_equal(log["value"].view(np.int64), want["value"].view(np.int64))
    assert same_state(after, final_state(name)), "global numpy stream after the run"


@pytest.mark.parametrize("name", GOOD)
def test_libm_batch_is_the_recording(stacked, name):
    recs, reason, state = stacked[0][name]
    want = recording(name)
    assert len(recs) == len(want) and reason in (0, 1)
    assert reason == (0 if not G[f"{name}/w_is_source"].any() else 1)
    assert recs.tobytes() == want.tobytes()
    assert same_state(state, final_state(name))


@pytest.mark.parametrize("m", [0, 1])
def test_no_sample_depends_on_its_position(stacked, m):
    rs = np.random.RandomState(17)
    for dim in DIMS:
        names = names_of_dim(dim)
        if len(names) < 2:
            continue
        order = [names[i] for i in rs.permutation(len(names))] + [names[0]]
        log = sv.run_batch_host(*case_arrays(order), math=m, max_records=0)
        for b, n in enumerate(order):
            first = stacked[m][n][0] if n_seeds(n) == 1 else stacked[m][n][0][:int(log.n_records[b])]
            assert sv.sample_log(log, b).tobytes() == first.tobytes(), (dim, n)
            if n_seeds(n) == 1:
                assert same_state(sv.state_of(log, b), stacked[m][n][2]), (dim, n)


def portable_ratio(name, recs):
    want = G[f"{name}/value"]
    if len(want) == 0:
        return 0.0
    return float((np.abs(recs["value"] - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.parametrize("name", GOOD)
def test_portable_math_keeps_the_event_structure(stacked, name):
    recs, reason, state = stacked[1][name]
    want = recording(name)
    assert len(recs) == len(want) and reason == stacked[0][name][1]
    for f in ("kind", "node", "event_id"):
        assert np.array_equal(recs[f], want[f]), f
    assert same_state(state, final_state(name))
    ratio = portable_ratio(name, recs)
    print(name, "max |portable - recording| / max(1, |t|):", ratio)
    if name in DETERMINISTIC:
        assert np.array_equal(recs["value"].view(np.int64), want["value"].view(np.int64))
    else:
        assert ratio <= BOUND < 1e-11


def test_the_measured_ratio_is_the_documented_one(stacked):
    """The figure in the module docstring and in DESIGN.md section 7: within a factor 2 of what this build gives (the
    bound itself is fixed above, not taken from this run)."""
    worst = max((portable_ratio(n, stacked[1][n][0]), n) for n in GOOD)
    print("worst portable / recording ratio:", worst)
    assert len(DETERMINISTIC) >= 5 and worst[0] <= 2 * REL_MEASURED


# ---- the corpus still reaches every branch ---------------------------------------------------------------------------
def w(name, key):
    return G[f"{name}/w_{key}"]


def test_witnesses_cover_the_catalogue():
    cap = lambda n: G[f"{n}/queue_list"]                           # noqa: E731
    scale = lambda n: G[f"{n}/dist"][:, 1]                         # noqa: E731
    loc = lambda n: G[f"{n}/dist"][:, 0]                           # noqa: E731
    assert len(NAMES) <= 60 and sum(len(G[f"{n}/value"]) for n in GOOD) < 40000
    for n in GOOD:                                                  # the condition the structural comparison rests on
        assert w(n, "min_gap") > 1e-9, n
    # ties between DISTINCT events
    for n in ("tie_a", "tie_b", "tie_d16", "tie_d65", "tie_e"):
        assert w(n, "ties") >= 20 and n in DETERMINISTIC, n
    assert w("tie_c", "ties") >= 20 and "tie_c" not in DETERMINISTIC and (scale("tie_c") == 0).sum() >= 3
    assert w("tie_d16", "group") >= 12 and G["tie_d16/sim_matrix"].shape[0] == 16
    assert w("tie_d65", "group") >= 12 and G["tie_d65/sim_matrix"].shape[0] == 65
    assert (loc("tie_b")[:3].tolist() == [0.25, 0.5, 0.75]) and loc("tie_e")[0] == float(np.float32(0.3))
    # queues
    for n, c in (("q_cap0", 0), ("q_cap1", 1), ("q_cap2", 2)):
        node = int(np.argmax(w(n, "reneges")))
        assert w(n, "reneges")[node] > 0 and cap(n)[node] == c, n
    assert sorted(set(cap("q_mix")[w("q_mix", "reneges") > 0].tolist())) == [0, 2]
    assert ((cap("q_wrap3") == 3) & (w("q_wrap3", "from_queue") >= 20)).any()
    # routing
    for n, k in (("route_u2", 2), ("route_u5", 5), ("route_u6", 6), ("route_u7", 7)):
        assert ((w(n, "uniform") == 1) & (w(n, "n_children") == k)).any(), n
    for n, k in (("route_p", 2), ("route_p7", 7)):
        assert ((w(n, "uniform") == 0) & (w(n, "n_children") == k)).any(), n
    assert ((w("route_single", "uniform") == 0) & (w("route_single", "n_children") == 1)).sum() >= 2
    assert not ((w("route_single", "uniform") == 1) & (w("route_single", "n_children") == 1)).any()   # p / p == 1: always p=
    off = G["route_neg/sim_matrix"][~np.eye(6, dtype=bool)]
    assert (off < 0).sum() >= 4 and len(G["route_neg/value"]) > 100
    src = w("route_interleave", "is_source")
    assert src[0] == 1 and src[-1] == 1 and src[1] == 0 and src[2] == 1 and w("route_interleave", "reneges").max() > 0
    # sinks
    assert ((w("tie_a", "is_sink") == 1) & (w("tie_a", "n_children") == 0)).any()                      # childless
    s0 = w("sink_node0_server", "is_sink")
    assert ((s0 == 1) & (w("sink_node0_server", "n_children") == 1)).any() and s0[0] == 1
    assert G["sink_node0_server/sim_matrix"][1, 0] > 0
    assert w("sink_node0_source", "is_source")[3] == 1 and G["sink_node0_source/sim_matrix"][3, 0] > 0
    assert w("sink_node0_source", "n_children")[3] == 1 and w("sink_node0_source", "is_sink")[0] == 0
    # draws
    assert w("draw_redraw", "redraw_services") >= 50 and w("draw_redraw", "redraw_share") >= 0.5
    assert bool(w("draw_backwards", "backwards")) and not any(bool(w(n, "backwards")) for n in DETERMINISTIC)
    z = scale("draw_scale0") == 0
    assert (z & (w("draw_scale0", "is_source") == 1)).any() and (z & (w("draw_scale0", "is_source") == 0)).any()
    assert G["draw_cached_gauss/state0_rest"][1] == 1 and G["draw_cached_gauss/final_rest"][1] == 1
    assert G["draw_cached_gauss/final_gauss"].tobytes() == G["draw_cached_gauss/state0_gauss"].tobytes()
    # stops (two sources: nothing is processed up to number_of_customers = 2)
    assert [int(G[f"stop_n{n}/customers"]) for n in range(5)] == [0, 1, 2, 3, 4]
    assert [len(G[f"stop_n{n}/value"]) > 0 for n in range(5)] == [False, False, False, True, True]
    assert int(w("stop_n0", "is_source").sum()) == 2
    assert len(G["stop_nosrc/value"]) == 0 and not w("stop_nosrc", "is_source").any()
    assert n_seeds("stop_two_seeds") == 2 and int((G["stop_two_seeds/event_id"] == 0).sum()) >= 4
    # sizes
    assert DIMS == [1, 2, 3, 5, 6, 15, 16, 17, 64, 65, 128]
    for d in (2, 3, 15, 16, 17, 64, 65, 128):
        assert len(G[f"size_{d}/value"]) > 100 and G[f"size_{d}/sim_matrix"].shape[0] == d
    assert w("size_65", "is_source")[64] == 1 and w("size_128", "is_source")[64:].any()
    served = np.bincount(G["size_128/node"][G["size_128/kind"] == 2], minlength=128)
    assert (served[64:] > 0).any() and (served[:64] > 0).any()
    # errors
    assert {n: str(G[f"{n}/error"]) for n in NAMES if str(G[f"{n}/error"])} == ERRORS


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_error_cases_raise_and_stop_alone(stacked, name):
    assert str(G[f"{name}/error"]) == ERRORS[name]
    d = G[f"{name}/dist"]
    sim = sv.Sim(G[f"{name}/sim_matrix"], [["normal", a, b] for a, b in d], list(G[f"{name}/queue_list"]),
                 seeds=G[f"{name}/seeds"], logging_mode='Music')
    keep = np.random.get_state()
    try:
        np.random.set_state(state0(name))
        with pytest.raises(ValueError):
            sim.run(number_of_customers=int(G[f"{name}/customers"]))
    finally:
        np.random.set_state(keep)
    for m in (0, 1):
        recs, reason, _state = stacked[m][name]
        assert reason == ERROR and len(recs) == 0
    names = ["q_cap1", name, "stop_n4", name, "tie_a"]
    log = sv.run_batch_host(*case_arrays(names), math=0, max_records=0)
    assert log.stop_reason.tolist()[1::2] == [ERROR, ERROR] and log.n_records.tolist()[1::2] == [0, 0]
    for b in (0, 2, 4):
        assert sv.sample_log(log, b).tobytes() == recording(names[b]).tobytes()
        assert same_state(sv.state_of(log, b), final_state(names[b]))


def test_the_error_table_is_documented():
    for name, exc in ERRORS.items():
        assert exc in sv.__doc__ and "ValueError" in sv.__doc__, name


# ---- the same header as a stand-alone program under the host sanitizers ----------------------------------------------
def dump_cases(path, names, expected):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        for n in names:
            st = state0(n)
            dim = G[f"{n}/sim_matrix"].shape[0]
            f.write(struct.pack("<iiiiqqqqd", dim, int(st[3]), int(st[2]), 0, int(G[f"{n}/seeds"][0]),
                                int(G[f"{n}/customers"]), 200000, len(expected[n]), float(st[4])))
            f.write(np.ascontiguousarray(G[f"{n}/sim_matrix"], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(G[f"{n}/dist"][:, 0], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(G[f"{n}/dist"][:, 1], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(G[f"{n}/queue_list"], dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(st[1], dtype="<u4").tobytes())


def read_records(path, names):
    out = {}
    with open(path, "rb") as f:
        for n in names:
            reason, has, pos, overflow, n_out, n_stored, gauss = struct.unpack("<iiiiqqd", f.read(40))
            recs = np.empty(n_stored, dtype=sv.EVENT_DTYPE)
            recs["value"] = np.frombuffer(f.read(8 * n_stored), dtype="<f8")
            recs["event_id"] = np.frombuffer(f.read(8 * n_stored), dtype="<i8")
            recs["node"] = np.frombuffer(f.read(4 * n_stored), dtype="<i4")
            recs["kind"] = np.frombuffer(f.read(4 * n_stored), dtype="<i4")
            key = np.frombuffer(f.read(4 * 624), dtype="<u4")
            out[n] = (recs, reason, ("MT19937", key, pos, has, gauss), n_out, overflow)
        assert f.read() == b""
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of tools/des_corpus_host.cpp "
                    "did not run")
    # each case alone, from its recorded state (the first seed of a two-seed case), uncapped
    expected, states, reasons = {}, {}, {}
    for n in NAMES:
        log = sv.run_batch_host(*case_arrays([n]), math=1, max_records=0)
        expected[n], states[n], reasons[n] = sv.sample_log(log, 0), sv.state_of(log, 0), int(log.stop_reason[0])
    exe, cases, records = str(tmp_path / "des_corpus_host"), str(tmp_path / "cases.bin"), str(tmp_path / "records.bin")
    dump_cases(cases, NAMES, expected)
    # the runtimes linked statically: gcc's shared one refuses to start in a process that has any other library preloaded
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                            "-I", os.path.join(ROOT, "gan_des_midi_music_gen_amd", "csrc"),
                            os.path.join(ROOT, "tools", "des_corpus_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases, records], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    got = read_records(records, NAMES)
    for n in NAMES:
        recs, reason, state, n_out, overflow = got[n]
        assert reason == reasons[n], n
        if n in ERRORS:
            # the arrival that precedes the error found no room (out_len 0) and was dropped, not written
            assert reason == ERROR and len(recs) == 0, n
            continue
        assert n_out == len(expected[n]) and not overflow, n
        assert recs.tobytes() == expected[n].tobytes(), n
        assert same_state(state, states[n]), n
