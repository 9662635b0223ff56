"""Exponential and uniform nodes in the LOGGING run (des::Sim<Math, OutSoa, NoStats, AnyDist> in csrc/des_sim.h, behind
gdm_des_run_batch_dist_host) against tests/golden/des_log_dist.npz: the 'Music' logs of the REFERENCE's own Sim on the 13
nets of des_dist.npz, recorded by tests/golden/make_des_log_dist_golden.py.  Runs without a GPU.

  1. math=0 (libm, numpy's bits): run_batch_host(kind=...) reproduces the reference's log record for record and bit
     for bit in `value`, and leaves numpy's recorded stream position (and key); cases of one dim stacked into one
     batch, in file order and shuffled.
  2. math=1 (portable, what the device runs): the same event structure; `value` within 1e-12 relative (floor 1), the
     bound tests/test_des_dist.py::test_portable_math_has_the_same_structure holds the statistics run to.
  3. all-normal kinds give the bytes of gdm_des_run_batch_host at dims 2, 15, 16, 64 and 128, both maths; kind=None
     calls the old symbol; run_batch_dist routes to the entries with kinds only when some node is not normal.
  4. refusals inside a batch: scale < 0, an exponential server with scale 0, a uniform server with scale 0 and loc <= 0
     -- reason 3, an empty log, the generator state kept, neighbours untouched; a kind outside 0..2 refuses the host
     call; Sim, run_batch and spec_arrays still raise.
  5. max_records cuts a dist log at the cap with reason 4; GDM_EWORKSPACE reports the count and a second call from the
     original states succeeds.
  6. write_music_log writes mix5 as the reference's log text; Sim.run's file is what it was.
  7. tools/des_log_dist_host.cpp, the logging policy and the track loop as a stand-alone program under the host
     compiler's sanitizers, agrees with the library."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import _lib, simlog_to_vid as sl, simulation_v3 as sv
from helpers import load_golden
from test_des_corpus import case_arrays, names_of_dim, same_state
from test_des_dist import D, DIMS, ERROR, NAMES, dist_case_arrays, dist_names_of_dim, dist_state0
from test_des_stats import ROOT, bits, corpus_spec, ratio

L = load_golden("des_log_dist.npz")
RECORDS = 4
FIELDS = ("value", "event_id", "node", "kind")
PORTABLE_BOUND = 1e-12                                   # test_des_dist.py::test_portable_math_has_the_same_structure


def batches(math, shuffled):
    """name -> (records of the sample, stop reason, final state), cases of one dim in one call."""
    out, rs = {}, np.random.RandomState(31)
    for dim in DIMS:
        names = dist_names_of_dim(dim)
        if shuffled and len(names) > 1:
            names = [names[i] for i in rs.permutation(len(names))] + [names[0]]
        a, kind = dist_case_arrays(names)
        log = sv.run_batch_host(*a, math=math, max_records=0, kind=kind)
        for b, n in enumerate(names):
            out[n] = (sv.sample_log(log, b), int(log.stop_reason[b]), sv.state_of(log, b))
    return out


@pytest.fixture(scope="module")
def runs():
    return {(m, sh): batches(m, sh) for m in (0, 1) for sh in (False, True)}


def test_the_recording_is_the_statistics_recordings_runs():
    assert [str(n) for n in L["names"]] == NAMES and len(NAMES) == 13
    total = 0
    for n in NAMES:
        assert len(L[f"{n}/value"]) == int(D[f"{n}/n_records"]), n
        total += len(L[f"{n}/value"])
    assert total == 27787 and len(L["rand128/value"]) == 4667


# ---- 1. libm: the reference's log ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_libm_log_is_the_recording(runs, name, shuffled):
    rec, reason, state = runs[0, shuffled][name]
    assert reason == 1 and len(rec) == len(L[f"{name}/value"]), name
    for f in FIELDS:
        assert rec[f].dtype == L[f"{name}/{f}"].dtype and bits(rec[f]) == bits(L[f"{name}/{f}"]), (name, f)
    assert state[2] == int(L[f"{name}/final_pos"]), name
    digest = hashlib.sha256(np.ascontiguousarray(state[1], dtype="<u4").tobytes()).digest()
    assert digest == L[f"{name}/final_key_sha256"].tobytes(), name


# ---- 2. portable math against libm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_portable_math_has_the_same_structure(runs, name):
    got, want = runs[1, False][name], runs[0, False][name]
    assert got[1] == want[1] and len(got[0]) == len(want[0]), name
    for f in ("event_id", "node", "kind"):
        assert np.array_equal(got[0][f], want[0][f]), (name, f)
    assert same_state(got[2], want[2]), name
    r = ratio(got[0]["value"], want[0]["value"])
    print(name, "max |portable - libm| / max(1, |x|):", r)
    assert r <= PORTABLE_BOUND, name
    shuffled = runs[1, True][name]
    assert bits(shuffled[0]) == bits(got[0]) and same_state(shuffled[2], got[2]), name


# ---- 3. kind 0 is the existing entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("dim", [2, 15, 16, 64, 128])
def test_all_normal_kinds_are_the_existing_entry(dim, math):
    a = case_arrays(names_of_dim(dim))
    old = sv.run_batch_host(*a, math=math)
    new = sv.run_batch_host(*a, math=math, kind=np.zeros(a[1].shape, dtype=np.int32))
    assert len(old.value) > 0
    for f in old._fields:
        assert bits(getattr(new, f)) == bits(getattr(old, f)), f


def test_kind_none_calls_the_old_symbol(monkeypatch):
    lib = _lib.load()
    called = []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("gdm_des_run_batch"):
                called.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    a, kind = dist_case_arrays(["mix5"])
    sv.run_batch_host(*a, math=1)
    sv.run_batch_host(*a, math=1, kind=kind)
    assert called == ["gdm_des_run_batch_host", "gdm_des_run_batch_dist_host"]


def test_run_batch_dist_routes_like_run_stats(monkeypatch):
    called = []
    real = sv.run_batch_host
    monkeypatch.setattr(sv, "run_batch_host", lambda *a, **k: (called.append(k.get("kind")), real(*a, **k))[1])
    state = np.random.RandomState(5).get_state()
    normal = sv.run_batch_dist([corpus_spec("q_wrap3")], states=[state])
    want = sv.run_batch([corpus_spec("q_wrap3")], states=[state])
    for f in want._fields:
        assert bits(getattr(normal, f)) == bits(getattr(want, f)), f
    spec = sv.mm1k_spec(0.8, 1.0, 3, 80, seed=7)
    log = sv.run_batch_dist([spec], states=[state], math=0)
    assert called[0] is None and called[1] is None and called[2].tolist() == [[1, 1]]
    assert log.stop_reason.tolist() == [1] and log.n_records[0] > 100 and set(log.kind.tolist()) == {0, 1, 2}
    st = sv.run_stats([spec], states=[state])
    assert int(st.n_records[0]) == int(sv.run_batch_dist([spec], states=[state], max_records=0).n_records[0])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_kind_out_of_range_refuses_the_host_call():
    a, kind = dist_case_arrays(["mix5"])
    for bad in (3, -1):
        k = kind.copy()
        k[0, 4] = bad
        with pytest.raises(_lib.GdmError, match="kind"):
            sv.run_batch_host(*a, math=1, kind=k)


@pytest.mark.parametrize("math", [0, 1])
def test_refused_samples_inside_a_batch(runs, math):
    names = ["uni_neg", "uni_neg", "uni_neg", "scale0_srv", "uni_neg", "scale0_src"]      # uni_neg: 0 -> 1 -> 2
    a, kind = dist_case_arrays(names)
    loc, scale = a[1].copy(), a[2].copy()
    scale[1, 2] = -0.5                                    # sample 1: scipy's "Domain error"
    kind[2, 1], scale[2, 1] = 1, 0.0                      # sample 2: an exponential server that only ever gives 0.0
    kind[4, 2], scale[4, 2], loc[4, 2] = 2, 0.0, 0.0      # sample 4: a uniform server that only ever gives loc = 0
    log = sv.run_batch_host(a[0], loc, scale, *a[3:], math=math, max_records=0, kind=kind)
    assert log.stop_reason.tolist() == [1, ERROR, ERROR, 1, ERROR, 1]
    for b in (1, 2, 4):
        assert log.n_records[b] == 0 and log.rec_ptr[b] == log.rec_ptr[b + 1], b
        assert same_state(sv.state_of(log, b), dist_state0(names[b])), b
    for b in (0, 3, 5):
        rec, reason, state = runs[math, False][names[b]]
        assert bits(sv.sample_log(log, b)) == bits(rec) and same_state(sv.state_of(log, b), state), b


def test_the_logging_surface_without_kinds_keeps_refusing():
    spec = sv.mm1k_spec(0.8, 1.0, 3, 50)
    with pytest.raises(NotImplementedError):
        sv.spec_arrays([spec])
    with pytest.raises(NotImplementedError):
        sv.run_batch([spec])
    with pytest.raises(NotImplementedError):
        sv.Sim(spec.sim_matrix, spec.distributions, spec.queue_list, seeds=[1], logging_mode='Music')
    spec.distributions = [["gamma", 2.0, 0.0, 1.0], ["normal", 0.5, 0.1]]
    with pytest.raises(NotImplementedError, match="gamma"):
        sv.run_batch_dist([spec])


# ---- 5. the record cap -----------------------------------------------------------------------------------------------
def test_max_records_cuts_the_log(runs):
    a, kind = dist_case_arrays(["mix5", "mix5"])
    log = sv.run_batch_host(*a, math=0, max_records=100, kind=kind)
    assert log.stop_reason.tolist() == [RECORDS, RECORDS] and log.rec_ptr.tolist() == [0, 100, 200]
    assert bits(sv.sample_log(log, 1)) == bits(runs[0, False]["mix5"][0][:100])


def test_workspace_error_reports_the_count_and_leaves_a_retry_possible(runs):
    lib = _lib.load()
    (adj, loc, scale, qcap, seed, cust, states), kind = dist_case_arrays(["uni2", "mix5"][1:] + ["mix5"])
    b, dim = adj.shape[0], adj.shape[1]
    seed, cust, qcap = seed.astype(np.int64), cust.astype(np.int64), qcap.astype(np.int32)
    want = runs[0, False]["mix5"][0]

    def call(cap):
        key, pos, has, gauss = (np.array(x) for x in sv.pack_states(states, b))      # the ORIGINAL states, every time
        value, eid = np.zeros(cap, dtype=np.float64), np.zeros(cap, dtype=np.int64)
        node, rkind = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        ptr, n_rec, stop = np.zeros(b + 1, dtype=np.int64), np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int32)
        rc = lib.gdm_des_run_batch_dist_host(adj.ctypes.data, b, dim, loc.ctypes.data, scale.ctypes.data,
                                             kind.ctypes.data, qcap.ctypes.data, seed.ctypes.data, cust.ctypes.data,
                                             int(qcap.max()), 0, 200000, 0, key.ctypes.data, pos.ctypes.data,
                                             has.ctypes.data, gauss.ctypes.data, value.ctypes.data, eid.ctypes.data,
                                             node.ctypes.data, rkind.ctypes.data, cap, ptr.ctypes.data,
                                             n_rec.ctypes.data, stop.ctypes.data)
        return rc, ptr, value, n_rec

    rc, ptr, _value, n_rec = call(len(want) + 10)          # room for one sample and ten records
    assert rc == -3 and b"gdm_des_run_batch_dist_host: record arrays too small" in lib.gdm_last_error()
    assert ptr[-1] == 2 * len(want) and n_rec.tolist() == [len(want)] * 2
    rc, ptr, value, _n = call(int(ptr[-1]))
    assert rc == 0 and bits(value[:len(want)]) == bits(want["value"]) == bits(value[len(want):])


# ---- 6. the log file -------------------------------------------------------------------------------------------------
def test_write_music_log_is_the_references_text(tmp_path, runs):
    rec = runs[0, False]["mix5"][0]
    path = str(tmp_path / "logs" / "simulation.log")
    os.makedirs(os.path.dirname(path))
    sv.write_music_log(rec, path)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == len(rec) + 1
    names = ("arrival", "departure", "processing")
    for i, line in enumerate(lines[:-1]):                 # logging.info's "%s" of a float is its repr
        want = "INFO:root:%s - %s - %s - %s" % (float(L["mix5/value"][i]), int(L["mix5/event_id"][i]),
                                                int(L["mix5/node"][i]), names[int(L["mix5/kind"][i])])
        assert line == want, i
    back = sl.process_adjsim_log(L["mix5/servers"].tolist(), log_path=path)
    assert np.array_equal(back, L["mix5/tracks"])


def test_sim_run_writes_the_file_it_wrote(tmp_path):
    spec = corpus_spec("q_wrap3")
    state = np.random.get_state()
    try:
        np.random.seed(11)
        sim = sv.Sim(spec.sim_matrix, spec.distributions, spec.queue_list, seeds=spec.seeds,
                     log_path=str(tmp_path) + "/", generate_log=True, logging_mode='Music')
        log = sim.run(number_of_customers=int(spec.num_customers))
    finally:
        np.random.set_state(state)
    want = "".join(f"INFO:root:{float(v)!r} - {int(e)} - {int(n)} - {sv.KIND_NAMES[k]}\n" for v, e, n, k in log)
    assert len(log) > 20 and open(str(tmp_path / "simulation.log")).read() == want


# ---- 7. the stand-alone program under the host sanitizers ------------------------------------------------------------
def stand_alone_cases():
    """(label, arrays of one case, kind, servers, max_records, max_lines)."""
    out = []
    for n, max_records, max_lines in (("mix5", 0, 5000), ("uni_neg", 0, 300), ("scale0_srv", 150, 5000),
                                      ("rand17", 0, 5000), ("mix6", 0, 5000), ("renege", 0, 5000)):
        a, kind = dist_case_arrays([n])
        servers = L[f"{n}/servers_perm"].tolist()
        if n == "mix6":
            kind = kind.copy()
            kind[0, 5] = 3
            n = "refused"
        if n == "renege":
            a = a[:2] + (np.array([[0.25, 0.0]]),) + a[3:]          # the exponential server's scale 0: stops inside the chain
            n = "scale0"
        out.append((n, a, kind, servers, max_records, max_lines))
    return out


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH: the sanitizer build of "
                    "tools/des_log_dist_host.cpp did not run")
    cases = stand_alone_cases()
    exe, cases_bin, logs_bin = str(tmp_path / "des_log_dist_host"), str(tmp_path / "cases.bin"), str(tmp_path / "logs.bin")
    with open(cases_bin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _n, (adj, loc, scale, qcap, seed, cust, states), kind, servers, max_records, max_lines in cases:
            st = states[0]
            f.write(struct.pack("<iiiiqqqdqq", adj.shape[1], int(st[3]), int(st[2]), len(servers), int(seed[0]),
                                int(cust[0]), 200000, float(st[4]), max_records, max_lines))
            for a, dt in ((adj[0], "<f8"), (loc[0], "<f8"), (scale[0], "<f8"), (kind[0], "<i4"), (qcap[0], "<i4"),
                          (st[1], "<u4"), (servers, "<i4")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            *static, "-I", os.path.join(ROOT, "gan_des_midi_music_gen_amd", "csrc"),
                            os.path.join(ROOT, "tools", "des_log_dist_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, cases_bin, logs_bin], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    with open(logs_bin, "rb") as f:
        for n, a, kind, servers, max_records, max_lines in cases:
            dim, s = a[0].shape[1], len(servers)
            reason, has, pos, track_status, n_rec, n_rows, gauss = struct.unpack("<iiiiqqd", f.read(40))
            rec = {name: np.frombuffer(f.read(np.dtype(dt).itemsize * n_rec), dtype=dt)
                   for name, dt in (("value", "<f8"), ("event_id", "<i8"), ("node", "<i4"), ("kind", "<i4"))}
            key = np.frombuffer(f.read(4 * 624), dtype="<u4")
            tracks = np.frombuffer(f.read(4 * n_rows * s), dtype="<i4").reshape(n_rows, s)
            state = ("MT19937", key, pos, has, gauss)
            if n == "refused":                            # the host ENTRY refuses the call: the device's rule is the header's
                assert reason == ERROR and n_rec == 0 and same_state(state, a[6][0])
                assert track_status == 0 and n_rows == 1 and not tracks.any()
                continue
            want = sv.run_batch_host(*a, math=1, max_records=max_records, kind=kind)
            assert reason == want.stop_reason[0] and n_rec == want.n_records[0], n
            assert {"scale0": ERROR, "scale0_srv": RECORDS}.get(n, 1) == reason, n
            for name in FIELDS:
                assert bits(rec[name]) == bits(getattr(want, name)), (n, name)
            assert same_state(state, sv.state_of(want, 0)), n
            if n == "scale0":
                assert same_state(state, a[6][0]) and n_rec == 0
            want_tracks, want_ptr = sl.log_tracks(want, servers, max_lines=max_lines, dim=dim)
            assert track_status == 0 and n_rows == want_ptr[1] and np.array_equal(tracks, want_tracks), n
        assert f.read() == b""
