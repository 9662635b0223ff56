"""GPU: the batched discrete-event simulator (gdm_des_run_batch, csrc/des_batch.hip) against its host mirror
(gdm_des_run_batch_host with portable math: the same csrc/des_sim.h compiled for the host, which tests/test_des_batch.py
pins to the reference's recording), and the "des_batch" bridges / trainers against the composition of their parts.

Bar: equal bits everywhere -- values, ids, nodes, kinds, rec_ptr, counts, stop reasons, final generator states.  Every
device run here writes into guarded buffers: the words behind every output and behind the workspace must be intact."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import _lib, matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402
from helpers import load_golden  # noqa: E402
from test_des_batch import ERROR, BUDGET, RECORDS, bound_cases, golden_arrays  # noqa: E402

DEV = torch.device("cuda")
HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 0x5A


def edge_inputs(n):
    rs = np.random.RandomState(8)
    r = np.sqrt(0.5)
    edge = [2.0 ** -106, np.nextafter(1.0, 0.0), np.nextafter(np.nextafter(1.0, 0.0), 0.0), 1.0 - 2.0 ** -21,
            1.0 - 2.0 ** -19, r, np.nextafter(r, 0.0), np.nextafter(r, 1.0), 0.5, np.nextafter(0.5, 0.0), 2.0 ** -1022]
    x = np.concatenate([edge, rs.random_sample(n - len(edge) - 8192), rs.random_sample(4096) * 2.0 ** -rs.randint(1, 300, 4096),
                        1.0 - rs.random_sample(4096) * 2.0 ** -rs.randint(1, 52, 4096)])
    return x[(x > 0) & (x < 1)]


def test_math_probe_device_equals_host_bit_for_bit():
    x = edge_inputs(65536 + 64)
    assert len(x) >= 65536
    want_log, want_fac = sv.math_probe_host(x)
    got_log, got_fac = ops.des_math_probe(torch.from_numpy(x).to(DEV))
    assert np.array_equal(got_log.cpu().numpy().view(np.int64), want_log.view(np.int64))
    assert np.array_equal(got_fac.cpu().numpy().view(np.int64), want_fac.view(np.int64))


def guarded(nbytes):
    """(whole buffer, inner view of nbytes, 256-aligned): 256 canary bytes on both sides."""
    pad = (-nbytes) % 256
    buf = torch.full((256 + nbytes + pad + 256,), CANARY, dtype=torch.uint8, device=DEV)
    return buf, buf[256:256 + nbytes]


def device_run(arrays, max_records, max_events=200000, max_queue_cap=254):
    """gdm_des_run_batch through the C ABI with every output and the workspace in guarded buffers -> BatchLog of numpy
    arrays (records cut to rec_ptr[B]); asserts the guards."""
    adj, loc, scale, qcap, seed, cust, states = arrays
    adj = np.ascontiguousarray(adj, dtype=np.float64)
    b, dim = adj.shape[0], adj.shape[1]
    key, pos, has, gauss = sv.pack_states(states, b)
    n = b * max_records

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)

    ins = [up(adj, np.float64), up(np.reshape(loc, (b, dim)), np.float64), up(np.reshape(scale, (b, dim)), np.float64),
           up(np.reshape(qcap, (b, dim)), np.int32), up(seed, np.int64), up(cust, np.int64)]
    sizes = {"key": b * 624 * 4, "pos": b * 4, "has": b * 4, "gauss": b * 8, "value": n * 8, "event_id": n * 8,
             "node": n * 4, "kind": n * 4, "rec_ptr": (b + 1) * 8, "n_records": b * 8, "stop": b * 4,
             "ws": ops.des_batch_workspace_bytes(b, dim, max_queue_cap)}
    bufs = {k: guarded(v) for k, v in sizes.items()}
    for name, src in (("key", key.view(np.uint8)), ("pos", pos.view(np.uint8)), ("has", has.view(np.uint8)),
                      ("gauss", gauss.view(np.uint8))):
        bufs[name][1].copy_(torch.from_numpy(src.reshape(-1)).to(DEV))
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}
    rc = _lib.load().gdm_des_run_batch(
        *(ctypes.c_void_p(t.data_ptr()) for t in ins[:1]), b, dim, *(ctypes.c_void_p(t.data_ptr()) for t in ins[1:]),
        max_queue_cap, max_events, max_records, p["key"], p["pos"], p["has"], p["gauss"], p["value"], p["event_id"],
        p["node"], p["kind"], n, p["rec_ptr"], p["n_records"], p["stop"], p["ws"], sizes["ws"],
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gdm_des_run_batch")
    torch.cuda.synchronize()
    for name, (buf, inner) in bufs.items():
        tail = buf[256 + inner.numel():]
        assert bool((buf[:256] == CANARY).all()) and bool((tail == CANARY).all()), f"guard of {name} overwritten"

    def down(name, dt):
        return bufs[name][1].cpu().numpy().view(dt).copy()

    rec_ptr = down("rec_ptr", np.int64)
    m = int(rec_ptr[-1])
    assert 0 <= m <= n
    return sv.BatchLog(down("value", np.float64)[:m], down("event_id", np.int64)[:m], down("node", np.int32)[:m],
                       down("kind", np.int32)[:m], rec_ptr, down("n_records", np.int64), down("stop", np.int32),
                       down("key", np.uint32).reshape(b, 624), down("pos", np.int32), down("has", np.int32),
                       down("gauss", np.float64))


def assert_same(dev, host):
    assert np.array_equal(dev.rec_ptr, host.rec_ptr), (dev.rec_ptr, host.rec_ptr)
    assert np.array_equal(dev.n_records, host.n_records) and np.array_equal(dev.stop_reason, host.stop_reason)
    assert np.array_equal(dev.value.view(np.int64), host.value.view(np.int64))
    for name in ("event_id", "node", "kind", "mt_key", "mt_pos", "has_gauss"):
        assert np.array_equal(getattr(dev, name), getattr(host, name)), name
    assert np.array_equal(dev.gauss.view(np.int64), host.gauss.view(np.int64))


def both(arrays, max_records, max_events=200000, max_queue_cap=254):
    host = sv.run_batch_host(*arrays, math=1, max_records=max_records, max_events=max_events, max_queue_cap=max_queue_cap)
    dev = device_run(arrays, max_records, max_events=max_events, max_queue_cap=max_queue_cap)
    assert_same(dev, host)
    return host


@pytest.fixture(scope="module")
def golden():
    return load_golden("des_core.npz")


def hand_variants(g, n):
    """n samples of the `hand` net (dim 5; node 2 has scale 0, node 2's only child is node 0: sink-like) with different
    Sim seeds and generator states."""
    adj, loc, scale, qcap, seed, cust, _ = golden_arrays(g, ("hand",) * n)
    seed = [4242 + 17 * i for i in range(n)]
    states = [np.random.RandomState(100 + i).get_state() for i in range(n)]
    if n > 1:                                                     # one state mid-stream, with a cached gauss
        rs = np.random.RandomState(7)
        rs.standard_normal(3)
        rs.random_sample(611)
        states[1] = rs.get_state()
    return adj, loc, scale, qcap, seed, cust, states


@pytest.mark.parametrize("n", [1, 3])
def test_hand_net(golden, n):
    host = both(hand_variants(golden, n), 1024)                   # above the run's 700-odd records: uncapped in effect
    assert (host.stop_reason == 1).all() and (host.n_records > 500).all() and (host.n_records < 1024).all()
    if n == 3:
        assert len({int(x) for x in host.n_records}) > 1          # ragged: the pack step moves records


@pytest.mark.parametrize("cases", [("wav0", "wav1"), ("midi0", "midi1")])
def test_bridge_sized_nets_at_the_record_cap(golden, cases):
    """dim 15: node generators in LDS; dim 61: in the workspace."""
    host = both(golden_arrays(golden, cases), 5001)
    assert host.stop_reason.tolist() == [RECORDS, RECORDS] and host.rec_ptr.tolist() == [0, 5001, 10002]


def test_more_samples_than_lanes(golden):
    a = hand_variants(golden, 65)
    host = both(a, 1024)
    for b in range(65):                                           # each row against its own single-sample run
        one = sv.run_batch_host(*(x[b:b + 1] for x in a), math=1, max_records=1024, max_queue_cap=254)
        assert np.array_equal(sv.sample_log(host, b), sv.sample_log(one, 0))
        assert np.array_equal(host.mt_key[b], one.mt_key[0])


def test_small_nets_regenerate_every_generator():
    """Sample 0, one source and one server (padded with an idle third node): every normal comes from the same two
    generators; the server is a sink, so the global stream is drawn from once.  Sample 1, source -> server -> server:
    every departure of the middle server draws its destination from the global stream.  1000 customers make each
    generator twist its 624 words several times."""
    adj = np.array([[[1.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]],
                    [[1.0, 1.0, 0.0], [0.0, -1.0, 1.0], [0.0, 0.0, -1.0]]])
    rs = np.random.RandomState(3)
    rs.random_sample(150)
    state = rs.get_state()
    a = (adj, [[2.0, 1.5, 1.0]] * 2, [[0.5, 0.4, 0.3]] * 2, [[254] * 3] * 2, [99, 99], [1000, 1000], [state, state])
    host = both(a, 8192)
    assert host.stop_reason.tolist() == [1, 1] and (host.n_records < 8192).all()
    logs = [sv.sample_log(host, b) for b in (0, 1)]
    # a polar pair costs at least 4 words and yields 2 normals: n service records -> at least 2 n words of one generator
    assert int(((logs[0]["kind"] == 2) & (logs[0]["node"] == 1)).sum()) >= 900 and not (logs[0]["node"] == 2).any()
    for b, routing_draws in ((0, 1), (1, 1 + int(((logs[1]["kind"] == 1) & (logs[1]["node"] == 1)).sum()))):
        total = int(state[2]) + 2 * routing_draws                 # one double = two words per routing draw
        regenerations = (total - 1) // 624
        assert int(host.mt_pos[b]) == total - 624 * regenerations
        assert regenerations >= (2 if b else 0)


def _uniform_row():
    """Two probabilities whose normalised values do not sum to exactly 1: FlowBranchOperator then draws uniformly."""
    rs = np.random.RandomState(1)
    for _ in range(10000):
        p = rs.random_sample(2)
        s = 0.0 + p[0] + p[1]
        if 0.0 + p[0] / s + p[1] / s != 1.0:
            return p
    raise AssertionError("no such row found")


def test_zero_scale_uniform_branch_and_sink_row(golden):
    adj, loc, scale, qcap, seed, cust, states = hand_variants(golden, 3)
    loc, scale = np.array(loc), np.array(scale)
    # 0: every server deterministic (scale 0, loc > 0): only the sources draw normals
    scale[0, :3] = 0.0
    assert (loc[0, :3] > 0).all()
    # 1: node 1's row (children 0 and 2) does not sum to 1 after normalisation: the uniform randint branch
    adj[1, 1, 0], adj[1, 1, 2] = _uniform_row()
    # 2: node 1 is a sink row: customers leave the net there
    adj[2, 1, :] = [0.0, -1.0, 0.0, 0.0, 0.0]
    host = both((adj, loc, scale, qcap, seed, cust, states), 2048)
    assert (host.stop_reason == 1).all() and (host.n_records > 100).all()
    l2 = sv.sample_log(host, 2)
    assert not ((l2["node"] == 0) | (l2["node"] == 2)).any()      # nothing ever leaves node 1 for another node
    assert (sv.sample_log(host, 0)["node"] == 2).any() and (sv.sample_log(host, 1)["node"] == 2).any()


def test_bounds_in_one_batch_with_healthy_neighbours(golden):
    adj, loc, scale, qcap, seed, cust, states = bound_cases(golden)      # [budget, healthy, queue_cap 2, bad]
    order = [0, 1, 2, 1, 3]
    a = (adj[order], loc[order], scale[order], qcap[order], np.asarray(seed)[order], np.asarray(cust)[order],
         [states[i] for i in order])
    host = both(a, 2048, max_events=2000)
    assert host.stop_reason.tolist() == [BUDGET, 1, int(host.stop_reason[2]), 1, ERROR]
    assert host.n_records[0] == 1 and host.n_records[4] == 0 and host.n_records[2] > 0
    assert np.array_equal(sv.sample_log(host, 1), sv.sample_log(host, 3))


def test_argument_checks():
    with pytest.raises(ops.GdmError):
        ops.des_batch_workspace_bytes(1, 129, 254)
    z = torch.zeros
    args = dict(max_queue_cap=4, max_events=10)
    ten = (z((1, 2, 2), dtype=torch.float64, device=DEV), z((1, 2), dtype=torch.float64, device=DEV),
           z((1, 2), dtype=torch.float64, device=DEV), z((1, 2), dtype=torch.int32, device=DEV),
           z(1, dtype=torch.int64, device=DEV), z(1, dtype=torch.int64, device=DEV),
           z((1, 624), dtype=torch.int32, device=DEV), z(1, dtype=torch.int32, device=DEV),
           z(1, dtype=torch.int32, device=DEV), z(1, dtype=torch.float64, device=DEV))
    with pytest.raises(ops.GdmError):
        ops.des_run_batch(*ten, max_records=0, **args)            # a record cap is required on the device
    with pytest.raises(ops.GdmError):
        ops.des_run_batch(*(t.cpu() for t in ten), max_records=8, **args)
    with pytest.raises(ops.GdmError):
        ops.des_run_batch(*ten, max_records=8, max_queue_cap=4, max_events=0)


# ---- bridges ------------------------------------------------------------------------------------------------------------
def _rng_fixture():
    return np.load(os.path.join(HERE, "golden", "des_prologue_rng.npz"))


@pytest.fixture(params=["device", "host"])
def route(request, monkeypatch):
    """"des_batch" picks the kernel or the host mirror by batch size (same bits): run these small batches through both."""
    monkeypatch.setattr(msp, "DES_BATCH_DEVICE_MIN_B", 1 if request.param == "device" else 1 << 30)
    return request.param


def test_route_by_batch_size(monkeypatch):
    seen = []
    log = sv.BatchLog(*[np.zeros(1, np.int32)] * 11)
    monkeypatch.setattr(sv, "run_batch_device", lambda *a, device, **kw: seen.append(device) or log)
    monkeypatch.setattr(sv, "run_batch_host", lambda *a, **kw: seen.append(None) or log)
    for b in (1, msp.DES_BATCH_DEVICE_MIN_B - 1, msp.DES_BATCH_DEVICE_MIN_B, 256):
        pro = msp.BatchedPrologue(msp.WAV, {"b": b}, np.zeros((b, 15, 15)), None, None, None)
        pro.loc = pro.scale = pro.queue_cap = np.ones((b, 15))      # the per-node arrays, which the stand-ins ignore
        pro.seed = pro.customers = np.ones(b)
        pro.simulate_on(DEV)
    assert seen == [None, None, DEV, DEV] and 30 < msp.DES_BATCH_DEVICE_MIN_B <= 64


def test_matrix_to_wav_des_batch_equals_its_parts(route):
    from gan_des_midi_music_gen_amd import sim_log_process_music as slpm, util
    d = _rng_fixture()
    m, seed = torch.from_numpy(d["wav/matrices"]).to(DEV), int(d["wav/np_seed"])
    np.random.seed(seed)
    pro = msp.batched_prologue_wav(m, 20)
    state_want = np.random.get_state()
    host = pro.simulate(None)
    logs = [sv.sample_log(host, b) for b in range(5)]
    assert all(len(lg) > 100 for lg in logs)
    *staged, status = slpm.stage_notes(logs, pro.instruments, pro.note_levels, device=DEV)
    want = util._db_from_frames(ops.synth_frames(*staged), 5, ops.SYNTH_FRAMES, ops.SYNTH_RATE, ops.SYNTH_NFFT, 128, 20,
                                8300, 80)
    slpm.raise_for_status(status)
    np.random.seed(seed)
    got = msp.matrix_to_wav(m, size=20, start=0, end=216, device=DEV, simulate="des_batch")
    state_got = np.random.get_state()
    assert state_got[2:] == state_want[2:] and np.array_equal(state_got[1], state_want[1])
    assert got.is_cuda and got.shape == (5, 128, 216) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got.max()) > -60.0                               # audible clips, not blanks
    np.random.seed(seed)
    specs = msp.wav_prologue(m, size=20)                          # ... which is where wav_prologue leaves the stream
    assert np.array_equal(np.random.get_state()[1], state_want[1]) and len(specs) == 5
    np.random.seed(seed)
    cut = msp.matrix_to_wav(m, size=20, start=20, end=194, device="cpu", simulate="des_batch")
    assert not cut.is_cuda and torch.equal(cut, got[:, :, 20:194].cpu())


def test_matrix_to_midi_des_batch_equals_its_parts(tmp_path, route):
    from gan_des_midi_music_gen_amd import sim_log_to_midi as s2m
    d = _rng_fixture()
    g1 = torch.from_numpy(d["midi/g1"]).unsqueeze(1).clone()
    g2 = torch.from_numpy(d["midi/g2"]).clone()
    g2[2, 3], g2[2, 4] = 0.0, 0.0                                 # sample 2: servers with loc = scale = 0 -> its run errors
    g1, g2, seed = g1.to(DEV), g2.to(DEV), int(d["midi/np_seed"])
    for generate in (False, True):
        np.random.seed(seed)
        pro = msp.batched_prologue_midi(g1, g2, (64, 64), None)
        state_want = np.random.get_state()
        host = pro.simulate(None)
        assert host.stop_reason.tolist()[2] == ERROR and host.n_records[2] == 0 and (host.n_records[[0, 1, 3]] > 0).all()
        logs = [sv.sample_log(host, b) for b in range(4)]
        save = [int(host.stop_reason[b]) not in (ERROR, BUDGET) and (generate or s2m.lines_read(len(logs[b])) % 100 == 0)
                for b in range(4)]
        want, _tracks = s2m.log_to_rolls(logs, pro.h["g2"][:, 10:], pro.instruments, pro.note_levels, start=100, end=150,
                                         save=save, device=DEV)
        np.random.seed(seed)
        path = str(tmp_path / "generation.mid")
        got, failed = msp.matrix_to_midi(g1, g2, adj_size=(64, 64), instrument=None, start=100, end=150, count=1,
                                         generate=generate, simulate="des_batch", return_tensor=True, midi_path=path)
        state_got = np.random.get_state()
        assert state_got[2:] == state_want[2:] and np.array_equal(state_got[1], state_want[1])
        assert failed == 1 and got.shape == (4, 2, 128, 50) and torch.equal(got, want) and not got[2].any()
        assert [bool(got[b].any()) for b in range(4)] == [bool(want[b].any()) for b in range(4)]
        if generate:
            assert save == [True, True, False, True] and bool(got[3].any()) and os.path.getsize(path) > 30
        else:
            assert not os.path.exists(path)
    np.random.seed(seed)
    msp.midi_prologue(g1, g2, adj_size=(64, 64))
    assert np.array_equal(np.random.get_state()[1], state_want[1])
    np.random.seed(seed)
    rolls, failed = msp.matrix_to_midi(g1, g2, adj_size=(64, 64), start=100, end=150, generate=True, simulate="des_batch",
                                       midi_path=str(tmp_path / "g.mid"))
    assert failed == 1 and len(rolls) == 4 and rolls[0].dtype == np.float64
    assert np.array_equal(np.stack(rolls), got.double().cpu().numpy())
    with pytest.raises(ops.GdmError):
        msp.matrix_to_midi(g1, g2, adj_size=(64, 64), simulate="des_batched")


def test_matrix_to_wav_des_batch_raises_for_an_errored_sample(route):
    d = _rng_fixture()
    m = torch.from_numpy(d["wav/matrices"][:2]).clone()
    m[1, 18, :], m[1, 19, :] = 0.0, 0.0                            # rows dim+3, dim+4 carry all their weight in a column
    m[1, 18, 19], m[1, 19, 19] = 1.0, 1.0                          # beyond the nodes: every loc and scale is 0
    with pytest.raises(ValueError):
        np.random.seed(1)
        msp.matrix_to_wav(m.to(DEV), size=20, start=0, end=216, device=DEV, simulate="des_batch")


# ---- trainers ---------------------------------------------------------------------------------------------------------
def test_simnn_train_with_des_batch_equals_the_host_mirror_route(route):
    from gan_des_midi_music_gen_amd import SIMNN, sim_log_process_music as slpm, util

    def mirror_provider(generated):
        pro = msp.batched_prologue_wav(generated, 20, None)
        host = pro.simulate(None)
        logs = [sv.sample_log(host, b) for b in range(generated.shape[0])]
        *staged, status = slpm.stage_notes(logs, pro.instruments, pro.note_levels, device=generated.device)
        mel = util._db_from_frames(ops.synth_frames(*staged), len(logs), ops.SYNTH_FRAMES, ops.SYNTH_RATE, ops.SYNTH_NFFT,
                                   128, 20, 8300, 80)
        return mel[:, :, 0:216]

    kw = dict(batch_size=2, max_steps=2, seed=11, save=False, log=lambda *_a: None, device=DEV)
    np.random.seed(4)
    _g, _d, g_want, d_want = SIMNN.train(fake_provider=mirror_provider, **kw)
    np.random.seed(4)
    _g, _d, g_got, d_got = SIMNN.train(fake_provider="des_batch", **kw)
    assert len(g_got) == 2 and g_got == g_want and d_got == d_want and np.isfinite(g_got).all()
    with pytest.raises(ValueError):
        SIMNN.train(fake_provider="des_batched", max_steps=1, save=False, device=DEV)


def test_training_loop_with_des_batch_equals_the_host_mirror_route(route):
    from gan_des_midi_music_gen_amd import network_tests as NT, sim_log_to_midi as s2m

    def mirror_provider(g1, g2, count):
        pro = msp.batched_prologue_midi(g1, g2, (64, 64), 0)
        host = pro.simulate(None)
        logs = [sv.sample_log(host, b) for b in range(g1.shape[0])]
        good = [int(r) not in (ERROR, BUDGET) for r in host.stop_reason]
        save = [ok and s2m.lines_read(len(lg)) % 100 == 0 for ok, lg in zip(good, logs)]
        rolls, _ = s2m.log_to_rolls(logs, pro.h["g2"][:, 10:], pro.instruments, pro.note_levels, start=100, end=150,
                                    save=save, device=g1.device)
        return rolls, len(good) - sum(good)

    kw = dict(num_epochs=1, steps_per_epoch=2, seed=1, log=lambda *_a: None)
    np.random.seed(9)
    d_want, g_want = NT.training_loop(2, fake_provider=mirror_provider, **kw)
    np.random.seed(9)
    d_got, g_got = NT.training_loop(2, fake_provider="des_batch", **kw)
    assert len(d_got) == 2 and list(d_got) == list(d_want) and list(g_got) == list(g_want) and np.isfinite(d_got).all()
    with pytest.raises(ValueError):
        NT.training_loop(2, fake_provider="des_batched", **kw)


def test_command_lines_accept_des_batch(monkeypatch):
    """The parsers and what they hand on: nothing is trained here."""
    from gan_des_midi_music_gen_amd import SIMNN, network_tests as NT
    seen = []
    monkeypatch.setattr(SIMNN, "train", lambda **kw: seen.append(kw))
    monkeypatch.setattr(NT, "training_loop", lambda *a, **kw: seen.append(kw))
    SIMNN.main(["--fake-provider", "des_batch", "--max-steps", "1", "--no-save"])
    NT.main(["--pickle", "none.pkl", "--fake-provider", "des_batch", "--max-steps", "1"])
    assert [kw["fake_provider"] for kw in seen] == ["des_batch", "des_batch"]
    with pytest.raises(SystemExit):
        SIMNN.main(["--fake-provider", "des_batched"])
