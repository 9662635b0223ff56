"""The batch form of the discrete-event simulator on the HOST (simulation_v3.run_batch_host -> gdm_des_run_batch_host,
csrc/des_core.hip on the shared event logic of csrc/des_sim.h).  Runs without a GPU, except the batched prologue.

  * libm math, no record cap: the five runs of tests/golden/des_core.npz (recorded from the reference's own Sim), batched
    by size, must come out bit for bit, whatever the batch and the position in it;
  * portable math (what the device runs): same events, ids, nodes, kinds, floor(value) and final generator state; values
    within 10x the relative difference measured on the five runs (7.7e-14, DESIGN.md section 7: later draws accumulate);
    des_log within 2 ulp of math.log (both are below 1 ulp from the true value);
  * the record cap gives a prefix; the bounds (draw budget, ring, routing to a source) end a sample and only that one;
  * the batched prologue makes midi_prologue's / wav_prologue's specs and snapshots the stream after every reseed."""
import math

import numpy as np
import pytest

from gan_des_midi_music_gen_amd import simulation_v3 as sv
from helpers import load_golden

CASES = ("midi0", "midi1", "wav0", "wav1", "hand")
GROUPS = (("midi0", "midi1"), ("wav0", "wav1"), ("hand",))
SEEDS = {"midi0": 1000, "midi1": 1001, "wav0": 2000, "wav1": 2001, "hand": 77}
REL_MEASURED = 7.7e-14          # max |portable - golden| / |golden| over the five runs
ERROR, RECORDS, BUDGET = 3, 4, 5


def golden_arrays(g, cases):
    """(adj, loc, scale, queue_cap, seed, customers, states) of golden runs of one size."""
    dist = [g[f"{c}/dist"] for c in cases]
    states = []
    for c in cases:
        np.random.seed(SEEDS[c])
        states.append(np.random.get_state())
    return (np.stack([g[f"{c}/sim_matrix"] for c in cases]),
            [[float(np.float32(a)) for a, _ in d] for d in dist], [[float(np.float32(b)) for _, b in d] for d in dist],
            [list(g[f"{c}/queue_list"]) for c in cases], [int(g[f"{c}/seeds"].reshape(-1)[0]) for c in cases],
            [int(g[f"{c}/customers"]) for c in cases], states)


def _rng_after(log, b):
    keep = np.random.get_state()
    np.random.set_state(sv.state_of(log, b))
    after = np.random.randint(0, 2 ** 31 - 1)
    np.random.set_state(keep)
    return after


@pytest.fixture(scope="module")
def golden():
    return load_golden("des_core.npz")


@pytest.fixture(scope="module")
def uncapped(golden):
    """math -> case -> (records, stop reason, rng_after) of the uncapped batched runs (computed once)."""
    out = {0: {}, 1: {}}
    for m in (0, 1):
        for cases in GROUPS:
            log = sv.run_batch_host(*golden_arrays(golden, cases), math=m, max_records=0)
            for b, c in enumerate(cases):
                out[m][c] = (sv.sample_log(log, b), int(log.stop_reason[b]), _rng_after(log, b), int(log.n_records[b]))
    return out


@pytest.mark.parametrize("pre", CASES)
def test_libm_batch_is_the_reference_bit_for_bit(golden, uncapped, pre):
    log, reason, after, n = uncapped[0][pre]
    assert n == len(log) == len(golden[f"{pre}/value"])
    for name in ("kind", "node", "event_id", "value"):
        assert np.array_equal(log[name], golden[f"{pre}/{name}"]), name
    assert after == int(golden[f"{pre}/rng_after"]) and reason == 1


def test_a_sample_does_not_depend_on_its_position_or_on_b(golden, uncapped):
    a = golden_arrays(golden, ("wav1", "wav0", "wav1"))
    log = sv.run_batch_host(*a, math=0, max_records=0)
    for b, c in enumerate(("wav1", "wav0", "wav1")):
        assert np.array_equal(sv.sample_log(log, b), uncapped[0][c][0]) and _rng_after(log, b) == uncapped[0][c][2]
    one = sv.run_batch_host(*golden_arrays(golden, ("wav1",)), math=0, max_records=0)
    assert np.array_equal(sv.sample_log(one, 0), uncapped[0]["wav1"][0])


@pytest.mark.parametrize("pre", CASES)
def test_portable_math_keeps_the_event_structure(golden, uncapped, pre):
    log, reason, after, _n = uncapped[1][pre]
    want = golden[f"{pre}/value"]
    assert len(log) == len(want) and reason == 1
    for name in ("kind", "node", "event_id"):
        assert np.array_equal(log[name], golden[f"{pre}/{name}"]), name
    assert after == int(golden[f"{pre}/rng_after"])
    assert np.array_equal(np.floor(log["value"]), np.floor(want))
    rel = np.abs(log["value"] - want) / np.abs(want)
    print(pre, "max relative difference", rel.max(), "differing", float((rel > 0).mean()))
    assert rel.max() <= 10 * REL_MEASURED < 1e-11


def test_des_log_against_libm():
    rs = np.random.RandomState(5)
    edge = [2.0 ** -106, 2.0 ** -1022, 5e-324, np.nextafter(1.0, 0.0), np.nextafter(np.nextafter(1.0, 0.0), 0.0),
            1.0 - 2.0 ** -21, 1.0 - 2.0 ** -19, math.sqrt(0.5), np.nextafter(math.sqrt(0.5), 0.0),
            np.nextafter(math.sqrt(0.5), 1.0), 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)]
    x = np.concatenate([edge, rs.random_sample(120000), rs.random_sample(20000) * 2.0 ** -rs.randint(1, 200, 20000),
                        1.0 - rs.random_sample(10000) * 2.0 ** -rs.randint(1, 50, 10000)])
    x = x[(x > 0) & (x < 1)]
    assert len(x) >= 100000
    got, fac = sv.math_probe_host(x)
    want = np.array([math.log(v) for v in x])
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    print("des_log vs math.log: max", ulp.max(), "ulp; differing", float((ulp > 0).mean()))
    assert ulp.max() <= 2
    with np.errstate(over="ignore"):
        assert np.array_equal(fac, np.sqrt(-2.0 * got / x))            # numpy's sqrt is the correctly rounded one


def test_record_cap_gives_a_prefix(golden, uncapped):
    for cases in GROUPS[:2]:
        a = golden_arrays(golden, cases)
        log = sv.run_batch_host(*a, math=1, max_records=5001)
        assert log.n_records.tolist() == [5001] * len(cases) and log.stop_reason.tolist() == [RECORDS] * len(cases)
        assert log.rec_ptr.tolist() == [5001 * i for i in range(len(cases) + 1)]
        for b, c in enumerate(cases):
            assert np.array_equal(sv.sample_log(log, b), uncapped[1][c][0][:5001])
    a = golden_arrays(golden, ("hand",))
    log = sv.run_batch_host(*a, math=1, max_records=5001)             # larger than the run: nothing changes
    assert np.array_equal(sv.sample_log(log, 0), uncapped[1]["hand"][0]) and log.stop_reason.tolist() == [1]
    assert _rng_after(log, 0) == uncapped[1]["hand"][2]


def bound_cases(g):
    """hand-sized batch: [never-positive service, healthy, queue_cap 2, routed to a source] -> arrays."""
    adj, loc, scale, qcap, seed, cust, states = golden_arrays(g, ("hand",) * 4)
    loc, scale, qcap = np.array(loc), np.array(scale), np.array(qcap)
    servers = np.flatnonzero(np.diag(adj[0]) <= 0)
    loc[0, servers], scale[0, servers] = -5.0, 1e-3
    qcap[2, :] = 2
    loc[2, servers] *= 20.0                                            # slow servers: the queues of two fill up
    adj[3, 1, 0], adj[3, 1, 3] = 0.0, 0.5                              # `bad` of test_des_core: a customer reaches a source
    seed[3] = 3
    return adj, loc, scale, qcap, seed, cust, states


def test_bounds_end_a_sample_and_only_that_one(golden, uncapped):
    a = bound_cases(golden)
    log = sv.run_batch_host(*a, math=1, max_events=2000, max_records=0, max_queue_cap=254)
    # 0: the first service draw never turns positive: draw budget, not a spin; only the first arrival was logged
    assert log.stop_reason[0] == BUDGET and log.n_records[0] == 1 and sv.sample_log(log, 0)["kind"].tolist() == [0]
    # 1: the healthy neighbour is the golden run
    assert np.array_equal(sv.sample_log(log, 1), uncapped[1]["hand"][0]) and log.stop_reason[1] == 1
    # 2: queues of two: customers renege (fewer records than the healthy run), the ring holds
    l2 = sv.sample_log(log, 2)
    assert log.stop_reason[2] == 1 and len(l2) > 0
    reneged = 0
    for nd in np.unique(l2["node"]):
        arrivals = int(((l2["node"] == nd) & (l2["kind"] == 0)).sum())
        served = int(((l2["node"] == nd) & (l2["kind"] == 2)).sum())
        assert arrivals >= served
        reneged += max(0, arrivals - served - 2)                      # at most 2 may still be waiting at the end
    assert reneged > 0
    # 3: routed to a source: error, empty log
    assert log.stop_reason[3] == ERROR and log.n_records[3] == 0 and log.rec_ptr[4] == log.rec_ptr[3]
    # a queue_cap beyond the ring capacity is refused for that sample alone
    small = sv.run_batch_host(*a, math=1, max_events=2000, max_records=0, max_queue_cap=2)
    assert small.stop_reason.tolist() == [ERROR, ERROR, int(log.stop_reason[2]), ERROR]
    assert np.array_equal(sv.sample_log(small, 2), l2)
    with pytest.raises(Exception):
        sv.run_batch_host(*a, math=1, max_events=0)                   # max_events must be positive


def test_run_batch_takes_specs_and_leaves_numpys_stream(golden, uncapped):
    from gan_des_midi_music_gen_amd.matrix_sim_process import DesSpec
    specs, states = [], []
    for c in ("wav0", "wav1"):
        dist = [["normal", np.float32(a), np.float32(b)] for a, b in golden[f"{c}/dist"]]
        specs.append(DesSpec(golden[f"{c}/sim_matrix"], dist, list(golden[f"{c}/queue_list"]), golden[f"{c}/seeds"],
                             int(golden[f"{c}/customers"]), 0.5, np.zeros(15), np.zeros(15)))
        states.append(np.random.RandomState(SEEDS[c]).get_state())
    np.random.seed(9)
    log = sv.run_batch(specs, states=states)
    assert np.random.randint(0, 2 ** 31 - 1) == np.random.RandomState(9).randint(0, 2 ** 31 - 1)
    for b, c in enumerate(("wav0", "wav1")):
        assert np.array_equal(sv.sample_log(log, b), uncapped[1][c][0][:5001])


@pytest.mark.gpu
def test_batched_prologue_makes_the_prologues_specs_and_snapshots():
    import torch
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp
    g = load_golden("des_prologue.npz")

    def same(pro, specs, after):
        got = pro.specs()
        assert len(got) == len(specs) == len(pro.states)
        for a, b in zip(got, specs):
            assert np.array_equal(a.sim_matrix, b.sim_matrix) and np.array_equal(a.seeds, b.seeds)
            assert [[float(x) for x in d[1:]] for d in a.distributions] == [[float(x) for x in d[1:]] for d in b.distributions]
            assert a.num_customers == b.num_customers and list(a.queue_list) == list(b.queue_list)
            assert np.array_equal(a.note_levels, b.note_levels) and np.array_equal(a.instruments, b.instruments)
        assert np.random.randint(0, 2 ** 31 - 1) == after
        # the snapshot after sample i's reseed is RandomState(seed drawn for the reseed) advanced by the one randint that
        # makes the Sim seed: the state np.random.seed(s); np.random.randint(0, 99999, size=1) leaves
        for i, st in enumerate(pro.states):
            assert np.array_equal(pro.loc[i], [float(d[1]) for d in specs[i].distributions])
            assert np.array_equal(pro.scale[i], [float(d[2]) for d in specs[i].distributions])
            assert pro.seed[i] == int(specs[i].seeds[0]) and pro.customers[i] == specs[i].num_customers
        return got

    pre = "midi0"
    g1 = torch.from_numpy(g[f"{pre}/g1"][:, None]).cuda()
    g2 = torch.from_numpy(g[f"{pre}/g2"]).cuda()
    np.random.seed(int(g[f"{pre}/np_seed"]))
    specs = msp.midi_prologue(g1, g2, adj_size=(64, 64))
    after = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(int(g[f"{pre}/np_seed"]))
    pro = msp.batched_prologue_midi(g1, g2, adj_size=(64, 64))
    same(pro, specs, after)
    # the reference order, replayed by hand: the state right after each sample's reseed
    np.random.seed(int(g[f"{pre}/np_seed"]))
    h = msp.MIDI.scan(g1, 64, g2)
    for i in range(h["b"]):
        msp.MIDI.draws(h, i)
        want = np.random.get_state()
        got = pro.states[i]
        assert np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    m = torch.from_numpy(g["wav/matrices"]).cuda()
    np.random.seed(int(g["wav/np_seed"]))
    specs = msp.wav_prologue(m, size=20)
    after = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(int(g["wav/np_seed"]))
    pro = msp.batched_prologue_wav(m, size=20)
    same(pro, specs, after)
    np.random.seed(int(g["wav/np_seed"]))
    h = msp.WAV.scan(m, 20)
    for i in range(h["b"]):
        msp.WAV.draws(h, i)
        want = np.random.get_state()
        assert np.array_equal(pro.states[i][1], want[1]) and pro.states[i][2:] == want[2:]
