"""GPU: the batched simulator kernel (gdm_des_run_batch, csrc/des_batch.hip) on the branch-covering corpus of
tests/golden/des_corpus.npz (recorded from the reference's Sim; tests/test_des_corpus.py pins the host builds to it), at
the dims and batch sizes the kernel changes behaviour at and that tests/test_des_batch_gpu.py never ran: node generators
in the workspace right above their threshold (dim 16, 17), one node per lane at exactly 64 lanes' worth, the second
lane pass (65, 128 = the maximum), a ring exactly as wide as the largest capacity (the head wraps), the pack kernel's
scan beyond one 256-sample chunk with its carry (B = 300), errors between healthy samples.

Bar, as in test_des_batch_gpu.py whose helpers run everything here: device equals host mirror (portable math) bit for
bit -- records, rec_ptr, counts, stop reasons, final generator states -- with guard words behind every output and the
workspace.

Wall times measured on an MI355X (helpers.record: host mirror, uploads, both launches, guard checks and read-back of one
`both` call): 3 to 11 ms per dim group (dim 1: 0.33 s, the process's first launch; dim 128, 1059 records at 776 KB of
workspace: 5 ms), 20 ms for the eight exact-stride launches, 5 ms for the B = 300 pack batch, 4 ms for the error batch;
the whole file takes 2.5 s.  DESIGN.md section 7 quotes the same figures."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import simulation_v3 as sv  # noqa: E402
from helpers import record  # noqa: E402
from test_des_batch import ERROR, RECORDS  # noqa: E402
from test_des_batch_gpu import both  # noqa: E402
from test_des_corpus import DIMS, ERRORS, G, NAMES, case_arrays, n_seeds, names_of_dim, recording  # noqa: E402

CAP = 1300                      # above the longest run of the corpus (1059 records): uncapped in effect


def timed(name, fn):
    t0 = time.perf_counter()
    out = fn()
    record(f"des_corpus_gpu/{name}", seconds=round(time.perf_counter() - t0, 3))
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_whole_corpus_by_dim(dim):
    """One launch per dim: 1, 2, 3, 5, 6 (LDS generators), 15 (their last dim), 16, 17 (workspace generators), 64 (every
    lane sets up a node), 65 (one node in a second pass), 128 (two full passes)."""
    names = names_of_dim(dim)
    host = timed(f"dim{dim}", lambda: both(case_arrays(names), CAP))
    for b, n in enumerate(names):
        if n in ERRORS:
            assert host.stop_reason[b] == ERROR and host.n_records[b] == 0, n
            continue
        log, want = sv.sample_log(host, b), recording(n)
        if n_seeds(n) == 1:                                       # the whole run, structurally the reference's
            assert len(log) == len(want) and host.stop_reason[b] in (0, 1), n
        for f in ("kind", "node", "event_id"):
            assert np.array_equal(log[f], want[f][:len(log)]), (n, f)
    assert DIMS == [1, 2, 3, 5, 6, 15, 16, 17, 64, 65, 128]


QUEUE_CASES = ("q_cap0", "q_cap1", "q_cap2", "q_mix", "q_wrap3", "tie_a", "tie_e", "draw_scale0")


def test_ring_stride_equal_to_the_largest_capacity():
    """max_queue_cap = the case's largest capacity (at least 1) instead of 254: the ring has no slack and its head wraps
    (q_wrap3: capacity 3 everywhere, more than 20 customers through one queue)."""
    assert ((G["q_wrap3/queue_list"] == 3).all() and (G["q_wrap3/w_from_queue"] >= 20).any())

    def run():
        for n in QUEUE_CASES:
            stride = max(1, int(G[f"{n}/queue_list"].max()))
            assert stride <= 3, n
            host = both(case_arrays([n]), CAP, max_queue_cap=stride)
            log, want = sv.sample_log(host, 0), recording(n)
            assert len(log) == len(want) and host.stop_reason[0] == 1, n
            for f in ("kind", "node", "event_id"):
                assert np.array_equal(log[f], want[f]), (n, f)
    timed("ring_stride", run)


def pack_batch(b=300, max_records=320):
    """300 ragged dim-5 samples cycled from the corpus with their own seeds, states and customer counts; at 0, 255, 256
    and 299: a sample that reaches max_records exactly, an error sample, a sample of more than 256 records after shorter
    ones, a sample without sources."""
    cycle = ("q_cap1", "tie_a", "draw_scale0", "sink_node0_server", "draw_backwards", "q_wrap3", "stop_n4")
    special = {0: "q_wrap3", 255: "err_to_source", 256: "tie_e", 299: "q_cap1"}
    names = [special.get(i, cycle[i % len(cycle)]) for i in range(b)]
    adj, loc, scale, qcap, seed, cust, _ = case_arrays(names)
    states = []
    for i in range(b):
        rs = np.random.RandomState(500 + i)
        if i % 5 == 3:                                            # mid-stream, with a cached gauss
            rs.standard_normal(1 + i % 3)
            rs.random_sample(i)
        states.append(rs.get_state())
        if i not in special:
            seed[i], cust[i] = 1000 + 13 * i, 6 + (i * 7) % 15
    adj[299][np.diag_indices(5)] = -1.0                           # no sources: nothing ever happens
    return (adj, loc, scale, qcap, seed, cust, states), max_records


def test_pack_kernel_beyond_one_scan_chunk():
    a, max_records = pack_batch()
    host = timed("pack_b300", lambda: both(a, max_records, max_queue_cap=6))
    n = host.n_records
    assert n[0] == max_records and host.stop_reason[0] == RECORDS
    assert n[255] == 0 and host.stop_reason[255] == ERROR
    assert 256 < n[256] < max_records and n[256] > n[:256][1:].max() and host.stop_reason[256] == 1
    assert n[299] == 0 and host.stop_reason[299] == 0
    assert len(set(n.tolist())) > 20 and (n[1:255] > 0).all() and n[1:255].max() <= 150
    assert host.rec_ptr.tolist() == [0] + np.cumsum(n).tolist()
    for b in range(len(n)):                                       # each row against its own single-sample run
        one = sv.run_batch_host(*(x[b:b + 1] for x in a), math=1, max_records=max_records, max_queue_cap=6)
        assert sv.sample_log(host, b).tobytes() == sv.sample_log(one, 0).tobytes(), b
        assert np.array_equal(host.mt_key[b], one.mt_key[0]) and host.mt_pos[b] == one.mt_pos[0], b
        assert host.stop_reason[b] == one.stop_reason[0], b


def test_errors_in_a_device_batch():
    names = ["q_cap1", "err_to_source", "stop_n4", "err_source_childless", "tie_a"]
    assert set(names[1::2]) == set(ERRORS) <= set(NAMES)
    host = timed("errors", lambda: both(case_arrays(names), CAP))
    assert host.stop_reason.tolist() == [1, ERROR, 1, ERROR, 1] and host.n_records.tolist()[1::2] == [0, 0]
    assert host.rec_ptr[1] == host.rec_ptr[2] and host.rec_ptr[3] == host.rec_ptr[4]
    for b in (0, 2, 4):
        log, want = sv.sample_log(host, b), recording(names[b])
        one = sv.run_batch_host(*case_arrays([names[b]]), math=1, max_records=CAP)
        assert log.tobytes() == sv.sample_log(one, 0).tobytes() and len(log) == len(want)
        for f in ("kind", "node", "event_id"):
            assert np.array_equal(log[f], want[f]), (names[b], f)
