"""GPU: the log-free statistics kernel (gdm_des_stats_batch, csrc/des_stats.hip) on the branch-covering corpus of
tests/golden/des_corpus.npz, whose host mirror tests/test_des_stats.py pins to the reference's own accumulators
(tests/golden/des_stats.npz).

  * device equals host mirror (portable math) bit for bit -- every statistic, the histogram, stop reasons, final
    generator states -- for every corpus dim: 1, 2, 3, 5, 6 and 15 (node generators in LDS), 16 and 17 (in the
    workspace), 64 (one node per lane), 65 (a second lane pass), 128 (the maximum: the accumulators fill their LDS
    arrays); in file order and shuffled, the two error cases inside the dim-5 batches, with and without the histogram,
    a ring exactly as wide as the batch's largest capacity, and a guard word behind the exactly sized workspace;
  * device statistics against the device LOG of the same inputs (gdm_des_run_batch with a cap no run reaches): record
    counts, stop reasons, generator states, served = the node's 'processing' records, time_in_service = the sequential
    sum of their values.  (A sample that errors DURING its run keeps its generator state here, while the logging
    entries hand back the advanced one: states are compared on the samples that did not error.);
  * replicate(device=...) with 64 seeds equals the host's result bit for bit;
  * ops.des_run_stats refuses CPU tensors.
Each case is one or two launches of corpus-sized nets (at most 1059 records): milliseconds."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402
from test_des_corpus import DIMS, ERRORS, G, case_arrays, names_of_dim  # noqa: E402

DEV = "cuda"
ERROR = 3
FIELDS = sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS + ("is_source", "mt_pos", "has_gauss", "gauss")
GUARD = 0x5A


def cpu(t):
    return t.cpu().numpy()


def device_stats(arrays, histogram, max_queue_cap):
    """run_stats_device on an exactly sized workspace with guard bytes behind it."""
    b, dim = arrays[0].shape[0], arrays[0].shape[1]
    need = ops.des_stats_workspace_bytes(b, dim, max_queue_cap)
    buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=DEV)
    dev = sv.run_stats_device(*arrays, device=DEV, histogram=histogram, max_queue_cap=max_queue_cap,
                              workspace_tensor=buf[:need])
    assert bool((buf[need:] == GUARD).all()), "the kernel wrote behind its workspace"
    return dev


def assert_same(dev, host):
    for f in FIELDS:
        got, want = cpu(getattr(dev, f)), np.asarray(getattr(host, f))
        assert got.dtype == want.dtype and got.shape == want.shape, f
        assert got.tobytes() == want.tobytes(), f
    assert np.array_equal(cpu(dev.mt_key).view(np.uint32), host.mt_key)
    assert (dev.queue_time is None) == (host.queue_time is None)
    if host.queue_time is not None:
        assert cpu(dev.queue_time).tobytes() == host.queue_time.tobytes()


def orders_of(dim):
    names = names_of_dim(dim)
    out = [names]
    if len(names) > 1:
        rs = np.random.RandomState(100 + dim)
        out.append([names[i] for i in rs.permutation(len(names))] + [names[0]])
    return out


@pytest.mark.parametrize("histogram", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_device_equals_host_mirror(dim, histogram):
    assert DIMS == [1, 2, 3, 5, 6, 15, 16, 17, 64, 65, 128]
    for order in orders_of(dim):
        a = case_arrays(order)
        cap = max(1, int(a[3].max()))                             # no slack in the rings: their heads wrap
        host = sv.run_stats_host(*a, math=1, histogram=histogram, max_queue_cap=cap)
        assert_same(device_stats(a, histogram, cap), host)
        for b, n in enumerate(order):
            if n in ERRORS:
                assert host.stop_reason[b] == ERROR and not host.served[b].any() and host.clock[b] == 0, n
            else:
                assert host.stop_reason[b] in (0, 1), n
        if dim == 5:
            assert set(ERRORS) <= set(order)


def test_wide_rings_and_histogram():
    """The bridges' ring width (254 slots per server) on the queueing cases: 255 histogram columns per node."""
    a = case_arrays(["q_wrap3", "q_cap0", "err_to_source", "q_mix", "tie_a"])
    host = sv.run_stats_host(*a, math=1, histogram=True, max_queue_cap=254)
    assert_same(device_stats(a, True, 254), host)
    assert host.queue_time.shape == (5, 5, 255) and not host.queue_time[:, :, 4:].any() and host.max_queue.max() == 3


@pytest.mark.parametrize("dim", [5, 17, 128])
def test_device_statistics_against_the_device_log(dim):
    names = names_of_dim(dim)
    a = case_arrays(names)
    st = sv.run_stats_device(*a, device=DEV)
    log = sv.run_batch_device(*a, device=DEV, max_records=2048)
    n_rec, stop = cpu(log.n_records), cpu(log.stop_reason)
    assert n_rec.max() < 2048 and np.array_equal(cpu(st.n_records), n_rec) and np.array_equal(cpu(st.stop_reason), stop)
    ran = stop != ERROR
    for f in ("mt_key", "mt_pos", "has_gauss", "gauss"):
        assert cpu(getattr(st, f))[ran].tobytes() == cpu(getattr(log, f))[ran].tobytes(), f
    ptr, node, kind, value = cpu(log.rec_ptr), cpu(log.node), cpu(log.kind), cpu(log.value)
    served, tis = cpu(st.served), cpu(st.time_in_service)
    for b in range(len(names)):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        proc = kind[lo:hi] == sv.PROCESSING
        for i in range(dim):
            mine = value[lo:hi][proc & (node[lo:hi] == i)]
            assert served[b, i] == len(mine), (names[b], i)
            total = functools.reduce(lambda x, y: x + y, mine.tolist(), 0.0)
            assert np.float64(total).tobytes() == tis[b, i].tobytes(), (names[b], i)


def test_replications_on_the_device():
    n = "q_wrap3"
    spec = msp.DesSpec(G[f"{n}/sim_matrix"], [["normal", a, b] for a, b in G[f"{n}/dist"]], list(G[f"{n}/queue_list"]),
                       np.array([0]), int(G[f"{n}/customers"]), 1.0, np.zeros(5), np.zeros(5))
    seeds = np.arange(64) * 7 + 3
    host = sv.replicate(spec, seeds)
    dev = sv.replicate(spec, seeds, device=DEV)
    assert_same(dev.stats, host.stats)
    assert host.valid.all() and np.array_equal(dev.valid, host.valid)
    assert len({float(x) for x in host.stats.clock}) == 64        # 64 different runs
    for name in host.mean:
        for part in ("mean", "std", "sem", "n"):
            got, want = np.asarray(getattr(dev, part)[name]), np.asarray(getattr(host, part)[name])
            assert got.tobytes() == want.tobytes(), (name, part)
    assert (host.n["server_utilizations"][~G[f"{n}/w_is_source"].astype(bool)] == 64).all()


def test_cpu_tensors_are_refused():
    z = torch.zeros
    with pytest.raises(ops.GdmError):
        ops.des_run_stats(z(1, 2, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64),
                          z(1, 2, dtype=torch.int32), z(1, dtype=torch.int64), z(1, dtype=torch.int64),
                          z(1, 624, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.int32),
                          z(1, dtype=torch.float64), max_queue_cap=4)
