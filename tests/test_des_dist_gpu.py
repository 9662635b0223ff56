"""GPU: the statistics kernel with a distribution kind per node (gdm_des_stats_batch_dist, des_stats_dist_kernel in
csrc/des_stats.hip) on the nets of tests/golden/des_dist.npz, whose host mirror tests/test_des_dist.py pins to the
reference's own accumulators.

  * device equals host mirror (run_stats_host(kind=..., math=1)) bit for bit -- every statistic, the histogram on and
    off, stop reasons, final generator states -- for dims 2, 3, 5, 6 and 15 (node generators in LDS), 16 and 17 (in the
    workspace), 64 (one node per lane), 65 (rand64 with an idle node: a second lane pass) and 128 (the maximum: the
    kinds fill their LDS row); in file order and shuffled; with an exactly sized workspace and guard bytes behind it;
  * one batch that holds every kind mix -- the recorded one, all normal, all exponential, all uniform -- and the
    refused samples: a kind the device entry cannot check on the host (3: the sample stops with an error, zeros, its
    generator state kept) and an exponential server with scale 0;
  * all-normal kinds through the new kernel give the bytes of gdm_des_stats_batch on the corpus of des_corpus.npz,
    dims 5 and 128;
  * mm1k_sweep(device=...) with the recorded grid's 6 configurations x 64 seeds x 4000 customers in ONE launch (about
    8000 events per sample): equal to the host mirror bit for bit, every |z| <= 4;
  * ops.des_run_stats_dist refuses CPU tensors.
Apart from the sweep each case is one or two launches of nets with at most 4667 records: milliseconds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops, simulation_v3 as sv  # noqa: E402
from test_des_corpus import case_arrays, names_of_dim  # noqa: E402
from test_des_dist import D, DIMS, ERROR, check_z, dist_case_arrays, dist_names_of_dim, dist_state0  # noqa: E402
from test_des_stats_gpu import DEV, FIELDS, GUARD, assert_same, cpu  # noqa: E402


def device_stats(arrays, kind, histogram, max_queue_cap):
    """run_stats_device(kind=...) on an exactly sized workspace with guard bytes behind it."""
    b, dim = arrays[0].shape[0], arrays[0].shape[1]
    need = ops.des_stats_workspace_bytes(b, dim, max_queue_cap)
    buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=DEV)
    dev = sv.run_stats_device(*arrays, device=DEV, histogram=histogram, max_queue_cap=max_queue_cap,
                              workspace_tensor=buf[:need], kind=kind)
    assert bool((buf[need:] == GUARD).all()), "the kernel wrote behind its workspace"
    return dev


def padded(arrays, kind):
    """The cases with one more node nobody routes to: an idle exponential server at the end."""
    adj, loc, scale, qcap, seed, cust, states = arrays
    b, dim = adj.shape[0], adj.shape[1]
    big = np.zeros((b, dim + 1, dim + 1))
    big[:, :dim, :dim] = adj

    def more(a, v):
        return np.concatenate([a, np.full((b, 1), v, dtype=a.dtype)], axis=1)

    return (big, more(loc, 0.0), more(scale, 0.25), more(qcap, 1), seed, cust, states), more(kind, 1)


def orders_of(dim):
    if dim == 65:
        return [("pad", n) for n in orders_of(64)]
    names = dist_names_of_dim(dim)
    out = [names]
    if len(names) > 1:
        rs = np.random.RandomState(200 + dim)
        out.append([names[i] for i in rs.permutation(len(names))] + [names[0]])
    return out


@pytest.mark.parametrize("histogram", [False, True])
@pytest.mark.parametrize("dim", [2, 3, 5, 6, 15, 16, 17, 64, 65, 128])
def test_device_equals_host_mirror(dim, histogram):
    assert DIMS == [2, 3, 5, 6, 15, 16, 17, 64, 128]
    for order in orders_of(dim):
        if dim == 65:
            a, kind = padded(*dist_case_arrays(order[1]))
            assert a[0].shape[1:] == (65, 65)
        else:
            a, kind = dist_case_arrays(order)
        cap = max(1, int(a[3].max()))                             # no slack in the rings: their heads wrap
        host = sv.run_stats_host(*a, math=1, histogram=histogram, max_queue_cap=cap, kind=kind)
        assert (host.stop_reason == 1).all() and host.served.sum() > 0
        assert_same(device_stats(a, kind, histogram, cap), host)


def test_every_kind_mix_and_the_refused_samples_in_one_batch():
    names = ["mix5"] * 6
    a, kind = dist_case_arrays(names)
    adj, loc, scale = a[0], a[1].copy(), a[2].copy()
    loc[:, :] = np.maximum(loc, 0.25)                             # (an exponential's loc is 0: give the other kinds one)
    kind[1], kind[2], kind[3] = 0, 1, 2
    kind[4, 3] = 3                                                # the device entry cannot see this on the host
    kind[5, 3], scale[5, 3] = 1, 0.0                              # an exponential server that only ever gives 0.0
    arrays = (adj, loc, scale, *a[3:])
    cap = int(a[3].max())
    valid = kind.copy()
    valid[4, 3] = 0                                               # (the host entry refuses the whole call for kind 3)
    host = sv.run_stats_host(*arrays, math=1, histogram=True, max_queue_cap=cap, kind=valid)
    assert host.stop_reason.tolist() == [1, 1, 1, 1, 1, ERROR]
    dev = device_stats(arrays, kind, True, cap)
    keep = np.array([0, 1, 2, 3, 5])
    for f in FIELDS + ("queue_time", "mt_key"):
        got, want = cpu(getattr(dev, f)), np.asarray(getattr(host, f))
        assert got[keep].tobytes() == want[keep].view(got.dtype).tobytes(), f
    assert len({cpu(dev.clock)[b].tobytes() for b in range(4)}) == 4          # four different runs
    assert int(cpu(dev.stop_reason)[4]) == ERROR
    for f in sv.STATS_NODE_FIELDS + ("clock", "end_time", "total_customers", "events", "n_records", "queue_time"):
        assert not cpu(getattr(dev, f))[4].any(), f
    assert not cpu(dev.served)[5].any() and cpu(dev.clock)[5] == 0
    for b in (4, 5):
        st0 = dist_state0("mix5")
        assert np.array_equal(cpu(dev.mt_key)[b].view(np.uint32), st0[1]) and int(cpu(dev.mt_pos)[b]) == st0[2]
        assert int(cpu(dev.has_gauss)[b]) == st0[3] and float(cpu(dev.gauss)[b]) == st0[4]


@pytest.mark.parametrize("dim", [5, 128])
def test_all_normal_kinds_are_the_existing_kernel(dim):
    a = case_arrays(names_of_dim(dim))
    cap = max(1, int(a[3].max()))
    old = sv.run_stats_device(*a, device=DEV, histogram=True, max_queue_cap=cap)
    new = device_stats(a, np.zeros(a[1].shape, dtype=np.int32), True, cap)
    for f in FIELDS + ("queue_time", "mt_key"):
        assert cpu(getattr(new, f)).tobytes() == cpu(getattr(old, f)).tobytes(), f
    assert int((cpu(old.stop_reason) == ERROR).sum()) == (2 if dim == 5 else 0)


def test_sweep_in_one_launch():
    cfg = D["grid/config"]
    lams, mus, caps = cfg[:, 0], cfg[:, 1], cfg[:, 2].astype(int)
    seeds = np.arange(64) * 11 + 5
    customers = int(D["grid/customers"])
    assert len(lams) == 6 and customers == 4000
    sweep = sv.mm1k_sweep(lams, mus, caps, seeds, customers=customers, device=DEV)
    st = sweep.stats
    assert st.served.shape == (384, 2) and bool((st.stop_reason == 1).all())
    events = cpu(st.events)
    print("events per sample: min", events.min(), "mean", events.mean(), "max", events.max())
    host = sv.mm1k_sweep(lams, mus, caps, seeds, customers=customers)        # the host mirror, portable math
    assert_same(st, host.stats)
    for name in sv.SWEEP_NAMES:
        for part in ("values", "mean", "sem", "n", "theory", "z"):
            assert np.asarray(getattr(sweep, part)[name]).tobytes() == np.asarray(getattr(host, part)[name]).tobytes()
    check_z(sweep, 64)


def test_cpu_tensors_are_refused():
    z = torch.zeros
    with pytest.raises(ops.GdmError):
        ops.des_run_stats_dist(z(1, 2, 2, dtype=torch.float64), z(1, 2, dtype=torch.float64),
                               z(1, 2, dtype=torch.float64), z(1, 2, dtype=torch.int32), z(1, 2, dtype=torch.int32),
                               z(1, dtype=torch.int64), z(1, dtype=torch.int64), z(1, 624, dtype=torch.int32),
                               z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.float64),
                               max_queue_cap=4)
