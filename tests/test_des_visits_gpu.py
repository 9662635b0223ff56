"""GPU: simulation_v3.log_visits and what is built on it, fed with logs that the DEVICE simulator wrote.

These tests launch EXISTING kernels only (gdm_des_run_batch, gdm_des_run_batch_dist, gdm_des_run_batch_net and the
statistics kernels beside them): the visit walk has no kernel and no device entry -- a device log is read back once
and walked by gdm_des_log_visits_host.  What they pin is the path from a device BatchLog into
the walk, and that the per-node identities of tests/test_des_visits.py tie the device's log run to the device's
statistics run as they tie the host's.

  1. on the corpus nets at dims 3, 16 and 128 and on two queue nets (det_tie and c4, whose runs both end while the queue
     node holds a customer back) log_visits(run_batch_device(...)) is byte-equal to log_visits(run_batch_host(math=1)),
     and visit_stats of the device log agrees with run_stats_device by the identities of test_des_visits.py (item 4);
  2. mm1k_wait_sweep(device=...) on 5 configurations x 4 seeds x 400 customers is bit-equal to its host result.
Every case is a few launches of nets with at most 3698 records: milliseconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import simulation_v3 as sv  # noqa: E402
from test_des_corpus import case_arrays, names_of_dim  # noqa: E402
from test_des_net import net_case_arrays  # noqa: E402
from test_des_visits import SWEEP, SWEEP_TS, check_identities, pending_delays  # noqa: E402

DEV = "cuda"
CAP = 1300                      # above the longest run of the corpus (1059 records): uncapped in effect
NET_CAP = 5001                  # above the longest run of des_net.npz (3698 records)


def host_stats(stats):
    """A device BatchStats as numpy arrays."""
    return sv.BatchStats(*(None if a is None else a.cpu().numpy() for a in stats))


def assert_same_visits(dev, host):
    for f in sv.LogVisits._fields:
        got, want = getattr(dev, f), getattr(host, f)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), f


@pytest.mark.parametrize("dim", [3, 16, 128])
def test_corpus_logs_from_the_device(dim):
    names = names_of_dim(dim)
    a = case_arrays(names)
    host = sv.run_batch_host(*a, math=1, max_records=CAP)
    assert 0 < host.n_records.max() < CAP
    dev = sv.run_batch_device(*a, device=DEV, max_records=CAP)
    hv, dv = sv.log_visits(host, dim=dim), sv.log_visits(dev, dim=dim)
    assert not hv.status.any() and hv.visit_ptr[-1] > 100
    assert_same_visits(dv, hv)
    stats = host_stats(sv.run_stats_device(*a, device=DEV))
    check_identities(sv.visit_stats(dv, dim), dv, stats, np.asarray(a[3]), None, names)


@pytest.mark.parametrize("name", ["det_tie", "c4"])
def test_queue_net_logs_from_the_device(name):
    a, kind = net_case_arrays([name])
    dim = a[0].shape[1]
    host = sv.run_batch_host(*a, math=1, max_records=NET_CAP, kind=kind, net=True)
    assert host.stop_reason.tolist() == [1] and 400 <= host.n_records[0] < NET_CAP
    dev = sv.run_batch_device(*a, device=DEV, max_records=NET_CAP, kind=kind, net=True)
    hv, dv = sv.log_visits(host, dim=dim), sv.log_visits(dev, dim=dim)
    assert not hv.status.any() and (hv.n_departures > 1).any()
    assert_same_visits(dv, hv)
    stats = host_stats(sv.run_stats_device(*a, device=DEV, kind=kind, net=True))
    pending = pending_delays(a, kind, host, dv)           # (the longer run is the host mirror's: the same bits)
    assert (pending != 0).sum() == 1
    worst = [0.0]
    check_identities(sv.visit_stats(dv, dim), dv, stats, None, kind, [name], worst, pending)
    print(name, "largest |wait_sum + blocked_sum + pending - time_in_queue| / bound:", worst[0])


def test_wait_sweep_on_the_device_is_the_host_sweep():
    seeds = [100, 101, 102, 103]
    kw = dict(seeds=seeds, ts=SWEEP_TS, customers=400, skip=50)
    host = sv.mm1k_wait_sweep(**SWEEP, **kw)              # the host mirror, portable math
    dev = sv.mm1k_wait_sweep(**SWEEP, **kw, device=DEV)
    assert host.values.shape == (5, 4, 4) and (host.stop_reason == 1).all() and host.visits.visit_ptr[-1] > 5 * 4 * 350
    assert_same_visits(dev.visits, host.visits)
    for part in ("lam", "mu", "queue_cap", "seeds", "ts", "stop_reason", "values", "mean", "sem", "n", "theory", "z"):
        got, want = np.asarray(getattr(dev, part)), np.asarray(getattr(host, part))
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), part
