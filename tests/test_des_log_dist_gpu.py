"""GPU: the logging kernel with a distribution kind per node (gdm_des_run_batch_dist, des_batch_dist_kernel in
csrc/des_batch.hip) on the nets of tests/golden/des_dist.npz, whose host mirror tests/test_des_log_dist.py pins to the
reference's own logs.

  1. device equals host mirror (run_batch_host(kind=..., math=1)) bit for bit -- records, rec_ptr, n_records, stop
     reasons, final generator states -- one launch per dim: 2, 3, 5, 6, 15 (node generators in LDS), 16 (kLdsGenDim's
     boundary: the first dim with the generators in the workspace), 17, 64 (one node per lane) and 128 (the maximum: the
     kinds fill their LDS row); on an exactly sized workspace with guard bytes behind it;
  2. all-normal kinds through the new kernel give the bytes of gdm_des_run_batch on the corpus of des_corpus.npz, dims
     2, 16 and 128;
  3. a refused sample inside a batch of 3 -- a kind the device entry cannot check on the host, and an exponential
     server with scale 0 --: reason 3, an empty log, its generator state kept, its neighbours intact;
  4. one exponential log through log_to_notes gives the notes of the host log through the same call.
Every case is one or two launches of nets with at most 4667 records: milliseconds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops, sim_log_process_music as slpm, simulation_v3 as sv  # noqa: E402
from test_des_corpus import case_arrays, names_of_dim, same_state  # noqa: E402
from test_des_dist import DIMS, ERROR, dist_case_arrays, dist_names_of_dim, dist_state0  # noqa: E402

DEV = "cuda"
GUARD = 0x5A
MAX_RECORDS = 5001
LOG_FIELDS = ("value", "event_id", "node", "kind", "rec_ptr", "n_records", "stop_reason", "mt_pos", "has_gauss", "gauss")


def device_log(arrays, kind, max_queue_cap):
    """run_batch_device(kind=...) on an exactly sized workspace with guard bytes behind it."""
    b, dim = arrays[0].shape[0], arrays[0].shape[1]
    need = ops.des_batch_workspace_bytes(b, dim, max_queue_cap)
    buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=DEV)
    dev = sv.run_batch_device(*arrays, device=DEV, max_records=MAX_RECORDS, max_queue_cap=max_queue_cap,
                              workspace_tensor=buf[:need], kind=kind)
    assert bool((buf[need:] == GUARD).all()), "the kernel wrote behind its workspace"
    return dev


def assert_same_log(dev, host):
    n = int(host.rec_ptr[-1])
    for f in LOG_FIELDS:
        got, want = getattr(dev, f).cpu().numpy(), np.asarray(getattr(host, f))
        if f in ("value", "event_id", "node", "kind"):
            got = got[:n]
        assert got.dtype == want.dtype and got.shape == want.shape, f
        assert got.tobytes() == want.tobytes(), f
    assert np.array_equal(dev.mt_key.cpu().numpy().view(np.uint32), host.mt_key)


@pytest.mark.parametrize("dim", DIMS)
def test_device_log_is_the_host_mirrors(dim):
    assert DIMS == [2, 3, 5, 6, 15, 16, 17, 64, 128]
    arrays, kind = dist_case_arrays(dist_names_of_dim(dim))
    cap = max(1, int(arrays[3].max()))
    host = sv.run_batch_host(*arrays, math=1, max_records=MAX_RECORDS, kind=kind)
    assert (host.stop_reason == 1).all() and host.n_records.min() >= 60
    assert_same_log(device_log(arrays, kind, cap), host)


@pytest.mark.parametrize("dim", [2, 16, 128])
def test_all_normal_kinds_are_the_existing_kernel(dim):
    arrays = case_arrays(names_of_dim(dim))
    cap = max(1, int(arrays[3].max()))
    old = sv.run_batch_device(*arrays, device=DEV, max_records=MAX_RECORDS, max_queue_cap=cap)
    new = device_log(arrays, np.zeros(arrays[1].shape, dtype=np.int32), cap)
    n = int(old.rec_ptr[-1])
    assert n > 0
    for f in LOG_FIELDS + ("mt_key",):
        got, want = getattr(new, f).cpu().numpy(), getattr(old, f).cpu().numpy()
        if f in ("value", "event_id", "node", "kind"):
            got, want = got[:n], want[:n]
        assert got.tobytes() == want.tobytes(), f


@pytest.mark.parametrize("how", ["kind", "scale0"])
def test_a_refused_sample_leaves_its_neighbours_alone(how):
    names = ["uni_neg", "uni_neg", "scale0_srv"]          # uni_neg: 0 -> 1 -> 2
    arrays, kind = dist_case_arrays(names)
    scale = arrays[2].copy()
    if how == "kind":
        kind[1, 2] = 3                                    # only the device entry lets this through to the sample
    else:
        kind[1, 1], scale[1, 1] = 1, 0.0                  # an exponential server that only ever gives 0.0
    arrays = arrays[:2] + (scale,) + arrays[3:]
    dev = device_log(arrays, kind, int(arrays[3].max()))
    assert dev.stop_reason.tolist() == [1, ERROR, 1] and dev.n_records.tolist()[1] == 0
    ptr = dev.rec_ptr.tolist()
    assert ptr[1] == ptr[2] and ptr[3] > ptr[2] > 0
    assert same_state(sv.state_of(dev, 1), dist_state0(names[1]))
    for b, name in ((0, "uni_neg"), (2, "scale0_srv")):
        a, k = dist_case_arrays([name])
        want = sv.run_batch_host(*a, math=1, max_records=MAX_RECORDS, kind=k)
        for f in ("value", "event_id", "node", "kind"):
            assert getattr(dev, f)[ptr[b]:ptr[b + 1]].cpu().numpy().tobytes() == getattr(want, f).tobytes(), (b, f)
        assert same_state(sv.state_of(dev, b), sv.state_of(want, 0)), b


def test_an_exponential_log_gives_the_host_logs_notes():
    arrays, kind = dist_case_arrays(["exp2"])
    host = sv.run_batch_host(*arrays, math=1, max_records=MAX_RECORDS, kind=kind)
    dev = device_log(arrays, kind, int(arrays[3].max()))
    down = sv.BatchLog(*(t.cpu().numpy() for t in dev))
    instruments, levels = [[0, 0]], [[60, 64]]
    got = slpm.log_to_notes([sv.sample_log(down, 0)], instruments, levels, device=DEV)
    want = slpm.log_to_notes([sv.sample_log(host, 0)], instruments, levels, device=DEV)
    assert int(want[1][0]) > 10
    for g, w in zip(got, want):
        assert torch.equal(g, w)
