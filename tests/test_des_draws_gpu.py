"""GPU: the draws kernel (gdm_des_draws, csrc/des_draws.hip) against its host mirror gdm_des_draws_host -- the same
csrc/des_draws.h compiled for the host, which tests/test_des_draws.py pins to numpy itself.

Bar: equal bits in every output buffer, error-status samples included.  Every output is a guarded buffer: the 256
sentinel bytes on both sides must be intact.  The wav route reads an (S, S) matrix with S = dim + 5 <= 64 and draws
S / 8 >= 1 sources, so its node counts are 4, 15 and 59 where the MIDI route runs 1, 4, 15 and 61."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops  # noqa: E402

DEV = torch.device("cuda")
CANARY = 0x5A


def _guarded_outputs(b, dim):
    shapes = {"d": (b, dim), "": (b,), "k": (b, 624)}
    whole, out = [], {}
    for name, dt, kind in ops._DES_DRAWS_FIELDS:
        n = int(np.prod(shapes[kind])) * torch.empty(0, dtype=dt).element_size()
        buf = torch.full((256 + n + (-n) % 256 + 256,), CANARY, dtype=torch.uint8, device=DEV)
        whole.append((name, buf, n))
        out[name] = buf[256:256 + n].view(dt).reshape(shapes[kind])
    return whole, out


def _inputs(route, b, dim, seed):
    rng = np.random.default_rng(seed)
    size = dim + (3 if route == ops.DES_DRAWS_MIDI else 5)
    density = rng.choice([0.0, 0.5, 0.9], size=b)
    zero = rng.random((b, dim, dim)) < density[:, None, None]
    if b > 2:
        zero[2, dim // 2, :] = True                                     # a row without candidates: status 1
    words = np.zeros((b, dim), dtype=np.uint64)
    for x in range(dim):
        words |= zero[:, :, x].astype(np.uint64) << np.uint64(x)
    base = rng.integers(0, 2 ** 32, size=b, dtype=np.uint64).astype(np.uint32)
    base[0], base[-1] = 0, 2 ** 32 - 1
    inst = rng.integers(0, 127, size=(b, dim)).astype(np.int32)
    notes = rng.integers(0, 128, size=(b, dim)).astype(np.int32)
    over = np.where(rng.random(b) < 0.5, ops.DES_DRAWS_NO_INSTRUMENT, rng.integers(0, 128, size=b)).astype(np.int32)
    thr = None
    if route == ops.DES_DRAWS_MIDI:
        params = rng.standard_normal((b, 16)).astype(np.float32)
        params[:, 6] = rng.choice([-1.0, 0.01, 0.2, 0.9, 5.0], size=b)
        if b > 1:
            params[1, 6] = np.inf                                       # status 5
    else:
        params = rng.random((b, 2, dim)).astype(np.float32)
        thr = np.zeros((b, size), dtype=np.uint8)
        for i in range(b):
            kind = i % 5                                                # none, one, two (status 2), >= dim (3), none
            if kind == 1:
                thr[i, rng.integers(0, dim)] = 1
            elif kind == 2:
                thr[i, 0] = thr[i, size - 1] = 1
            elif kind == 3:
                thr[i, dim + rng.integers(0, 5)] = 1
    return size, base, words.view(np.int64), thr, inst, notes, params, over


@pytest.mark.parametrize("b", [1, 3, 64, 130])
@pytest.mark.parametrize("route,dim", [(0, 1), (0, 4), (0, 15), (0, 61), (1, 4), (1, 15), (1, 59)])
def test_kernel_equals_host_mirror_bit_for_bit(route, dim, b):
    size, base, zmask, thr, inst, notes, params, over = _inputs(route, b, dim, 100 * dim + b + route)
    want = msp.des_draws_host(route, size, dim, base, zmask, inst, notes, params, thr_mask=thr, instrument_override=over)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    scan = {"zero_mask": up(zmask), "instruments": up(inst), "note_levels": up(notes), "thr_mask": up(thr)}
    whole, out = _guarded_outputs(b, dim)
    got = ops.des_draws(route, size, dim, up(base.view(np.int32)), scan, up(params), up(over), out=out)
    torch.cuda.synchronize()
    for name, buf, n in whole:
        host = buf.cpu().numpy()
        assert (host[:256] == CANARY).all() and (host[256 + n:] == CANARY).all(), f"{name}: guard bytes overwritten"
        g = got[name].cpu().numpy()
        w = want[name]
        assert g.tobytes() == w.tobytes(), f"{name} differs (route {route}, dim {dim}, B {b})"
    status = want["status"]
    if b >= 64:
        seen = set(status.tolist())
        assert (dim == 1 or 0 in seen) and 1 in seen and (route == 0 or {2, 3} <= seen) and (route == 1 or 5 in seen)
        if dim > 1:
            assert (status == 0).sum() >= b // 8


def test_wrapper_refuses_what_the_kernel_cannot_take():
    z = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    i4 = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    base = torch.zeros(2, dtype=torch.int32, device=DEV)
    scan = {"zero_mask": z, "instruments": i4, "note_levels": i4, "thr_mask": None}
    with pytest.raises(ops.GdmError):
        ops.des_draws(ops.DES_DRAWS_MIDI, 7, 4, base, scan, torch.zeros((2, 6), device=DEV))           # gen2 too narrow
    with pytest.raises(ops.GdmError):
        ops.des_draws(ops.DES_DRAWS_WAV, 9, 4, base, scan, torch.zeros((2, 2, 4), device=DEV))         # no thr_mask
    with pytest.raises(ops.GdmError):
        ops.des_draws(ops.DES_DRAWS_MIDI, 7, 4, base.cpu(), scan, torch.zeros((2, 16), device=DEV))
