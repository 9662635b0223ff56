"""GPU: the DES bridge prologue kernels ``gdm_des_scan`` / ``gdm_des_routing`` (csrc/des_prologue.hip) and the in-place
compaction ``gdm_des_pack`` (csrc/des_batch.hip) against the numpy references of tests/des_prologue_ref.py, at every
geometry of its tables and at the value edges the header comment of des_prologue.hip promises.  The references are
pinned to the oracle on the CPU (test_des_prologue_ref.py), where the tables are also shown to tell a wrong summation
order, a missing abs and ``>=`` at the threshold apart.

All of it is integer or float64-bit-exact work: every comparison is of integers or bit patterns, every element of every
output is compared (but the unspecified tail of the packed arrays), and the one rule is that any NaN equals any NaN
(0/0 in an all-zero aux row: host and device default NaNs differ in sign).

What these cases found when they were written: ``test_scan_value_edges`` (both forms) failed on the three samples that
hold a NaN -- the scan's exponent-mask test had been compiled, NaNs assumed away, into ``|v| == inf``, so a NaN raised no
flag (±inf did).  Everything else -- 117 of the 119 cases -- held bit for bit before any change to the kernels but the
int32 limit (``test_the_integer_limit_through_the_package``).  The file runs in about 3.5 s."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402
from oracle import des_prologue as odp  # noqa: E402  (checker only)

import des_prologue_ref as R  # noqa: E402
from test_des_device_bridge_gpu import _numpy_prologue  # noqa: E402
from test_des_prologue_gpu import _same  # noqa: E402

DEV = "cuda"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(m, gap=37):
    """The batch as a view with stride(0) = S*S + gap into a buffer whose gaps hold NaN."""
    b, s = m.shape[0], m.shape[1]
    buf = torch.full((b, s * s + gap), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :s * s] = _up(m).reshape(b, s * s)
    g = buf[:, :s * s].view(b, s, s)
    assert g.stride(0) == s * s + gap and g.stride(1) == s and g.stride(2) == 1
    return g


def _first(bad):
    return np.argwhere(bad)[0].tolist() if bad.any() else None


# ---- A: gdm_des_scan -------------------------------------------------------------------------------------------------
def _check_scan(form, S, dim, m, g=None, names=None):
    args = R.SCAN_ARGS[form]
    got = ops.des_scan(_up(m) if g is None else g, S, dim, **args)
    want = [R.scan_ref(x, S, dim, **args) for x in m]
    what = (form, S, dim, len(m))
    for key in ("instruments", "note_levels"):
        ref = np.array([w[key] for w in want], dtype=np.int64)
        out = got[key].cpu().numpy()
        assert out.dtype == np.int32 and out.shape == ref.shape
        assert np.array_equal(out.astype(np.int64), ref), (what, key, _first(out != ref), names)
    ref = np.array([w["zero_mask"] for w in want], dtype=np.uint64)
    out = got["zero_mask"].cpu().numpy().view(np.uint64)
    assert out.shape == ref.shape and np.array_equal(out, ref), (what, "zero_mask", _first(out != ref), names)
    ref = np.array([w["flag"] for w in want], dtype=np.int32)
    out = got["flags"].cpu().numpy()
    assert out.dtype == np.int32 and np.array_equal(out, ref), (what, "flags", out.tolist(), ref.tolist(), names)
    if args["threshold"] is None:
        assert got["thr_mask"] is None and got["aux"] is None
    else:
        ref = np.stack([w["thr_mask"] for w in want])
        out = got["thr_mask"].cpu().numpy()
        assert out.dtype == np.uint8 and out.shape == ref.shape
        assert np.array_equal(out, ref), (what, "thr_mask", _first(out != ref), names)
        ref = np.stack([w["aux"] for w in want])
        out = got["aux"].cpu().numpy()
        assert out.dtype == np.float32 and R.same_f32_bits(out, ref), \
            (what, "aux", _first(out.view(np.int32) != ref.view(np.int32)), names)
    return want


@pytest.mark.parametrize("form,S,dim", R.SCAN_GEOMS)
def test_scan_at_every_geometry(form, S, dim):
    _check_scan(form, S, dim, R.generator_like(form, S, 3, 0))


@pytest.mark.parametrize("form,S,dim", [("wav", 64, 59), ("midi", 35, 32)])
def test_scan_large_batch_and_strided_view(form, S, dim):
    _check_scan(form, S, dim, R.generator_like(form, S, 300, 2))
    m = R.generator_like(form, S, 5, 3)
    want = _check_scan(form, S, dim, m, _strided(m))
    assert not any(w["flag"] for w in want)                           # the NaNs of the gaps raise no flag


@pytest.mark.parametrize("form,S,dim", [("midi", 64, 61), ("wav", 64, 59)])
def test_scan_value_edges(form, S, dim):
    """-0.0 and denormals in the zero mask, the threshold and its float32 neighbours, int(x * 126) at its rounding
    boundaries and the % 128 wrap, 1.7e7 (equal to the oracle) and 1.8e7 (flagged), Python's sequential sum() in the
    aux rows, 0/0 -> NaN, and NaN / +inf / -inf flagged in the sample that holds them and in no other."""
    m, names = R.scan_edge_batch(form, S, dim)
    want = _check_scan(form, S, dim, m, names=names)
    assert [w["flag"] for w in want] == [int(n not in ("edges", "zero_aux", "clean")) for n in names]
    edges = want[names.index("edges")]
    assert edges["zero_mask"][0] & 0b1111 == 0b0010                   # -0.0 is zero, 1e-40 and the denormal are not
    assert 2142000000 in edges["instruments"] and (2142000000 in edges["note_levels"]) == (form == "wav")
    if form == "wav":
        assert np.isnan(want[names.index("zero_aux")]["aux"][0]).all()


# ---- B: gdm_des_routing ----------------------------------------------------------------------------------------------
def _check_routing(dim, S, m, src, cols, g=None):
    got = ops.des_routing(_up(m) if g is None else g, S, dim, _up(src.astype(np.uint8)), _up(cols.astype(np.int32)))
    out = got.cpu().numpy()
    want = np.stack([R.routing_ref(m[k], S, dim, src[k], cols[k]) for k in range(len(m))])
    assert out.dtype == np.float64 and out.shape == want.shape
    bad = out.view(np.int64) != want.view(np.int64)
    assert not bad.any(), ((dim, S, len(m)), int(bad.sum()), _first(bad))
    return want


@pytest.mark.parametrize("dim,S", R.ROUTING_GEOMS)
def test_routing_at_every_geometry(dim, S):
    m, src, cols = R.routing_batch(dim, S, 4)
    want = _check_routing(dim, S, m, src, cols)
    z, c = 2 % dim, (2 % dim + 1) % dim                               # the all-zero row of sample 1
    row = np.zeros(dim)
    row[c] = 1.0
    row[z] = 1.0 if src[1, z] else -1.0
    assert np.array_equal(want[1, z], row)


@pytest.mark.parametrize("dim,S", [(61, 64), (64, 64), (7, 10)])
def test_routing_batch_sizes_and_strided_view(dim, S):
    _check_routing(dim, S, *R.routing_batch(dim, S, 1, seed=1))
    _check_routing(dim, S, *R.routing_batch(dim, S, 300, seed=2))
    m, src, cols = R.routing_batch(dim, S, 5, seed=3)
    _check_routing(dim, S, m, src, cols, _strided(m))


# ---- C: through the package ------------------------------------------------------------------------------------------
def _midi_both(S, g1, g2, **kw):
    np.random.seed(40 + S)
    want = odp.midi_prologue(g1, g2, **kw)
    pos = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(40 + S)
    got = msp.midi_prologue(_up(g1), _up(g2), **kw)
    assert np.random.randint(0, 2 ** 31 - 1) == pos, "global RNG stream position"
    assert len(got) == len(want)
    for i, (s_, w) in enumerate(zip(got, want)):
        _same(s_, w, ("midi", S, i))


@pytest.mark.parametrize("S", R.MIDI_SIZES)
def test_midi_prologue_equals_the_oracle_at_every_size(S):
    g1, g2 = R.generator_like("midi", S, 4, 0)[:, None], R.gen2_like(4, S)
    if S in R.MIDI_RAISES:
        for fn, up in ((odp.midi_prologue, np.asarray), (msp.midi_prologue, _up)):
            np.random.seed(40 + S)
            with pytest.raises(ValueError):
                fn(up(g1), up(g2), adj_size=(S, S))
        return
    _midi_both(S, g1, g2, adj_size=(S, S))


def test_midi_prologue_default_adj_size():
    _midi_both(32, R.generator_like("midi", 32, 3, 5)[:, None], R.gen2_like(3, 5))       # no adj_size: (32, 32)


@pytest.mark.parametrize("S", R.WAV_SIZES)
def test_wav_prologue_equals_the_oracle_at_every_size(S):
    m = R.generator_like("wav", S, 4, 0)
    if S in R.WAV_RAISES:
        for fn, up in ((odp.wav_prologue, np.asarray), (msp.wav_prologue, _up)):
            np.random.seed(40 + S)
            with pytest.raises(ValueError):
                fn(up(m), size=S)
        return
    np.random.seed(40 + S)
    want = odp.wav_prologue(m, size=S)
    pos = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(40 + S)
    got = msp.wav_prologue(_up(m), size=S)
    assert np.random.randint(0, 2 ** 31 - 1) == pos, "global RNG stream position"
    assert len(got) == len(want)
    for i, (s_, w) in enumerate(zip(got, want)):
        _same(s_, w, ("wav", S, i))


def test_the_integer_limit_through_the_package():
    """|m| = 1.7e7 in an instrument and a note-level entry: the oracle's integers.  1.8e7: upstream carries the Python
    big integer 2268000000 on, the package refuses the batch like a non-finite one."""
    g1, g2 = R.generator_like("midi", 12, 3, 7)[:, None], R.gen2_like(3, 7)
    g1[1, 0, 10, 3], g1[2, 0, 11, 8] = 1.7e7, -1.7e7
    _midi_both(12, g1, g2, adj_size=(12, 12))
    m = R.generator_like("wav", 13, 3, 7)
    m[1, 9, 3], m[2, 10, 7] = -1.7e7, 1.7e7
    np.random.seed(3)
    want = odp.wav_prologue(m, size=13)
    np.random.seed(3)
    for i, (s_, w) in enumerate(zip(msp.wav_prologue(_up(m), size=13), want)):
        _same(s_, w, ("wav", 13, i))
    assert want[2]["note_levels"][7] == 2142000000.0
    for row in (10, 11):
        big = g1.copy()
        big[1, 0, row, 3] = 1.8e7
        with pytest.raises(ValueError, match="int32"):
            msp.midi_prologue(_up(big), _up(g2), adj_size=(12, 12))
    for row in (9, 10):
        big = m.copy()
        big[2, row, 0] = -1.8e7
        with pytest.raises(ValueError, match="int32"):
            msp.wav_prologue(_up(big), size=13)
    np.random.seed(3)
    assert odp.wav_prologue(big, size=13)[2]["note_levels"][0] == 2268000000.0


@pytest.mark.parametrize("form,S", [("midi", 5), ("midi", 12), ("midi", 32), ("wav", 8), ("wav", 13)])
def test_device_prologue_equals_numpy_per_sample(form, S):
    b = 4
    base = np.array([3, 2 ** 32 - 1, 77, 12345], dtype=np.uint32)
    m = R.generator_like(form, S, b, 4)
    state = np.random.get_state()
    if form == "midi":
        g1, g2 = _up(m[:, None]), _up(R.gen2_like(b, S))
        dev = msp.device_prologue_midi(g1, g2, (S, S), None, base=base)
        want = _numpy_prologue(msp.MIDI, msp.MIDI.scan(g1, S, g2), None, base)
    else:
        dev = msp.device_prologue_wav(_up(m), S, None, base=base)
        want = _numpy_prologue(msp.WAV, msp.WAV.scan(_up(m), S), None, base)
    assert np.array_equal(np.random.get_state()[1], state[1])         # a given base: the global stream is not touched
    assert not dev.status.any() and not dev.flags.any()
    assert torch.equal(dev.routing.view(torch.int64), want.routing.view(torch.int64))
    for name in ("loc", "scale", "queue_cap", "seed", "customers", "instruments", "note_levels"):
        assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(want, name)), name
    key, pos, _has, _gauss = sv.pack_states(want.states, b)
    assert np.array_equal(dev.mt_key.cpu().numpy().view(np.uint32), key) and np.array_equal(dev.mt_pos.cpu().numpy(), pos)
    # the routing matrices once more, against the reference that does not go through ops.des_routing
    src, cols = dev.src.cpu().numpy().astype(bool), dev.cols.cpu().numpy()
    dim = S - (3 if form == "midi" else 5)
    ref = np.stack([R.routing_ref(m[k], S, dim, src[k], cols[k]) for k in range(b)])
    assert np.array_equal(dev.routing.cpu().numpy().view(np.int64), ref.view(np.int64))


# ---- D: gdm_des_pack -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,cap,pattern", R.PACK_CASES)
def test_pack_equals_the_reference(b, cap, pattern):
    n, arrays = R.pack_case(b, cap, pattern)
    want_ptr, want = R.pack_ref(n, arrays, cap)
    dev = [_up(a) for a in arrays]
    rec_ptr = torch.full((b + 1,), -7, dtype=torch.int64, device=DEV)
    ops.des_pack(_up(n), rec_ptr, *dev, cap)
    assert np.array_equal(rec_ptr.cpu().numpy(), want_ptr), (b, cap, pattern)
    total = int(want_ptr[-1])
    for name, t, w in zip(("value", "event_id", "node", "kind"), dev, want):
        out = t.cpu().numpy()[:total]
        assert out.dtype == w.dtype and out.tobytes() == w.tobytes(), (b, cap, pattern, name, _first(out != w))
