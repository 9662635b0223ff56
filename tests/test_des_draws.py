"""CPU: ``gdm_des_draws_host`` -- the source the "des_device" kernel is compiled from -- against numpy itself.

For every sample the expected values come from ``np.random.seed(int(base[i]))`` followed by the calls the bridges make
today (``_midi_draws`` / ``_wav_draws``, ``_midi_spec`` / ``_wav_spec``) on the same scan dictionary; everything is
compared bit for bit, the final stream included.  Where numpy raises, the status code and the defined values of a
refused sample are checked instead."""
import numpy as np
import pytest

from gan_des_midi_music_gen_amd import matrix_sim_process as msp
from gan_des_midi_music_gen_amd import ops

EDGE_SEEDS = (0, 2 ** 32 - 1)
P6 = (-1.0, 0.01, 0.2, 0.9, 5.0)          # 3000 * p6 = -3000, 30, 600 (-> 1000), 2700, 15000 (-> themselves)


def _bases(rng, b):
    base = rng.integers(0, 2 ** 32, size=b, dtype=np.uint64).astype(np.uint32)
    base[:2] = EDGE_SEEDS[:b] if b < 2 else EDGE_SEEDS
    return base


def _words_of(zero):
    b, dim, _ = zero.shape
    words = np.zeros((b, dim), dtype=np.uint64)
    for x in range(dim):
        words |= zero[:, :, x].astype(np.uint64) << np.uint64(x)
    return words.view(np.int64)


def _fresh_state(seed):
    return np.random.RandomState(int(seed)).get_state()


def _expect(draws, h, i, base):
    """numpy's answer for sample i: (src, cols, seed, state) or the exception it raises."""
    np.random.seed(int(base[i]))
    try:
        src, cols, sd = draws(h, i)
    except (ValueError, IndexError) as e:
        return e
    return src, cols, int(np.asarray(sd).reshape(-1)[0]), np.random.get_state()


def _compare(out, i, exp, base, status_of):
    if isinstance(exp, Exception):
        want_status, want_type = status_of(exp)
        assert out["status"][i] == want_status, (i, out["status"][i], exp)
        assert isinstance(msp.draws_error(want_status), want_type)
        assert not out["src"][i].any() and not out["cols"][i].any() and out["seed"][i] == 0
        state = _fresh_state(base[i])
        assert (out["scale"][i] == -1.0).all()            # what makes the simulator skip the sample
    else:
        src, cols, sd, state = exp
        assert out["status"][i] == 0, (i, out["status"][i])
        assert np.array_equal(out["src"][i].astype(bool), src)
        assert np.array_equal(out["cols"][i], cols)
        assert out["seed"][i] == sd
    assert np.array_equal(out["mt_key"][i], state[1]) and out["mt_pos"][i] == state[2]
    assert out["has_gauss"][i] == state[3] == 0 and out["gauss"][i] == 0.0
    assert (out["queue_cap"][i] == 254).all()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def _compare_spec(out, i, spec, customers):
    assert _same_bits(out["loc"][i], [float(d[1]) for d in spec.distributions])
    assert _same_bits(out["scale"][i], [float(d[2]) for d in spec.distributions])
    assert out["customers"][i] == customers
    assert np.array_equal(out["instruments"][i], [int(x) for x in spec.instruments])
    assert np.array_equal(out["note_levels"][i], [int(x) for x in spec.note_levels])


def _midi_status(e):
    assert isinstance(e, ValueError), e
    return 1, ValueError


def _run_midi(h, base, instrument):
    b, dim = h["b"], h["dim"]
    out = msp.des_draws_host(ops.DES_DRAWS_MIDI, h["size"], dim, base, h["zmask"], h["inst"], h["notes"], h["g2"],
                             instrument_override=msp._instrument_override(instrument, b))
    n_ok = 0
    for i in range(b):
        exp = _expect(msp._midi_draws, h, i, base)
        _compare(out, i, exp, base, _midi_status)
        if not isinstance(exp, Exception):
            spec = msp._midi_spec(h, i, None, exp[0], np.array([exp[2]]), instrument)
            _compare_spec(out, i, spec, spec.num_customers)
            n_ok += 1
    return out, n_ok


def _midi_h(rng, b, dim, zero):
    g2 = rng.standard_normal((b, 16)).astype(np.float32)
    g2[:, 6] = [P6[i % len(P6)] for i in range(b)]
    return {"size": dim + 3, "dim": dim, "b": b, "g2": g2, "zmask": _words_of(zero),
            "inst": rng.integers(0, 127, size=(b, dim)).astype(np.int32),
            "notes": rng.integers(0, 128, size=(b, dim)).astype(np.int32)}


@pytest.mark.parametrize("density", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("dim", [1, 2, 4, 5, 15, 29, 61])
def test_midi_route_equals_numpy(dim, density):
    rng = np.random.default_rng(1000 * dim + int(10 * density))
    b = 7
    zero = rng.random((b, dim, dim)) < density
    h = _midi_h(rng, b, dim, zero)
    h["zmask"] = h["zmask"] | np.int64(-1 << dim if dim < 63 else 0)          # junk above dim must be ignored
    base = _bases(rng, b)
    instrument = [None, 7, [None if i % 2 else i + 1 for i in range(b)]][dim % 3]
    out, n_ok = _run_midi(h, base, instrument)
    if dim == 1:
        assert n_ok == 0 and (out["status"] == 1).all()      # no other column: np.random.choice([]) raises
    if dim >= 2 and density == 0.0:
        assert n_ok == b
    customers = {int(c) for c in out["customers"][out["status"] == 0]}
    if n_ok == b:
        assert min(customers) == 1000 and len(customers) == 3   # every arm of max(200, max(1000, int(3000 * p6)))


@pytest.mark.parametrize("dim", [2, 3, 5, 15])
def test_midi_rows_with_one_and_with_no_candidate(dim):
    """A one-element candidate list consumes no word; an empty one is status 1 (numpy: ValueError)."""
    rng = np.random.default_rng(dim)
    b = 8
    zero = np.zeros((b, dim, dim), dtype=bool)
    zero[:, 0, :] = True
    zero[:, 0, dim - 1] = False                    # row 0: only the last column (a source for some seeds: then empty)
    zero[b - 1, dim - 1, :] = True                 # last sample: a row without any candidate
    h = _midi_h(rng, b, dim, zero)
    base = _bases(rng, b)
    out, n_ok = _run_midi(h, base, None)
    assert out["status"][b - 1] == 1
    assert n_ok >= 1 and (out["cols"][out["status"] == 0][:, 0] == dim - 1).all()
    if dim // 4 == 0:
        assert n_ok == b - 1                       # no sources: row 0 always keeps its one candidate


def _wav_status(e):
    if isinstance(e, IndexError):
        return 3, IndexError
    assert isinstance(e, ValueError), e
    return (2 if "ambiguous" in str(e) else 1), ValueError


@pytest.mark.parametrize("density", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("dim", [3, 4, 5, 15, 29, 59])
def test_wav_route_equals_numpy(dim, density):
    rng = np.random.default_rng(77 * dim + int(10 * density))
    size, b = dim + 5, 8
    zero = rng.random((b, dim, dim)) < density
    thr = np.zeros((b, size), dtype=bool)
    thr[1, rng.integers(0, dim)] = True                      # one thresholded source: no permutation is drawn
    thr[2, 0] = True                                         # two: status 2
    thr[2, size - 1] = True
    thr[3, dim] = True                                       # a column >= dim: status 3
    thr[4, size - 1] = True
    thr[5, dim - 1] = True
    aux = rng.random((b, 2, dim)).astype(np.float32)
    h = {"size": size, "dim": dim, "b": b, "thr": thr, "aux": aux, "zmask": _words_of(zero),
         "inst": rng.integers(0, 127, size=(b, dim)).astype(np.int32),
         "notes": rng.integers(0, 300, size=(b, dim)).astype(np.int32)}
    base = _bases(rng, b)
    same = [None, 11][dim % 2]
    out = msp.des_draws_host(ops.DES_DRAWS_WAV, size, dim, base, h["zmask"], h["inst"], h["notes"], aux, thr_mask=thr,
                             instrument_override=msp._instrument_override(same, b))
    for i in range(b):
        exp = _expect(msp._wav_draws, h, i, base)
        _compare(out, i, exp, base, _wav_status)
        if not isinstance(exp, Exception):
            _compare_spec(out, i, msp._wav_spec(h, i, None, exp[0], np.array([exp[2]]), same), 1000)
    assert out["status"][2] == 2 and out["status"][3] == 3 and out["status"][4] == 3
    if density == 0.0:
        assert list(out["status"]) == [0, 0, 2, 3, 3, 0, 0, 0]
        assert out["src"][1].sum() == 1 and out["src"][0].sum() == size // 8


def test_customers_that_python_cannot_convert():
    rng = np.random.default_rng(5)
    dim, b = 4, 4
    h = _midi_h(rng, b, dim, np.zeros((b, dim, dim), dtype=bool))
    h["g2"][:, 6] = [np.nan, np.inf, -3e38, 0.5]
    base = _bases(rng, b)
    out = msp.des_draws_host(ops.DES_DRAWS_MIDI, dim + 3, dim, base, h["zmask"], h["inst"], h["notes"], h["g2"])
    assert list(out["status"]) == [5, 5, 5, 0]
    for i in range(3):
        with pytest.raises((ValueError, OverflowError)), np.errstate(over="ignore"):
            np.int64(max(200, max(1000, int(3000 * h["g2"][i][6]))))
        assert np.array_equal(out["mt_key"][i], _fresh_state(base[i])[1]) and out["mt_pos"][i] == 624


def test_arguments_are_checked_on_the_host():
    z = np.zeros((1, 4), dtype=np.int64)
    i4 = np.zeros((1, 4), dtype=np.int32)
    with pytest.raises(ops.GdmError):
        msp.des_draws_host(ops.DES_DRAWS_MIDI, 7, 4, [1], z, i4, i4, np.zeros((1, 6), dtype=np.float32))
    with pytest.raises(ops.GdmError):
        msp.des_draws_host(ops.DES_DRAWS_WAV, 9, 4, [1], z, i4, i4, np.zeros((1, 8), dtype=np.float32))   # no thr_mask
    with pytest.raises(ops.GdmError):
        msp.des_draws_host(2, 7, 4, [1], z, i4, i4, np.zeros((1, 16), dtype=np.float32))


def test_base_seeds_are_the_one_call_on_the_global_stream():
    np.random.seed(1234)
    base = msp.draw_base_seeds(5)
    after = np.random.get_state()
    np.random.seed(1234)
    want = np.random.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    ref = np.random.get_state()
    assert base.dtype == np.uint32 and np.array_equal(base, want)
    assert np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]


def test_back_end_names():
    import torch
    for call in (lambda: msp.matrix_to_midi(torch.zeros(1, 1, 8, 8), torch.zeros(1, 16), simulate="des_gpu"),
                 lambda: msp.matrix_to_midis(torch.zeros(1, 1, 8, 8), torch.zeros(1, 16), (8, 8), None, 0, 50,
                                             simulate="des_gpu")):
        with pytest.raises(ops.GdmError, match="des_device"):
            call()
    assert {k: v[0] for k, v in ops.DES_DRAWS_ERRORS.items()}[3] is IndexError
