"""CPU: tests/mel_ref.py checked before it is used, and the featuriser's host-built constants.

The reference rounded to fp32 passes its own checker on every case of the GPU tables (tests/test_mel_stages_gpu.py)
with no case left out, every planted fault is rejected by at least one of those cases, the frame reference is
torch.stft's own framing, the dB reference is torch's clamp / amax / maximum, and an fp32 evaluation on the CPU of each
stage and of the whole chain stays inside the derived bounds (so the bounds do not ask the impossible).  The fp32 DFT
matrix and the padded mel matrix of gan_des_midi_music_gen_amd.util are held to independent float64 evaluations."""
import math

import numpy as np
import pytest
import torch

import mel_ref as mr
from gan_des_midi_music_gen_amd import util
from oracle import mel as om


def _f32(bits):
    return torch.from_numpy(np.array(bits, copy=True)).view(torch.float32)


# ------------------------------------------------------------------------------------------------- frames
def test_frame_reference_is_torch_stfts_framing():
    """torch.stft with a window of ones and all n_fft bins is the DFT of each frame: its inverse is the frame"""
    c = mr.FrameCase("stft", 64, 16, 70)
    x = torch.randn(c.L, generator=torch.Generator().manual_seed(1))
    spec = torch.stft(x.double(), n_fft=c.n_fft, hop_length=c.hop, win_length=c.n_fft,
                      window=torch.ones(c.n_fft, dtype=torch.float64), center=True, pad_mode="reflect",
                      normalized=False, onesided=False, return_complex=True)
    want = torch.fft.ifft(spec, dim=0).real.t()
    got = _f32(mr.frames_ref(c, x.numpy().view(np.int32)[None, :])).double()
    assert got.shape == want.shape == (c.frames, c.n_fft)
    assert float((got - want).abs().max()) < 1e-12


def test_frame_tables_reach_what_they_name():
    by = {c.name: c for c in mr.FRAME_CASES}
    assert mr.trips(by["second grid trip"].total4) == 2
    assert all(mr.trips(c.total4) == 1 for c in mr.FRAME_CASES if c.name != "second grid trip")
    assert any(c.L == c.n_fft // 2 + 1 for c in mr.FRAME_CASES)                     # the minimum length
    assert any(c.hop == 1 for c in mr.FRAME_CASES) and any(c.hop > c.n_fft for c in mr.FRAME_CASES)
    assert any(c.n_fft == 4 for c in mr.FRAME_CASES)
    assert any(c.L % c.hop == 0 and c.B > 1 and c.extra for c in mr.FRAME_CASES)
    both = by["minimum L, both sides reflected in one frame"]
    assert both.hop < both.n_fft // 2 and both.hop + both.n_fft // 2 > both.L      # frame 1 leaves both ends
    for c in mr.FRAME_CASES:
        bits = mr.frame_input(c)
        nan = (bits & 0x7fffffff) > 0x7f800000
        if c.L >= 33:                                                               # payload NaNs and -0 inside
            assert nan[:, :c.L].any() and (bits[:, :c.L] == np.int32(-2 ** 31)).any()
        assert len(set(bits[0, [0, c.L - 1]].tolist()) & set(mr._FRAME_SPECIALS.tolist())) == 2   # at both ends
        assert (bits[:, c.L:] == mr.TRAILING_NAN).all() and not (bits[:, :c.L] == mr.TRAILING_NAN).any()


def test_frame_checker_passes_the_reference_and_rejects_every_fault():
    caught = {f: [] for f in mr.FRAME_FAULTS}
    for c in mr.FRAME_CASES:
        bits = mr.frame_input(c)
        clean = mr.frames_ref(c, bits)
        assert mr.check_frames(_f32(clean), clean, what=c.name) == []              # through an fp32 tensor: bits kept
        for f in mr.FRAME_FAULTS:
            if mr.check_frames(_f32(mr.frames_ref(c, bits, faults=(f,))), clean, what=f):
                caught[f].append(c.name)
    assert all(caught.values()), {f: v for f, v in caught.items() if not v}
    assert caught["stride_ignored"] and all("strided" in n for n in caught["stride_ignored"])
    assert caught["second_trip_dropped"] == ["second grid trip"]
    # the right edge is judged by several geometries, the centred last frame among them
    assert "last frame centred on L" in caught["symmetric_right"] and len(caught["reflect_about_L"]) >= 6


# -------------------------------------------------------------------------------------------------- power
ALL_POWER = mr.POWER_CASES + [mr.POWER_SECOND_TRIP]


def test_power_tables_reach_what_they_name():
    assert mr.trips(mr.POWER_SECOND_TRIP.rows * mr.POWER_SECOND_TRIP.ldp) == 2 and mr.POWER_SECOND_TRIP.ldp == 1024
    assert all(mr.trips(c.rows * c.ldp) == 1 for c in mr.POWER_CASES)
    seen = torch.cat([mr.power_input(c).reshape(-1) for c in mr.POWER_CASES if c.rows * c.nfreq <= 15])
    assert bool(torch.isnan(seen).any()) and bool((seen == 2e19).any()) and bool((seen.abs() == 1e19).any())
    assert bool(((seen != 0) & (seen.abs() < 2.0 ** -126)).any()) and bool((seen == 0).any())
    assert math.isinf(float(torch.tensor(2e19) ** 2)) and math.isfinite(float(torch.tensor(1e19) ** 2))


def test_power_checker_passes_the_reference_and_rejects_every_fault():
    caught = {f: [] for f in mr.POWER_FAULTS}
    for c in ALL_POWER:
        x = mr.power_input(c)
        exp = mr.power_expected(c, x)
        fails, _ = mr.check_power(exp["out"].float(), c, exp, what=c.name)
        assert fails == [], fails
        own = torch.zeros(c.rows, c.ldp)                                  # the operation in fp32 on the CPU
        own[:, :c.nfreq] = x[:, :c.nfreq] * x[:, :c.nfreq] + x[:, c.nfreq:] * x[:, c.nfreq:]
        fails, _ = mr.check_power(own, c, exp, what=c.name)
        assert fails == [], fails
        for f in mr.POWER_FAULTS:
            if mr.check_power(mr.power_expected(c, x, faults=(f,))["out"].float(), c, exp, what=f)[0]:
                caught[f].append(c.name)
    assert all(caught.values()), {f: v for f, v in caught.items() if not v}
    assert caught["second_trip_dropped"] == [mr.POWER_SECOND_TRIP.name]
    assert len(caught["pads_unwritten"]) == sum(c.pad > 0 for c in ALL_POWER)
    neg_zero = torch.full((1, 6), -0.0)
    c = mr.PowerCase(1, 5, 1)
    exp = mr.power_expected(c, torch.zeros(1, 10))
    assert mr.check_power(neg_zero, c, exp)[0] and not mr.check_power(torch.zeros(1, 6), c, exp)[0]   # +0, not -0


# ----------------------------------------------------------------------------------------------------- dB
ALL_DB = mr.DB_CASES + mr.DB_MANY_WINDOWS + mr.DB_LDS_FITS + mr.DB_NONFINITE


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_db_tables_reach_what_they_name():
    ns = {c.n for c in ALL_DB}
    assert any(n < mr.DB_BLOCK for n in ns) and any(n > mr.DB_BLOCK and n % mr.DB_BLOCK for n in ns)
    assert 216 * 128 in ns and (216 * 128) % mr.DB_BLOCK == 0                 # the one shape the suite had
    assert any(math.gcd(c.frames, c.n_mels) == 1 and c.frames > c.n_mels > 1 for c in ALL_DB)
    assert any(math.gcd(c.frames, c.n_mels) == 1 and 1 < c.frames < c.n_mels for c in ALL_DB)
    f, k = mr.DB_LDS_REFUSED
    assert k * (f + 1) > mr.LDS_FLOATS == mr.DB_LDS_FITS[0].n_mels * (mr.DB_LDS_FITS[0].frames + 1)
    for c in ALL_DB:
        p = mr.db_input(c).reshape(c.B, c.n)
        if c.kind == "finite" and c.top_db is not None:
            assert int(p[0].argmax()) == c.n - 1                              # window 0: the maximum is the last element
        if c.n >= 7:
            flat = p.reshape(-1)
            a = np.float32(mr.AMIN)
            for v in (0.0, float(a), float(np.nextafter(a, np.float32(0))), float(np.nextafter(a, np.float32(1))), 1.0):
                assert bool((flat == v).any()), (c.name, v)
        if c.B == 3:
            assert bool((p[2] == 3.0e38).any()) == (c.n > 6)
        if c.kind != "finite":
            bad = ~torch.isfinite(p)
            assert int(bad.sum()) == 1 and bool(bad[1].any())


def test_db_reference_is_torchs_clamp_amax_maximum():
    for c in ALL_DB:
        exp = mr.db_expected(mr.db_input(c), c.B, c.frames, c.n_mels, c.top_db)
        assert _same(exp["out"], mr.db_torch(mr.db_input(c), c.B, c.frames, c.n_mels, c.top_db)), c.name
        if c.kind == "inf":
            w = exp["out"][1]
            assert bool(torch.isinf(w).all()) if c.top_db is not None else int(torch.isinf(w).sum()) == 1
        if c.kind == "nan":
            w = exp["out"][1]
            assert bool(torch.isnan(w).all()) if c.top_db is not None else int(torch.isnan(w).sum()) == 1
        if c.kind != "finite":
            assert bool(torch.isfinite(exp["out"][0]).all()) and bool(torch.isfinite(exp["out"][2]).all())


def test_db_checker_passes_the_reference_and_rejects_every_fault():
    caught = {f: [] for f in mr.DB_FAULTS}
    for c in ALL_DB:
        p = mr.db_input(c)
        exp = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db)
        fails, _ = mr.check_values(exp["out"].float(), exp["out"], exp["E"], what=c.name)
        assert fails == [], fails
        own = 10.0 * torch.log10(torch.clamp(p.reshape(c.B, c.frames, c.n_mels), min=mr.AMIN))       # fp32 on the CPU
        if c.top_db is not None:
            own = torch.maximum(own, own.amax((1, 2), keepdim=True) - c.top_db)
        fails, worst = mr.check_values(own.transpose(1, 2), exp["out"], exp["E"], what=c.name)
        assert fails == [], fails
        for f in mr.DB_FAULTS:
            wrong = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db, faults=(f,))["out"].float()
            if mr.check_values(wrong, exp["out"], exp["E"], what=f)[0]:
                caught[f].append(c.name)
    assert all(caught.values()), {f: v for f, v in caught.items() if not v}
    assert all("top_db=None" in n for n in caught["none_as_zero"])
    assert all("nan" in n for n in caught["nan_swallowed"]) and len(caught["nan_swallowed"]) == 6
    assert any("top_db=80" in n for n in caught["ragged_tail_dropped"])      # through the floor: the dropped maximum
    assert any("B=3" in n or "B=300" in n for n in caught["floor_window0"])


def test_a_floor_from_another_window_is_far_outside_the_bound():
    c = mr.DbCase(5, 3, 300, 80)
    p = mr.db_input(c)
    exp = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db)
    wrong = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db, faults=("floor_batch_max",))["out"]
    floored = exp["out"] > mr.db_torch(p, c.B, c.frames, c.n_mels, None)
    assert bool(floored.any())
    ratio = ((wrong - exp["out"]).abs() / exp["E"])[floored]
    assert float(ratio.max()) > 1e4


# ----------------------------------------------------------------------------------------- host constants
@pytest.mark.parametrize("n", [4, 8, 64, 2048])
def test_dft_matrix_is_the_periodic_hann_times_cos_and_sin(n):
    m = util._dft_matrix(n, "cpu")
    assert m.shape == (n, 2 * (n // 2 + 1)) and m.dtype == torch.float32 and m.is_contiguous()
    assert mr.check_dft_matrix(m, n, what=f"n_fft {n}") == []
    wrong = torch.from_numpy(mr.dft_matrix_ref(n, symmetric=True)).float()
    assert mr.check_dft_matrix(wrong, n, what="symmetric Hann")


def test_dft_matrix_reference_is_the_dft():
    """[cos | sin] of the reference without its window against numpy's FFT of the identity"""
    n = 64
    eye = np.fft.rfft(np.eye(n), axis=1)
    win = torch.hann_window(n, periodic=True, dtype=torch.float64).numpy()[:, None]
    want = np.concatenate([eye.real, -eye.imag], axis=1) * win
    np.testing.assert_allclose(mr.dft_matrix_ref(n), want, atol=1e-14)


MEL_GEOMETRIES = [c.mel_args() for c in mr.CHAIN_CASES]


@pytest.mark.parametrize("n_fft,sr,n_mels,fmin,fmax,ldp", MEL_GEOMETRIES, ids=[c.name for c in mr.CHAIN_CASES])
def test_mel_matrix_is_the_published_filter_bank_rounded_once(n_fft, sr, n_mels, fmin, fmax, ldp):
    nfreq = n_fft // 2 + 1
    m = util._mel_matrix(n_fft, sr, n_mels, fmin, fmax, ldp, "cpu")
    assert m.shape == (ldp, n_mels) and m.dtype == torch.float32 and m.is_contiguous()
    assert ldp % 4 == 0 and 0 <= ldp - nfreq < 4
    want = om.melscale_fbanks(nfreq, float(fmin), float(fmax), n_mels, sr)
    assert np.array_equal(m[:nfreq].numpy(), want.astype(np.float32))
    assert not bool(m[nfreq:].any()) and not bool(torch.signbit(m[nfreq:]).any())        # the pad rows: exactly +0
    assert bool((want.max(0) > 0).all()), "an empty filter: choose sr / fmin / fmax so that every triangle holds a bin"
    try:
        from transformers import audio_utils as au
    except ImportError:
        return
    pub = au.mel_filter_bank(num_frequency_bins=nfreq, num_mel_filters=n_mels, min_frequency=float(fmin),
                             max_frequency=float(fmax), sampling_rate=sr, norm=None, mel_scale="htk")
    assert np.array_equal(m[:nfreq].numpy(), pub.astype(np.float32))


# -------------------------------------------------------------------------------------------------- chain
def _chain_fp32(c, dft, mel_m):
    """the chain in fp32 on the CPU -> (mel power, dB)"""
    bits = c_bits(c)
    frames = _f32(mr.frames_ref(mr.FrameCase(c.name, c.n_fft, c.hop, c.L, c.B), bits))
    spec = frames @ dft
    p = torch.zeros(frames.shape[0], c.ldp)
    p[:, :c.nfreq] = spec[:, :c.nfreq] ** 2 + spec[:, c.nfreq:] ** 2
    mel = p @ mel_m
    d = 10.0 * torch.log10(torch.clamp(mel.reshape(c.B, c.frames, c.n_mels), min=mr.AMIN))
    d = torch.maximum(d, d.amax((1, 2), keepdim=True) - c.top_db)
    return frames, mel, d.transpose(1, 2)


def c_bits(c):
    return mr.chain_input(c).numpy().view(np.int32)


@pytest.mark.parametrize("c", mr.CHAIN_CASES[:3], ids=[c.name for c in mr.CHAIN_CASES[:3]])
def test_chain_bounds_hold_an_fp32_evaluation_and_reject_wrong_constants(c):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dft, mel_m = util._dft_matrix(c.n_fft, "cpu"), util._mel_matrix(*c.mel_args(), "cpu")
    frames, mel, d = _chain_fp32(c, dft, mel_m)
    exp = mr.chain_expected(c, frames, dft, mel_m, 1, 1)
    for got, (ref, E), what in ((mel, exp["mel"], "mel power"), (d, (exp["db"]["out"], exp["db"]["E"]), "dB")):
        fails, worst = mr.check_values(got, ref, E, what=f"{c.name} {what}")
        assert fails == [] and worst < 1.0, fails
    silent = exp["db"]["out"][3]
    assert bool((silent == 10.0 * math.log10(mr.AMIN)).all())                       # the silent window: the clamp
    at_max = exp["db"]["out"] == exp["db"]["out"].amax((1, 2), keepdim=True)
    assert float(exp["db"]["E"][at_max].max()) < 0.02          # at the window maxima: tighter than tests/test_mel.py
    # wrong constants: a symmetric Hann window; the filter bank one bin off (what a wrong ldp hand-off would do)
    sym = torch.from_numpy(mr.dft_matrix_ref(c.n_fft, symmetric=True)).float()
    shifted = torch.roll(mel_m, 1, 0)
    for name, (dd, mm) in (("symmetric Hann", (sym, mel_m)), ("filter bank shifted", (dft, shifted))):
        _, mel_w, d_w = _chain_fp32(c, dd, mm)
        assert mr.check_values(mel_w, *exp["mel"], what=name)[0], name
        assert mr.check_values(d_w, exp["db"]["out"], exp["db"]["E"], what=name)[0], name


def test_chain_inputs_are_what_the_table_says():
    for c in mr.CHAIN_CASES:
        x = mr.chain_input(c)
        assert x.shape == (c.B, c.L) and c.L > c.n_fft // 2 and c.ldp >= c.nfreq
        assert not bool(x[3].any()) and float(x[2, 0]) != 0 and float(x[2, -1]) != 0
        assert int((x[2] != 0).sum()) == 2 and bool((x[1] == x[1].round()).all())
        levels = [float(x[w].abs().max()) for w in range(c.B) if w != 3]
        assert len(set(levels)) == len(levels)
