"""GPU: model 1's file input -- the device PCM front end (gdm_pcm_to_float, gdm_pcm_stft_frames: csrc/mel.hip) against its
numpy mirror (tests/pcm_ref.py), and what is built on it: util.split_audio_data,
util.get_melspectrogram_db_tensor_from_file, datasets.InputSong, SIMNN.train(audio_file=...).

Bar: equal bits (int32 view of the floats) wherever the arithmetic is defined exactly -- the decode and mono rule, the
frame matrix, and everything downstream of it compared with today's path on the decoded windows; the featuriser's own
bounds of tests/test_mel.py (0.02 dB within 60 dB of the window maximum, 0.5 dB elsewhere) against oracle/mel.py.  Every
kernel output is written between two 64-element guards that must come back untouched.
PARITY: S16 is pinned (exact arithmetic; the reference's own three files); U8 / S24 / S32 / F32 are checked against the
formula torchaudio documents, which is all there is to check them against here.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pcm_ref as P  # noqa: E402

from oracle import mel as om  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

WAV_DIR = os.path.join(HERE, "golden", "wav")
FIXTURES = ["simulation.wav", "generation_first5s.wav", "output_0_first5s.wav"]
GUARD = 64
GUARD_VALUE = -7777.25
FORMATS = [P.U8, P.S16, P.S24, P.S32, P.F32]
NAMES = {P.U8: "u8", P.S16: "s16", P.S24: "s24", P.S32: "s32", P.F32: "f32"}


def _guarded(shape):
    """(whole buffer, view of `shape` between two guards); the view starts 256 bytes in: 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu().numpy()
    return bool((g == np.float32(GUARD_VALUE)).all())


def _upload(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _planted(fmt, n, channels, seed):
    """(n, channels) sample values of a format: seeded noise over the full range with the format's extremes planted."""
    g = np.random.default_rng(seed)
    if fmt == P.F32:
        v = (g.standard_normal((n, channels)) * 0.5).astype(np.float32)
        edge = np.float32([-0.0, 0.0, 1e-41, -1e-40, 1.1754942e-38, 3.5, -17.25, 1e30, -1e30, 1.0, -1.0])
    else:
        bits = P.BYTES[fmt] * 8
        lo, hi = (0, 255) if fmt == P.U8 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        v = g.integers(lo, hi + 1, size=(n, channels))
        edge = [lo, hi, lo + 1, hi - 1, 0, 1, -1 if lo < 0 else 128]
        if fmt == P.S32:                                            # odd low bits: the int -> fp32 rounding is visible
            edge += [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, -(1 << 24) - 3, (1 << 30) + 65, 0x7FFFFFBF, 0x7FFFFFC0,
                     -0x7FFFFFBF, 0x12345679]
        edge = np.asarray(edge)
    k = len(edge)
    for c in range(channels):                                       # every edge in every channel, shifted so that the
        v[c:c + k, c] = edge                                        # mean meets min + max, min + min, ...
    v[n - k:, 0] = edge[::-1]
    return v


# ---- ops.pcm_to_float ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_pcm_to_float_bits(fmt, channels):
    from gan_des_midi_music_gen_amd import ops
    n = 257
    raw = P.encode(_planted(fmt, n, channels, seed=fmt * 10 + channels), fmt)
    x = P.decode(raw, fmt, channels)
    pcm = _upload(raw)
    for mix in sorted({-1, 0, channels - 1}):
        want = P.mono(x, mix)
        for first in (0, 1, 3):
            for count in (1, 254):
                buf, out = _guarded((count,))
                got = ops.pcm_to_float(pcm, fmt, channels, mix, n, first, count, out=out)
                assert got is out
                P.check_bits(out.cpu().numpy(), want[first:first + count], f"mix={mix} first={first} count={count}")
                assert _guards_intact(buf), (mix, first, count)
        # the default: the whole signal into a fresh tensor
        P.check_bits(ops.pcm_to_float(pcm, fmt, channels, mix, n).cpu().numpy(), want, f"mix={mix} whole")


def test_pcm_to_float_refuses():
    from gan_des_midi_music_gen_amd import ops
    raw = P.encode(np.arange(64).reshape(32, 2), P.S16)
    pcm = _upload(raw)
    for kw in (dict(first=30, count=3), dict(fmt=7), dict(channels=9), dict(n=33), dict(mix=2), dict(first=-1, count=2)):
        a = dict(fmt=P.S16, channels=2, mix=0, n=32, first=0, count=4)
        a.update(kw)
        buf, out = _guarded((a["count"],))
        with pytest.raises(ops.GdmError):
            ops.pcm_to_float(pcm, a["fmt"], a["channels"], a["mix"], a["n"], a["first"], a["count"], out=out)
        assert bool((buf.cpu() == GUARD_VALUE).all()), kw               # refused on the host: nothing was launched


# ---- ops.pcm_stft_frames -------------------------------------------------------------------------------------------------
N_SONG = 211


def _song(fmt, channels, seed=3):
    """N_SONG sample frames of distinct values (over all channels), spread over the format's whole range."""
    g = np.random.default_rng(seed + 7 * fmt + channels)
    shape = (N_SONG, channels)
    if fmt == P.U8:
        return np.stack([g.permutation(256)[:N_SONG] for _ in range(channels)], axis=1)     # distinct per channel
    top = g.permutation(65536)[:N_SONG * channels].reshape(shape) - 32768                   # distinct upper 16 bits
    if fmt == P.F32:
        return (top / 16384.0).astype(np.float32)
    low_bits = P.BYTES[fmt] * 8 - 16
    return top * (1 << low_bits) + g.integers(0, 1 << low_bits, size=shape)


def _frames_case(ops, pcm, x, fmt, channels, mix, start0, stride, n_regular, tail_start, win_len, hop, n_fft):
    want, frames = P.frames_matrix(P.mono(x, mix), P.starts_of(start0, stride, n_regular, tail_start), win_len, hop, n_fft)
    buf, out = _guarded(want.shape)
    got, got_frames = ops.pcm_stft_frames(pcm, fmt, channels, mix, N_SONG, start0, stride, n_regular, tail_start, win_len,
                                          hop, n_fft, out=out)
    what = f"start0={start0} stride={stride} n_regular={n_regular} tail={tail_start} win={win_len} hop={hop} n_fft={n_fft}"
    assert got is out and got_frames == frames, what
    P.check_bits(out.cpu().numpy(), want, what)
    assert _guards_intact(buf), what


@pytest.mark.parametrize("n_fft", [8, 16])
@pytest.mark.parametrize("fmt,channels,mix", [(P.S16, 2, -1), (P.S16, 2, 1), (P.S24, 1, 0)],
                         ids=["s16-stereo-mean", "s16-stereo-right", "s24-mono"])
def test_pcm_stft_frames_bits_over_the_window_grid(fmt, channels, mix, n_fft):
    from gan_des_midi_music_gen_amd import ops
    raw = P.encode(_song(fmt, channels), fmt)
    x = P.decode(raw, fmt, channels)
    pcm = _upload(raw)
    cases = 0
    for hop in (1, 3, 5):
        for win_len in (n_fft // 2 + 1, 13, 37):                      # the first: both reflections within one frame
            for start0 in (0, 3):
                for stride in (5, win_len, win_len + 2):              # overlapping, abutting, with gaps
                    for n_regular in (1, 4):
                        for tail_start in (-1, N_SONG - win_len):     # absent, or ending exactly at the last sample
                            _frames_case(ops, pcm, x, fmt, channels, mix, start0, stride, n_regular, tail_start, win_len,
                                         hop, n_fft)
                            cases += 1
    assert cases == 216


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_pcm_stft_frames_bits_in_every_format(fmt, channels):
    from gan_des_midi_music_gen_amd import ops
    raw = P.encode(_song(fmt, channels), fmt)
    x = P.decode(raw, fmt, channels)
    pcm = _upload(raw)
    for mix in sorted({-1, 0, channels - 1}):
        _frames_case(ops, pcm, x, fmt, channels, mix, 3, 5, 4, N_SONG - 13, 13, 3, 16)
    # a tail window alone, and a table of many windows one sample apart
    _frames_case(ops, pcm, x, fmt, channels, -1, 0, 0, 0, N_SONG - 37, 37, 1, 8)
    _frames_case(ops, pcm, x, fmt, channels, 0, 1, 1, 170, -1, 37, 1, 16)


def test_both_kernels_beyond_one_trip_of_the_grid_stride_loop():
    """blocks_for caps the grid at 16384 blocks of 256 lanes, four values each: outputs of more than 16 777 216 floats
    take a second trip.  Checked on the device against the decoded signal gathered by torch (64 MiB each)."""
    from gan_des_midi_music_gen_amd import ops
    n = 16384 * 256 * 4 + 1027
    g = torch.Generator().manual_seed(11)
    raw = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    pcm = raw.cuda()
    sig = (pcm.to(torch.int32) - 128).to(torch.float32) * 2.0 ** -7          # U8 mono: every step exact
    P.check_bits(sig[:4096].cpu().numpy(), P.decode(raw[:4096].numpy().tobytes(), P.U8, 1)[:, 0])
    buf, out = _guarded((n - 3,))
    ops.pcm_to_float(pcm, P.U8, 1, 0, n, 3, n - 3, out=out)
    assert torch.equal(out.view(torch.int32), sig[3:].view(torch.int32)) and _guards_intact(buf)
    del buf, out
    win_len, hop, n_fft, start = 8200, 1, 2048, n - 8200                     # 8201 frames of 2048: 16 795 648 floats
    frames = 1 + win_len // hop
    idx = (torch.arange(frames, device="cuda")[:, None] * hop + torch.arange(n_fft, device="cuda")[None, :]
           - n_fft // 2).abs()
    idx = torch.where(idx >= win_len, 2 * (win_len - 1) - idx, idx)
    want = sig[start:start + win_len][idx]
    buf, out = _guarded((frames, n_fft))
    _, got_frames = ops.pcm_stft_frames(pcm, P.U8, 1, -1, n, 0, 0, 0, start, win_len, hop, n_fft, out=out)
    assert got_frames == frames and frames * n_fft > 16384 * 256 * 4
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and _guards_intact(buf)


def test_pcm_stft_frames_refuses_a_bad_window_table():
    from gan_des_midi_music_gen_amd import ops
    raw = P.encode(_song(P.S16, 2), P.S16)
    pcm = _upload(raw)
    base = dict(start0=3, stride=13, n_regular=4, tail=-1, win=13, hop=3, n_fft=16, n=N_SONG)
    bad = [dict(n_regular=17),                   # window 16 would end at 3 + 16 * 13 + 13 = 224 > 211
           dict(tail=N_SONG - 12),               # the tail window one sample past the end
           dict(start0=-1),                      # a negative start
           dict(stride=-2),                      # ... reached by a later window
           dict(win=8),                          # win_len = n_fft / 2: the reflection would leave the window
           dict(n=N_SONG + 1)]                   # more samples than the buffer holds
    for kw in bad:
        a = dict(base)
        a.update(kw)
        frames = 1 + a["win"] // a["hop"]
        buf, out = _guarded(((a["n_regular"] + (a["tail"] >= 0)) * frames, a["n_fft"]))
        with pytest.raises(ops.GdmError):
            ops.pcm_stft_frames(pcm, P.S16, 2, 0, a["n"], a["start0"], a["stride"], a["n_regular"], a["tail"], a["win"],
                                a["hop"], a["n_fft"], out=out)
        assert bool((buf.cpu() == GUARD_VALUE).all()), kw               # no launch
    # too many frames: the wrapper derives `frames` itself, so this one goes to the C entry
    import ctypes
    from gan_des_midi_music_gen_amd import _lib
    buf, out = _guarded((6, 16))
    rc = _lib.load().gdm_pcm_stft_frames(ctypes.c_void_p(pcm.data_ptr()), P.S16, 2, 0, N_SONG, 0, 0, 1, -1, 13, 3, 16, 6,
                                         ctypes.c_void_p(out.data_ptr()), None)
    assert rc == -1 and b"6 frames of hop 3 exceed 13" in _lib.load().gdm_last_error()
    assert bool((buf.cpu() == GUARD_VALUE).all())


def test_pcm_stft_frames_at_the_reference_geometry():
    """output_0_first5s.wav as InputSong cuts it (its one 5-second window, twice), n_fft 2048, hop 1025: the frame matrix
    equals ops.stft_frames on the float windows the mirror decodes, for channel 0 and for the channel mean."""
    from gan_des_midi_music_gen_amd import ops, util
    wav = util.load_wav(os.path.join(WAV_DIR, "output_0_first5s.wav"))
    assert (wav.n_frames, wav.channels, wav.fmt) == (220500, 2, P.S16)
    x = P.decode(wav.data, wav.fmt, wav.channels)
    pcm = util.upload_pcm(wav)
    windows = util.song_windows(wav.n_frames, wav.sample_rate)
    assert windows == [(0, 220500)] * 2
    for mix in (0, -1):
        sig = P.mono(x, mix)
        stacked = torch.from_numpy(np.stack([sig[s:s + n] for s, n in windows])).cuda()
        want, frames = ops.stft_frames(stacked, 1025, 2048)
        buf, out = _guarded(tuple(want.shape))
        got, got_frames = ops.pcm_stft_frames(pcm, wav.fmt, wav.channels, mix, wav.n_frames, 0, 0, 2, -1, 220500, 1025,
                                              2048, out=out)
        assert got_frames == frames == 216
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), mix
        assert _guards_intact(buf)


# ---- InputSong and the file functions -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """(path, (n, 2) fp32 decoded channels, rate) of the generated song (pcm_ref.generated_song)."""
    blob, pcm = P.generated_song()
    path = tmp_path_factory.mktemp("song") / "generated.wav"
    path.write_bytes(blob)
    return str(path), P.decode(pcm.tobytes(), P.S16, 2), 22050


def _song_case(name, generated):
    if name == "generated":
        path, x, rate = generated
        return path, x, rate, 1
    from gan_des_midi_music_gen_amd import util
    path = os.path.join(WAV_DIR, name)
    wav = util.load_wav(path)
    return path, P.decode(wav.data, wav.fmt, wav.channels), wav.sample_rate, 5


def _todays_path(windows_np, rate):
    """What a user computes on the parent commit: the float windows, stacked and uploaded, through
    util.get_melspectrogram_db_tensor."""
    from gan_des_midi_music_gen_amd import util
    return util.get_melspectrogram_db_tensor(torch.from_numpy(np.stack(windows_np)).cuda(), sr=rate)


def _within_the_featurisers_bounds(got, window, rate):
    want = om.get_melspectrogram_db_tensor(np.ascontiguousarray(window), sr=rate)
    assert got.shape == want.shape
    loud = want > want.max() - 60.0
    assert np.abs(got - want)[loud].max() < 0.02, np.abs(got - want)[loud].max()
    assert np.abs(got - want).max() < 0.5, np.abs(got - want).max()


@pytest.mark.parametrize("name", FIXTURES + ["generated"])
def test_input_song_is_todays_featuriser_on_the_same_windows(name, generated):
    from gan_des_midi_music_gen_amd import datasets, util
    path, x, rate, hop_s = _song_case(name, generated)
    n = len(x)
    ds = datasets.InputSong(path, 5, hop_s)
    windows = util.song_windows(n, rate, hop_s)
    frames = {"simulation.wav": 216, "generation_first5s.wav": 216, "output_0_first5s.wav": 216, "generated": 217}[name]
    assert len(ds) == len(windows) == {"simulation.wav": 1, "generated": 4}.get(name, 2)
    assert ds.sample_rate == rate and ds.audio_file_length == n / rate
    assert (ds.window_size, ds.hop_length_audio) == (5, hop_s)
    spec = ds.spectrograms()
    assert spec.is_cuda and spec.dtype == torch.float32 and tuple(spec.shape) == (len(windows), 128, frames)
    assert ds.spectrograms() is spec                                    # computed once
    left = x[:, 0]
    want = _todays_path([left[s:s + m] for s, m in windows], rate)
    assert torch.equal(spec.view(torch.int32), want.view(torch.int32))
    got = spec.cpu().numpy()
    seen = {}
    for i, (s, m) in enumerate(windows):
        if s in seen:                                                   # the repeated last window: the same tensor
            assert np.array_equal(got[i], got[seen[s]])
            continue
        seen[s] = i
        _within_the_featurisers_bounds(got[i], left[s:s + m], rate)
    # items are views of that tensor; negative indices count from the end; past the end is an IndexError
    item = ds[len(ds) - 1]
    assert tuple(item.shape) == (128, frames) and item.data_ptr() == spec[len(ds) - 1].data_ptr()
    assert ds[-1].data_ptr() == item.data_ptr() and ds[-len(ds)].data_ptr() == spec.data_ptr()
    for bad in (len(ds), -len(ds) - 1):
        with pytest.raises(IndexError):
            ds[bad]
    # orig_waveform: what torchaudio.load(normalize=True) returns, (channels, n)
    wave_t = ds.orig_waveform
    assert tuple(wave_t.shape) == (2, n) and ds.orig_waveform is wave_t
    P.check_bits(wave_t.cpu().numpy(), x.T, "orig_waveform")


def test_input_song_chunks_are_todays_path_on_the_same_chunks(generated):
    from gan_des_midi_music_gen_amd import datasets, util
    path, x, rate = generated
    windows = util.song_windows(len(x), rate, 1)
    ds = datasets.InputSong(path, 5, 1, windows_per_chunk=3)
    spec = ds.spectrograms()
    assert tuple(spec.shape) == (4, 128, 217)
    cut = [x[s:s + m, 0] for s, m in windows]
    want = torch.cat([_todays_path(cut[:3], rate), _todays_path(cut[3:], rate)])
    assert torch.equal(spec.view(torch.int32), want.view(torch.int32))
    one = datasets.InputSong(path, 5, 1, windows_per_chunk=1).spectrograms()    # tail-only and single-window tables
    want = torch.cat([_todays_path(cut[i:i + 1], rate) for i in range(4)])
    assert torch.equal(one.view(torch.int32), want.view(torch.int32))


def test_split_audio_data(generated):
    from gan_des_midi_music_gen_amd import util
    path = os.path.join(WAV_DIR, "simulation.wav")
    wav = util.load_wav(path)
    mean = P.mono(P.decode(wav.data, wav.fmt, wav.channels), -1)
    items = util.split_audio_data(path)
    assert len(items) == 1 and items[0].is_cuda and items[0].dtype == torch.float32
    P.check_bits(items[0].cpu().numpy(), mean, "simulation.wav")
    path, x, rate = generated
    mean = P.mono(x, -1)
    items = util.split_audio_data(path, hop_length_audio=1, window_size=2)
    want = [(0, 44100), (22050, 44100), (44100, 28665), (28665, 44100)]          # ragged, as upstream
    assert [tuple(t.shape) for t in items] == [(m,) for _, m in want]
    for t, (s, m) in zip(items, want):
        P.check_bits(t.cpu().numpy(), mean[s:s + m], f"window at {s}")
    assert len({t.untyped_storage().data_ptr() for t in items}) == 1             # slices of one decoded buffer


def test_get_melspectrogram_db_tensor_from_file():
    from gan_des_midi_music_gen_amd import util
    path = os.path.join(WAV_DIR, "simulation.wav")
    wav = util.load_wav(path)
    mean = P.mono(P.decode(wav.data, wav.fmt, wav.channels), -1)
    got = util.get_melspectrogram_db_tensor_from_file(path)
    assert got.is_cuda and tuple(got.shape) == (128, 216)
    want = util.get_melspectrogram_db_tensor(torch.from_numpy(mean).cuda(), sr=wav.sample_rate)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    _within_the_featurisers_bounds(got.cpu().numpy(), mean, wav.sample_rate)


def test_input_song_under_a_dataloader(generated):
    from torch.utils.data import DataLoader
    from gan_des_midi_music_gen_amd import datasets
    ds = datasets.InputSong(generated[0], 5, 1)
    batches = list(DataLoader(ds, batch_size=3, shuffle=False))
    assert [tuple(b.shape) for b in batches] == [(3, 128, 217), (1, 128, 217)]
    assert all(b.is_cuda and b.dtype == torch.float32 for b in batches)
    assert torch.equal(torch.cat(batches), ds.spectrograms())
    shuffled = torch.cat(list(DataLoader(ds, batch_size=3, shuffle=True)))
    assert tuple(shuffled.shape) == (4, 128, 217)


def test_train_from_a_file_is_train_on_its_windows(generated):
    from gan_des_midi_music_gen_amd import SIMNN, datasets
    path = generated[0]
    spec = datasets.InputSong(path, 5, 1).spectrograms()
    *_, g_file, d_file = SIMNN.train(audio_file=path, hop_length_audio=1, batch_size=2, shuffle=False, max_steps=2, seed=0,
                                     save=False, log=lambda *_: None)
    *_, g_list, d_list = SIMNN.train(dataloader=[spec[0:2], spec[2:4]], input_hw=(128, 217), batch_size=2, max_steps=2,
                                     seed=0, save=False, log=lambda *_: None)
    assert len(g_file) == len(d_file) == 2
    assert np.float64(g_file + d_file).tobytes() == np.float64(g_list + d_list).tobytes(), (g_file, d_file, g_list, d_list)
    assert all(np.isfinite(g_file + d_file))
    with pytest.raises(ValueError):
        SIMNN.train(audio_file=path, dataloader=[spec[0:2]], save=False)
    with pytest.raises(ValueError):
        SIMNN.train(audio_file=path, hop_length_audio=1, input_hw=(128, 216), save=False)
