"""CPU: the host side of model 1's file input -- util.load_wav (RIFF/WAVE reader), util.song_windows (the reference's
two window loops, GAN_DES/datasets.py:38-43 and util.py:113-118, in integers) -- and the numpy mirror of the device PCM
front end (tests/pcm_ref.py), whose bit comparison must reject planted faults."""
import os
import struct
import sys
import wave

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pcm_ref as P  # noqa: E402

from gan_des_midi_music_gen_amd import util  # noqa: E402

WAV_DIR = os.path.join(HERE, "golden", "wav")
FIXTURES = ["simulation.wav", "generation_first5s.wav", "output_0_first5s.wav"]


# ---- load_wav ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_load_wav_reads_the_fixtures_like_wave_and_scipy(name):
    from scipy.io import wavfile
    path = os.path.join(WAV_DIR, name)
    got = util.load_wav(path)
    with wave.open(path) as w:
        assert (got.sample_rate, got.channels, got.n_frames) == (w.getframerate(), w.getnchannels(), w.getnframes())
        assert w.getsampwidth() == 2 and got.fmt == P.S16
        assert bytes(got.data) == w.readframes(w.getnframes())
    rate, data = wavfile.read(path)
    assert rate == got.sample_rate and data.shape == (got.n_frames, got.channels)
    assert bytes(got.data) == data.astype("<i2").tobytes()
    assert isinstance(got.data, memoryview)
    # a path and the file's bytes are the same thing to the reader
    same = util.load_wav(open(path, "rb").read())
    assert bytes(same.data) == bytes(got.data) and same.n_frames == got.n_frames


def _samples(fmt, n, channels, seed=0):
    g = np.random.default_rng(seed)
    if fmt == P.F32:
        return g.standard_normal((n, channels)).astype(np.float32)
    bits = P.BYTES[fmt] * 8
    lo, hi = (0, 256) if fmt == P.U8 else (-(1 << (bits - 1)), 1 << (bits - 1))
    return g.integers(lo, hi, size=(n, channels))


def test_load_wav_skips_an_odd_sized_chunk_and_its_pad_byte(tmp_path):
    data = P.encode(_samples(P.S16, 11, 2), P.S16)
    blob = P.wav_bytes(data, P.S16, 2, 8000, extra_chunks=[(b"LIST", b"INFOabc")])      # 7 bytes + 1 pad byte
    assert blob[36:40] == b"LIST" and blob[40:44] == struct.pack("<I", 7) and blob[52:56] == b"data"
    path = tmp_path / "list.wav"
    path.write_bytes(blob)
    got = util.load_wav(str(path))
    assert (got.fmt, got.channels, got.sample_rate, got.n_frames) == (P.S16, 2, 8000, 11)
    assert bytes(got.data) == data


@pytest.mark.parametrize("fmt,channels", [(P.S24, 3), (P.F32, 2)])
def test_load_wav_reads_extensible_headers(tmp_path, fmt, channels):
    data = P.encode(_samples(fmt, 9, channels), fmt)
    path = tmp_path / "ext.wav"
    path.write_bytes(P.wav_bytes(data, fmt, channels, 48000, extensible=True))
    got = util.load_wav(str(path))
    assert (got.fmt, got.channels, got.sample_rate, got.n_frames) == (fmt, channels, 48000, 9)
    assert bytes(got.data) == data


@pytest.mark.parametrize("fmt", [P.U8, P.S16, P.S24, P.S32, P.F32])
def test_load_wav_reads_every_plain_format(fmt):
    data = P.encode(_samples(fmt, 5, 1), fmt)
    got = util.load_wav(P.wav_bytes(data, fmt, 1, 16000))
    assert (got.fmt, got.channels, got.n_frames) == (fmt, 1, 5) and bytes(got.data) == data


@pytest.mark.parametrize("size_field", [0, 0xFFFFFFFF, 10 ** 6])
def test_load_wav_data_size_that_means_to_the_end_of_the_file(tmp_path, size_field):
    data = P.encode(_samples(P.S16, 13, 2), P.S16)
    path = tmp_path / "stream.wav"
    path.write_bytes(P.wav_bytes(data, P.S16, 2, 44100, data_size=size_field))
    got = util.load_wav(str(path))
    assert got.n_frames == 13 and bytes(got.data) == data


def test_load_wav_drops_a_trailing_partial_frame():
    data = P.encode(_samples(P.S24, 7, 2), P.S24)
    got = util.load_wav(P.wav_bytes(data + b"\x01\x02\x03\x04", P.S24, 2, 44100))        # 4 of a frame's 6 bytes
    assert got.n_frames == 7 and bytes(got.data) == data


def _fmt_chunk(tag, channels, bits, block=None):
    block = channels * bits // 8 if block is None else block
    return struct.pack("<HHIIHH", tag, channels, 8000, 8000 * block, block, bits)


def _riff(chunks, magic=b"RIFF"):
    body = b"WAVE" + b"".join(t + struct.pack("<I", len(b)) + b + (b"\0" if len(b) & 1 else b"") for t, b in chunks)
    return magic + struct.pack("<I", len(body)) + body


@pytest.mark.parametrize("blob", [
    _riff([(b"fmt ", _fmt_chunk(1, 1, 16)), (b"data", b"\0" * 8)], magic=b"RIFX"),      # big-endian container
    _riff([(b"data", b"\0" * 8)]),                                                        # no fmt chunk
    _riff([(b"fmt ", _fmt_chunk(1, 1, 16)), (b"LIST", b"INFO")]),                         # no data chunk
    _riff([(b"fmt ", _fmt_chunk(0x11, 1, 4, block=256)), (b"data", b"\0" * 256)]),        # IMA ADPCM
    _riff([(b"fmt ", _fmt_chunk(0x55, 2, 0, block=1)), (b"data", b"\0" * 64)]),           # MPEG layer 3
    _riff([(b"fmt ", _fmt_chunk(6, 1, 8)), (b"data", b"\0" * 64)]),                       # A-law
    _riff([(b"fmt ", _fmt_chunk(3, 1, 64)), (b"data", b"\0" * 64)]),                      # 64-bit float
    _riff([(b"fmt ", _fmt_chunk(1, 9, 16)), (b"data", b"\0" * 36)]),                      # nine channels
    _riff([(b"fmt ", _fmt_chunk(1, 2, 16)), (b"data", b"")]),                             # nothing in the data chunk
    _riff([(b"fmt ", _fmt_chunk(1, 2, 16)), (b"data", b"\0" * 3)]),                       # less than one frame
    b"RIFF\x04\x00\x00\x00AVI ",
], ids=["rifx", "no-fmt", "no-data", "adpcm", "mp3", "alaw", "f64", "nine-channels", "empty", "partial-only", "not-wave"])
def test_load_wav_refuses(blob):
    with pytest.raises(ValueError):
        util.load_wav(blob)


# ---- song_windows ------------------------------------------------------------------------------------------------------
def _reference_slices(n, sr, hop, window, input_song):
    """The two loops as the reference writes them, on np.arange(n) standing in for the waveform: (first, length)."""
    waveform = np.arange(n)
    out = []
    if input_song:                                                    # GAN_DES/datasets.py:38-43
        for i in np.arange(0, len(waveform) + 1, hop * sr):
            if i + hop * sr > len(waveform):
                out.append(waveform[-hop * sr:])
            else:
                out.append(waveform[i:i + hop * sr])
    else:                                                             # GAN_DES/util.py:113-118
        for i in np.arange(0, len(waveform) + 1, hop * sr):
            if i + hop * sr > len(waveform):
                out.append(waveform[-window * sr:])
            else:
                out.append(waveform[i:i + window * sr])
    return [(int(x[0]), len(x)) for x in out]


def test_song_windows_is_the_reference_loops():
    cases = 0
    for mode in ("input_song", "split"):
        for n in (1, 5, 9, 10, 11, 19, 20, 21, 29, 30, 31, 33, 47):
            for hop in (1, 2, 3):
                for window in (1, 2, 3, 5):
                    want = _reference_slices(n, 10, hop, window, mode == "input_song")
                    got = util.song_windows(n, 10, hop, window, mode=mode)
                    assert got == want, (mode, n, hop, window, got, want)
                    cases += 1
    assert cases == 312


def test_song_windows_on_the_fixtures_and_its_quirks():
    assert util.song_windows(220500, 44100) == [(0, 220500)] * 2       # an exact multiple of the hop: last window twice
    assert util.song_windows(110250, 22050) == [(0, 110250)] * 2
    assert util.song_windows(88576, 44100) == [(0, 88576)]             # shorter than one window: the whole file
    got = util.song_windows(72765, 22050, 1)                           # the generated song of the GPU tests
    assert got == [(0, 22050), (22050, 22050), (44100, 22050), (50715, 22050)]
    assert len({length for _, length in util.song_windows(1000003, 44100, 3, 7)}) == 1   # one length per file
    assert util.song_windows(25, 10, 1, 2, mode="split") == [(0, 20), (10, 15), (5, 20)]   # ragged in split mode
    for bad in (dict(hop_length_audio=2.5), dict(window_size=1.5, mode="split"), dict(hop_length_audio="5")):
        with pytest.raises(TypeError):
            util.song_windows(100, 10, **bad)
    with pytest.raises(ValueError):
        util.song_windows(100, 10, 0)
    with pytest.raises(ValueError):
        util.song_windows(100, 10, mode="maestro")


# ---- the mirror and its checker ------------------------------------------------------------------------------------------
def test_mirror_values_at_the_edges_of_every_format():
    x = P.decode(P.encode([0, 128, 255], P.U8), P.U8, 1)[:, 0]
    assert x.tolist() == [-1.0, 0.0, 127 / 128]
    x = P.decode(P.encode([-32768, 32767, 1], P.S16), P.S16, 1)[:, 0]
    assert x.tolist() == [-1.0, 32767 / 32768, 2.0 ** -15]
    x = P.decode(P.encode([-(1 << 23), (1 << 23) - 1, -1], P.S24), P.S24, 1)[:, 0]
    assert x.tolist() == [-1.0, 1.0 - 2.0 ** -23, -2.0 ** -23]
    x = P.decode(P.encode([-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 3], P.S32), P.S32, 1)[:, 0]
    assert x.tolist() == [-1.0, 1.0, 2.0 ** -7, 2.0 ** -7 + 2.0 ** -29]      # ties to even: ...+1 down, ...+3 up
    x = P.decode(P.encode(np.float32([-0.0, 1e-41, -3.5]), P.F32), P.F32, 1)[:, 0]
    assert np.signbit(x[0]) and x[1] == np.float32(1e-41) and x[1] != 0 and x[2] == -3.5
    # S16 is torchaudio's v / 32768 exactly, and what tests/test_mel.py decodes by hand
    v = np.arange(-32768, 32768, dtype=np.int16)
    P.check_bits(P.decode(v.tobytes(), P.S16, 1)[:, 0], v.astype(np.float32) / 32768.0)
    # mean: left to right, one division
    x = np.float32([[1.0, 2.0 ** -24, 2.0 ** -24]])
    assert P.mono(x, -1)[0] == np.float32(1.0) / np.float32(3.0) and P.mono(x, 2)[0] == 2.0 ** -24


def test_the_bit_comparison_rejects_planted_faults():
    g = np.random.default_rng(5)
    # S32 stereo: the sum of two rounded samples is not the rounded integer sum
    v = g.integers(-(1 << 31), 1 << 31, size=(4096, 2))
    want = P.mono(P.decode(P.encode(v, P.S32), P.S32, 2), -1)
    wrong = (v.sum(axis=1).astype(np.float32) * np.float32(2.0 ** -31)) / np.float32(2.0)
    P.check_bits(want, want.copy())
    with pytest.raises(P.CheckError):
        P.check_bits(wrong, want, "S32 summed as integers")
    # mean taken as channel 0
    x = P.decode(P.encode(g.integers(-32768, 32768, size=(300, 2)), P.S16), P.S16, 2)
    with pytest.raises(P.CheckError):
        P.check_bits(P.mono(x, 0), P.mono(x, -1), "mean taken as channel 0")
    # scale 2^-15 on S24
    v24 = g.integers(-(1 << 23), 1 << 23, size=(300, 1))
    want = P.decode(P.encode(v24, P.S24), P.S24, 1)
    with pytest.raises(P.CheckError):
        P.check_bits(v24.astype(np.float32) * np.float32(2.0 ** -15), want, "S16's scale on S24")
    # reflect across the window edge into the neighbour: pad the SONG around the window instead of the window
    song = np.arange(211, dtype=np.float32)
    starts, win_len, hop, n_fft = [0, 13, 26], 13, 3, 16
    want, frames = P.frames_matrix(song, starts, win_len, hop, n_fft)
    assert frames == 5 and want.shape == (15, 16)
    rows = []
    for s in starts:
        idx = s + np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
        rows.append(song[np.abs(idx)])                                  # reads the neighbours' samples
    with pytest.raises(P.CheckError):
        P.check_bits(np.concatenate(rows), want, "padding taken from the neighbouring window")
    # and a sign of zero or a denormal flushed is a difference too
    with pytest.raises(P.CheckError):
        P.check_bits(np.float32([0.0]), np.float32([-0.0]))
    with pytest.raises(P.CheckError):
        P.check_bits(np.float32([0.0]), np.float32([1e-41]))
    with pytest.raises(P.CheckError):
        P.check_bits(np.zeros(3, np.float32), np.zeros(4, np.float32))


def test_mirror_frames_are_torch_stft_padding():
    """frames_matrix == the frames torch.stft(center=True, pad_mode='reflect') cuts from each window on its own."""
    song = np.random.default_rng(1).standard_normal(211).astype(np.float32)
    for win_len, hop, n_fft in ((9, 1, 16), (13, 3, 8), (37, 5, 16)):
        got, frames = P.frames_matrix(song, [3, 50], win_len, hop, n_fft)
        for k, s in enumerate((3, 50)):
            padded = np.pad(song[s:s + win_len], n_fft // 2, mode="reflect")
            want = np.stack([padded[f * hop:f * hop + n_fft] for f in range(frames)])
            P.check_bits(got[k * frames:(k + 1) * frames], want)


def test_new_ops_refuse_cpu_tensors():
    import torch
    from gan_des_midi_music_gen_amd import ops
    pcm = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ops.GdmError):
        ops.pcm_to_float(pcm, ops.PCM_S16, 1, 0, 32)
    with pytest.raises(ops.GdmError):
        ops.pcm_stft_frames(pcm, ops.PCM_S16, 1, 0, 32, 0, 8, 2, -1, 16, 4, 8)


def test_pcm_entry_points_validate_before_any_launch():
    """Argument checks happen on the host (safe without a GPU): a window table that leaves the buffer is an error code."""
    import ctypes
    from gan_des_midi_music_gen_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    out = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    o = ctypes.c_void_p((ctypes.addressof(out) + 15) & ~15)

    def frames(**kw):
        a = dict(fmt=1, channels=1, mix=0, n=32, start0=0, stride=8, n_regular=3, tail=-1, win=16, hop=4, n_fft=8, fr=5)
        a.update(kw)
        return lib.gdm_pcm_stft_frames(p, a["fmt"], a["channels"], a["mix"], a["n"], a["start0"], a["stride"],
                                       a["n_regular"], a["tail"], a["win"], a["hop"], a["n_fft"], a["fr"], o, None)

    for kw in (dict(n_regular=4), dict(start0=-1), dict(tail=17), dict(win=4), dict(fr=6), dict(fmt=5), dict(channels=9),
               dict(mix=1), dict(mix=-2), dict(n_regular=0), dict(stride=-8), dict(n_fft=6), dict(win=33),
               dict(stride=1 << 62), dict(n=1 << 62)):
        assert frames(**kw) == -1, kw
        assert b"gdm_pcm_stft_frames" in lib.gdm_last_error()
    assert lib.gdm_pcm_to_float(p, 1, 1, 0, 32, 30, 3, o, None) == -1
    assert lib.gdm_pcm_to_float(p, 1, 1, 0, 32, -1, 3, o, None) == -1
    assert lib.gdm_pcm_to_float(p, 7, 1, 0, 32, 0, 3, o, None) == -1
    assert lib.gdm_pcm_to_float(p, 1, 9, 0, 32, 0, 3, o, None) == -1
    assert lib.gdm_pcm_to_float(ctypes.c_void_p(ctypes.addressof(buf) + 1), 1, 1, 0, 16, 0, 3, o, None) == -1
