"""numpy mirror of the PCM front end (include/gdm.h: gdm_pcm_to_float, gdm_pcm_stft_frames) and its checker.

The arithmetic is defined exactly (one fp32 per stored sample first, channels added left to right in fp32, one correctly
rounded division), every step below is a single IEEE fp32 operation in numpy, and so the checker demands equal bits.
S16 is what the reference's files hold and what torchaudio.load(normalize=True) is pinned for (v / 32768, exact); the
other formats follow torchaudio's documented formula and nothing else.
"""
import struct

import numpy as np

U8, S16, S24, S32, F32 = range(5)
BYTES = (1, 2, 3, 4, 4)
F = np.float32


class CheckError(AssertionError):
    pass


def check_bits(got, want, what=""):
    """Equal shape and equal int32 views: -0.0 differs from 0.0, a denormal from 0, one ulp from none."""
    got = np.ascontiguousarray(np.asarray(got), dtype=np.float32)
    want = np.ascontiguousarray(np.asarray(want), dtype=np.float32)
    if got.shape != want.shape:
        raise CheckError(f"{what}: shape {got.shape} vs {want.shape}")
    bad = np.flatnonzero(got.view(np.int32).ravel() != want.view(np.int32).ravel())
    if bad.size:
        i = int(bad[0])
        raise CheckError(f"{what}: {bad.size} of {got.size} values differ in their bits, first at {i}: "
                         f"{got.ravel()[i]!r} vs {want.ravel()[i]!r}")


def decode(raw, fmt, channels):
    """bytes of interleaved little-endian frames -> (n, channels) fp32, one value per stored sample."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    n = raw.size // (BYTES[fmt] * channels)
    raw = raw[:n * BYTES[fmt] * channels]
    if fmt == U8:
        x = (raw.astype(np.int32) - 128).astype(F) * F(2.0 ** -7)
    elif fmt == S16:
        x = raw.view("<i2").astype(F) * F(2.0 ** -15)
    elif fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(F) * F(2.0 ** -23)                       # |v| < 2^24: the conversion is exact
    elif fmt == S32:
        x = raw.view("<i4").astype(F) * F(2.0 ** -31)         # int32 -> fp32 rounds to nearest even; the scale is exact
    elif fmt == F32:
        x = raw.view("<f4").copy()
    else:
        raise ValueError(fmt)
    return x.reshape(n, channels)


def mono(x, mix):
    """(n, channels) -> (n,): channel ``mix``, or for mix = -1 the channels added left to right, then divided once."""
    if mix >= 0:
        return x[:, mix].copy()
    acc = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        acc = acc + x[:, c]
    return acc / F(x.shape[1])


def starts_of(start0, stride, n_regular, tail_start):
    return [start0 + w * stride for w in range(n_regular)] + ([tail_start] if tail_start >= 0 else [])


def frames_matrix(signal, starts, win_len, hop, n_fft):
    """(len(starts) * frames, n_fft): centred frames of each window, reflect padding inside the window."""
    frames = 1 + win_len // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    idx = np.abs(idx)
    idx = np.where(idx >= win_len, 2 * (win_len - 1) - idx, idx)
    assert idx.min() >= 0 and idx.max() < win_len
    return np.concatenate([signal[s:s + win_len][idx] for s in starts]).astype(F), frames


def encode(values, fmt):
    """Integer (or, for F32, float) sample values, any shape, C order -> the bytes a WAV data chunk holds."""
    v = np.asarray(values)
    if fmt == U8:
        return v.astype(np.uint8).tobytes()
    if fmt == S16:
        return v.astype("<i2").tobytes()
    if fmt == S24:
        u = (v.astype(np.int64) & 0xFFFFFF).ravel()
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    if fmt == S32:
        return v.astype("<i4").tobytes()
    return v.astype("<f4").tobytes()


def wav_bytes(data, fmt, channels, rate, extensible=False, data_size=None, extra_chunks=()):
    """A RIFF/WAVE file around ``data``.  extra_chunks: (tag, body) pairs written in front of the data chunk (padded to
    even sizes as the format demands); data_size: the size field to write instead of the true one."""
    bits = BYTES[fmt] * 8
    tag = 3 if fmt == F32 else 1
    block = BYTES[fmt] * channels
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        head += struct.pack("<HHIH", 22, bits, 0, tag) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head
    for ctag, cbody in extra_chunks:
        body += ctag + struct.pack("<I", len(cbody)) + cbody + (b"\0" if len(cbody) & 1 else b"")
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def generated_song():
    """The generated song of the tests: 22 050 Hz, 72 765 samples, stereo S16 -> (file bytes, (n, 2) int16 samples).
    With hop_length_audio = 1 it has four windows of 22 050 samples, the last one taken from the end (start 50 715)."""
    rate, n = 22050, 72765
    t = np.arange(n) / rate
    g = np.random.default_rng(20240)
    left = 0.4 * np.sin(2 * np.pi * 440.0 * t * (1 + 0.1 * t)) + 0.02 * g.standard_normal(n)
    right = 0.3 * np.sin(2 * np.pi * 1250.0 * t) * np.clip(np.sin(2 * np.pi * 0.9 * t) + 0.5, 0, 1) \
        + 0.02 * g.standard_normal(n)
    pcm = np.round(np.stack([left, right], axis=1) * 32767.0).clip(-32768, 32767).astype("<i2")
    return wav_bytes(pcm.tobytes(), S16, 2, rate), pcm
