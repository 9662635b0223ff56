"""Mel-spectrogram featuriser on the device: the drop-in for ``get_melspectrogram_db_tensor`` of the reference's
``GAN_DES/util.py:37-61`` (= ``MMGAN_MIDI_DES/util.py``), which turns a mono window into the (128, 216) dB tensor that
model 1's discriminator consumes (first "next" row).

torchaudio's ``MelSpectrogram`` + ``AmplitudeToDB`` are restated as (all fp32):

    frames (gdm_stft_frames: centred, reflect padded)  x  [w*cos | w*sin] (2048 x 2050, Hann window folded in)
      -> gdm_gemm (exact-fp32 MFMA)  -> re^2 + im^2 (gdm_power_spectrum)  x  HTK filter bank (1025 x 128)
      -> gdm_gemm  -> 10 log10(max(., 1e-10)), floored at (window max - top_db)  (gdm_power_to_db)

The DFT is a GEMM on purpose: 1.8 GFLOP per window on matrix cores is cheaper to get right than a hand-written FFT and
is still thousands of windows per second; it is data preparation, not part of the training iteration.
There is no CPU path (the constant matrices are built on the host once per geometry and cached).

From a file (GAN_DES/util.py:89-119, GAN_DES/datasets.py:26-43; torchaudio.load is restated, torchaudio is absent):
``load_wav`` parses the RIFF container on the host, the data chunk's bytes are uploaded once as they are, and the first
launch of the chain becomes ``gdm_pcm_stft_frames``, which decodes, reduces the channels and cuts the (overlapping)
windows while it writes the frame matrix; ``gdm_pcm_to_float`` is the same decode for callers that want the waveform
(``split_audio_data``, ``InputSong.orig_waveform``).  What is pinned: 16-bit PCM, by exact arithmetic and the reference's
own three files; the other sample formats follow torchaudio's documented formula only (include/gdm.h).
"""
import math
import operator
import os
import struct
import warnings

import torch

from . import ops
from .ops import F32

_CONST = {}


def _dft_matrix(n_fft, device):
    """(n_fft, 2 * (n_fft // 2 + 1)) = [w[n] cos(2 pi k n / N) | w[n] sin(2 pi k n / N)], periodic Hann window w."""
    key = ("dft", n_fft, str(device))
    if key not in _CONST:
        n = torch.arange(n_fft, dtype=torch.float64)
        k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
        win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / n_fft)
        # reduce k*n modulo N in integers first: the angle stays exact for large products
        kn = (torch.outer(n.long(), k.long()) % n_fft).to(torch.float64)
        ang = 2.0 * math.pi * kn / n_fft
        # (sin(float64 pi) is 1.2e-16, not 0: the sine columns k = 0 and k = N/2 are exact zeros)
        sin = torch.where((2.0 * kn) % n_fft == 0, torch.zeros_like(ang), torch.sin(ang))
        m = torch.cat([torch.cos(ang), sin], dim=1) * win[:, None]
        _CONST[key] = m.to(torch.float32).to(device).contiguous()
    return _CONST[key]


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk") restated: (n_freqs, n_mels) float64."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


def _mel_matrix(n_fft, sr, n_mels, fmin, fmax, ldp, device):
    key = ("mel", n_fft, sr, n_mels, float(fmin), float(fmax), ldp, str(device))
    if key not in _CONST:
        nfreq = n_fft // 2 + 1
        fb = torch.zeros((ldp, n_mels), dtype=torch.float64)
        fb[:nfreq] = melscale_fbanks(nfreq, float(fmin), float(fmax), n_mels, sr)
        _CONST[key] = fb.to(torch.float32).to(device).contiguous()
    return _CONST[key]


def _db_from_frames(frames_m, b, frames, sr, n_fft, n_mels, fmin, fmax, top_db):
    """(b * frames, n_fft) frame matrix -> (b, n_mels, frames) dB: everything after the first launch of the chain."""
    nfreq = n_fft // 2 + 1
    ldp = (nfreq + 3) // 4 * 4                       # K of the mel GEMM padded to whole 16-byte chunks
    spec = ops.gemm(frames_m, _dft_matrix(n_fft, frames_m.device), compute=F32)          # (B*frames, 2*nfreq)
    power = ops.power_spectrum(spec, nfreq, ldp)
    mel = ops.gemm(power, _mel_matrix(n_fft, sr, n_mels, fmin, fmax, ldp, frames_m.device), compute=F32)
    return ops.power_to_db(mel, b, frames, top_db=top_db)


def melspectrogram_db_batch(waveforms, sr=44100, n_fft=2048, hop=None, n_mels=128, fmin=20, fmax=8300, top_db=80):
    """waveforms (B, L) fp32 on the device -> (B, n_mels, 1 + L // hop) dB (one top_db floor per window)."""
    if not waveforms.is_cuda:
        raise ops.GdmError("melspectrogram_db_batch runs on a HIP device only (no CPU fallback)")
    x = waveforms if waveforms.dtype == torch.float32 else waveforms.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    frames_m, frames = ops.stft_frames(x, hop, n_fft)
    return _db_from_frames(frames_m, x.shape[0], frames, sr, n_fft, n_mels, fmin, fmax, top_db)


def melspectrogram_db_from_pcm(pcm, wav, mix, starts, win_len, sr=44100, n_fft=2048, hop=None, n_mels=128, fmin=20,
                               fmax=8300, top_db=80):
    """melspectrogram_db_batch over windows of a song that stay in the file's own sample format: ``pcm`` is ``wav``'s
    data chunk on the device (``upload_pcm``), ``mix`` a channel index or -1 for the channel mean, ``starts`` the first
    sample of each window (equally spaced, except that the last may lie anywhere: the window taken from the end) and
    ``win_len`` their common length -> (len(starts), n_mels, 1 + win_len // hop) dB.  Same frames, bit for bit, as
    ``ops.stft_frames`` on the decoded windows, in one launch and without the windows."""
    start0, stride, n_regular, tail_start = _window_table(starts)
    frames_m, frames = ops.pcm_stft_frames(pcm, wav.fmt, wav.channels, mix, wav.n_frames, start0, stride, n_regular,
                                           tail_start, win_len, hop, n_fft)
    return _db_from_frames(frames_m, len(starts), frames, sr, n_fft, n_mels, fmin, fmax, top_db)


def melspectrogram_db_from_synth_windows(pcm, n_windows, win_len, out_stride, sr=44100, n_fft=2048, n_mels=128, fmin=20,
                                         fmax=8300, top_db=80):
    """The mel-dB tensors of the windows ``ops.synth_windows`` rendered: ``pcm`` is its (n_windows, out_stride) int16
    buffer, read as one mono 16-bit song whose windows start ``out_stride`` samples apart; ``win_len`` is the length a
    window has in the clip, cut to ``mel_geometry(win_len)`` as ``get_melspectrogram_db_tensor`` cuts it ->
    (n_windows, n_mels, 216) dB.  The chain of the WAV route (``melspectrogram_db_from_pcm``) from its first launch on,
    so the result is the one a WAV file holding these samples gives."""
    n_windows, out_stride = int(n_windows), int(out_stride)
    if pcm.dtype != torch.int16 or pcm.numel() != n_windows * out_stride or not pcm.is_contiguous():
        raise ops.GdmError(f"melspectrogram_db_from_synth_windows: pcm must be a contiguous ({n_windows}, {out_stride}) "
                           "int16 tensor")
    hop, kept = mel_geometry(int(win_len))
    if kept > out_stride:
        raise ValueError(f"windows of {win_len} samples do not fit rows of {out_stride}")
    frames_m, frames = ops.pcm_stft_frames(pcm.view(torch.uint8).reshape(-1), ops.PCM_S16, 1, 0, n_windows * out_stride,
                                           0, out_stride, n_windows, -1, kept, hop, n_fft)
    return _db_from_frames(frames_m, n_windows, frames, sr, n_fft, n_mels, fmin, fmax, top_db)


def _window_table(starts):
    """Window starts -> (start0, stride, n_regular, tail_start) of gdm_pcm_stft_frames (scalars, so that the C entry can
    check every window against the buffer)."""
    starts = [int(v) for v in starts]
    if not starts or min(starts) < 0:
        raise ValueError("melspectrogram_db_from_pcm needs at least one window, none starting before the song")
    if len(starts) == 1:
        return starts[0], 0, 1, -1
    stride = starts[1] - starts[0]
    even = [starts[0] + i * stride for i in range(len(starts))]
    if starts == even:
        return starts[0], stride, len(starts), -1
    if starts[:-1] == even[:-1]:
        return starts[0], stride, len(starts) - 1, starts[-1]
    raise ValueError("window starts must be equally spaced, except for the last one")


def get_melspectrogram_db_tensor(waveform, sr=44100, n_fft=2048, hop_length=512, n_mels=128, fmin=20, fmax=8300,
                                 top_db=80, mel_length=216):
    """Same signature and result as the reference (util.py:37-61): waveform (L,) -> (n_mels, frames) dB tensor.
    Like there, ``hop_length`` is overridden by ``len(waveform) // (mel_length - 1)`` and the input is cropped to
    ``mel_length * hop`` samples.  A (B, L) batch is accepted too and returns (B, n_mels, frames)."""
    single = waveform.dim() == 1
    x = waveform.unsqueeze(0) if single else waveform
    hop = x.shape[1] // (mel_length - 1)
    x = x[:, : mel_length * hop]
    out = melspectrogram_db_batch(x, sr=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, fmin=fmin, fmax=fmax, top_db=top_db)
    return out[0] if single else out


def mel_geometry(length, mel_length=216):
    """The reference's rule (util.py:40-44) for a window of ``length`` samples -> (hop, samples kept after the crop)."""
    hop = length // (mel_length - 1)
    if hop <= 0:
        raise ValueError(f"a window of {length} samples is shorter than the {mel_length - 1} hops it is cut into")
    return hop, min(length, mel_length * hop)


# ---- WAV files (torchaudio.load(normalize=True) restated: GAN_DES/datasets.py:26, util.py:90,104) ---------------------
_KS_SUBFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")     # KSDATAFORMAT_SUBTYPE_*: the tag + this GUID tail


class WavData:
    """What ``load_wav`` returns: ``data`` (zero-copy view of the data chunk, whole sample frames only), ``fmt`` (an
    ``ops.PCM_*`` code), ``channels``, ``sample_rate``, ``n_frames``."""

    def __init__(self, data, fmt, channels, sample_rate, n_frames):
        self.data, self.fmt, self.channels, self.sample_rate, self.n_frames = data, fmt, channels, sample_rate, n_frames


def load_wav(path_or_bytes):
    """Host RIFF/WAVE reader (sequential byte work, like ``datasets.read_midi``): PCM of 8 / 16 / 24 / 32 bits and 32-bit
    IEEE float, plain or WAVE_FORMAT_EXTENSIBLE, 1 to 8 channels.  Nothing is decoded: the samples stay the file's bytes.
    A data chunk whose size field is 0, 0xFFFFFFFF or reaches beyond the file (streamed writers) runs to the end of the
    file; a trailing partial sample frame is dropped."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        buf = memoryview(path_or_bytes).cast("B")
    else:
        with open(path_or_bytes, "rb") as f:
            raw = bytearray(f.read())                  # writable: torch.frombuffer can share it without a copy
        buf = memoryview(raw)
    if len(buf) < 12 or bytes(buf[8:12]) != b"WAVE" or bytes(buf[:4]) not in (b"RIFF", b"RIFX"):
        raise ValueError("not a RIFF/WAVE file")
    if bytes(buf[:4]) == b"RIFX":
        raise ValueError("big-endian RIFX files are not supported")
    fmt_chunk = data = None
    pos = 12
    while pos + 8 <= len(buf) and (fmt_chunk is None or data is None):
        tag = bytes(buf[pos:pos + 4])
        size = struct.unpack_from("<I", buf, pos + 4)[0]
        pos += 8
        if tag == b"data":
            if size in (0, 0xFFFFFFFF) or pos + size > len(buf):
                size = len(buf) - pos
            data = buf[pos:pos + size]
        elif tag == b"fmt ":
            if size < 16 or pos + size > len(buf):
                raise ValueError("truncated fmt chunk")
            fmt_chunk = buf[pos:pos + size]
        pos += size + (size & 1)                       # chunks are padded to even sizes
    if fmt_chunk is None:
        raise ValueError("no fmt chunk")
    if data is None:
        raise ValueError("no data chunk")
    tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", fmt_chunk, 0)
    if tag == 0xFFFE:                                  # WAVE_FORMAT_EXTENSIBLE: the real tag heads the sub-format GUID
        if len(fmt_chunk) < 40 or bytes(fmt_chunk[26:40]) != _KS_SUBFORMAT_TAIL:
            raise ValueError("WAVE_FORMAT_EXTENSIBLE with an unknown sub-format")
        tag = struct.unpack_from("<H", fmt_chunk, 24)[0]
    if tag == 1 and bits in (8, 16, 24, 32):
        fmt = {8: ops.PCM_U8, 16: ops.PCM_S16, 24: ops.PCM_S24, 32: ops.PCM_S32}[bits]
    elif tag == 3 and bits == 32:
        fmt = ops.PCM_F32
    elif tag == 3:
        raise ValueError(f"{bits}-bit float samples are not supported (32-bit only)")
    else:
        raise ValueError(f"unsupported WAV format tag {tag:#x} with {bits} bits (uncompressed PCM or 32-bit float only)")
    if not 1 <= channels <= 8:
        raise ValueError(f"{channels} channels (1 to 8 are supported)")
    if block_align != channels * ops.PCM_BYTES[fmt]:
        raise ValueError(f"block align {block_align} is not {channels} x {ops.PCM_BYTES[fmt]} bytes")
    n_frames = len(data) // block_align
    if n_frames == 0:
        raise ValueError("empty data chunk")
    return WavData(data[:n_frames * block_align], fmt, channels, rate, n_frames)


def wav_header(n_samples, sample_rate=44100):
    """The 44 bytes in front of ``n_samples`` mono 16-bit samples: RIFF/WAVE, one fmt chunk, the data chunk's head."""
    return (b"RIFF" + struct.pack("<I", 36 + 2 * n_samples) + b"WAVEfmt " +
            struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, 2 * sample_rate, 2, 16) +
            b"data" + struct.pack("<I", 2 * n_samples))


_WAV_CHUNK = 1 << 22          # samples rendered per synth launch (8 MB of PCM)


def write_wav_chunks(path, total, render, *, blank=False, max_seconds=None, rate=ops.SYNTH_RATE, chunk=None):
    """A clip of ``total`` samples as a mono 16-bit WAV file, rendered on the device in bounded chunks:
    ``render(first, count)`` -> int16 tensor of samples [first, first + count).  A ``blank`` clip is five seconds of
    silence (the reference's ``np.zeros(5 * 44100)``, GAN_DES/matrix_sim_process.py:103) and ``render`` is not called;
    ``max_seconds`` cuts the clip.  Directories are created.  chunk: samples per ``render`` call (default: _WAV_CHUNK).
    Returns the samples written."""
    chunk = chunk or _WAV_CHUNK
    if blank:
        total = 5 * rate
    if max_seconds is not None:
        total = max(1, min(total, int(max_seconds * rate)))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(wav_header(total, rate))
        for first in range(0, total, chunk):
            count = min(chunk, total - first)
            f.write(bytes(2 * count) if blank else render(first, count).cpu().numpy().astype("<i2").tobytes())
    return total


def upload_pcm(wav, device="cuda"):
    """The data chunk's bytes as a uint8 device tensor: the one upload of the file-based paths."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)   # a read-only source (bytes) is only read
        host = torch.frombuffer(wav.data, dtype=torch.uint8)
    return host.to(device)


def song_windows(n, sample_rate, hop_length_audio=5, window_size=5, mode="input_song"):
    """The window loops of the reference in integers -> list of (start, length) in samples.

    mode "input_song" (GAN_DES/datasets.py:38-43): windows of hop_length_audio seconds, hop_length_audio seconds apart;
    ``window_size`` is stored but unused there, and so it is here.  mode "split" (util.py:113-118, split_audio_data):
    windows of window_size seconds, hop_length_audio seconds apart.  Both iterate ``np.arange(0, n + 1, hop * sr)`` and
    take the last ``w`` samples of the song once fewer than one hop remain, so, as upstream:
      * a song whose length is an exact multiple of the hop yields its last window twice (i = n is visited);
      * a song shorter than one window yields one window holding the whole song (``x[-w:]`` of a shorter ``x``);
      * in "input_song" mode all windows of a song have one length; in "split" mode they may be ragged.
    Seconds that are not integers raise TypeError, as the slices do upstream."""
    if mode not in ("input_song", "split"):
        raise ValueError(f"unknown mode {mode!r}")
    n, sample_rate = operator.index(n), operator.index(sample_rate)
    step = operator.index(hop_length_audio) * sample_rate
    w = step if mode == "input_song" else operator.index(window_size) * sample_rate
    if n <= 0 or step <= 0 or w <= 0:
        raise ValueError("song length, sample rate, hop and window must be positive")
    out = []
    for i in range(0, n + 1, step):
        if i + step > n:
            out.append((max(0, n - w), min(n, w)))                     # waveform[-w:]
        else:
            out.append((i, min(w, n - i)))                             # waveform[i:i + w]
    return out


def split_audio_data(wav_file_path, hop_length_audio=5, window_size=5, device="cuda"):
    """Reference signature (util.py:103-119) plus ``device``: the channel mean of the file cut into windows of
    window_size seconds every hop_length_audio seconds -> list of 1-D fp32 device tensors (views of one buffer that one
    launch decodes; the last ones may be shorter or repeat the song's end, as upstream)."""
    wav = load_wav(wav_file_path)
    windows = song_windows(wav.n_frames, wav.sample_rate, hop_length_audio, window_size, mode="split")
    mono = ops.pcm_to_float(upload_pcm(wav, device), wav.fmt, wav.channels, -1, wav.n_frames)
    return [mono[s:s + l] for s, l in windows]


def get_melspectrogram_db_tensor_from_file(file_path, device="cuda"):
    """Reference signature (util.py:89-100) plus ``device``: the whole file as one window, channel mean, the file's own
    sample rate for the filter bank; hop, crop and frame count as in ``get_melspectrogram_db_tensor``."""
    wav = load_wav(file_path)
    hop, win_len = mel_geometry(wav.n_frames)
    return melspectrogram_db_from_pcm(upload_pcm(wav, device), wav, -1, [0], win_len, sr=wav.sample_rate, hop=hop)[0]
