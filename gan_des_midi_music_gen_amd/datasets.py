"""Drop-in surface of the two data paths on MI355X: model 2's piano rolls (MMGAN_MIDI_DES/datasets.py, SURVEY.md
section 8f row 3) and model 1's single-song dataset (GAN_DES/datasets.py:17-52, "the single-song dataset of BASELINE
config 1").

    InputSong(audio_file, window_size=5, hop_length_audio=5, device='cuda')                     GAN_DES/datasets.py:17-52
    generate_piano_roll(midi_input, sequence_length=100, beats_length=50, start=0, end=50)      datasets.py:13-70
    MaestroDatasetMidi(root_dir, sequence_length=100, beats_length=50, device='cpu')            datasets.py:103-123
    MaestroDatasetPickle(pickle_file_name, sequence_length=100, beats_length=50, device='cpu')  datasets.py:73-87
    MaestroDatasetTorch(root_dir, sequence_length=100, beats_length=50, device='cpu')           datasets.py:90-100
    MaestroWindows.from_midi(root_dir_or_list, sample_size=300, sequence_length=50, ...)        notebook cells 10-11
    MaestroDataset(batch_size, input_folder=..., device='cuda'), my_collate                     GAN_DES/datasets.py:55-100

``generate_piano_roll`` keeps the reference's signature and return value (numpy ``piano_roll (128, W)``, ``durations
(128, W)``, ``beats (beats_length,)``); ``generate_piano_rolls`` is the batched form the training data path wants: a list
of files in, the (F, 128, W) fp32 planes as DEVICE tensors out (one kernel launch for all files, nothing copied back).

What runs where: a Standard MIDI File is a byte stream with running status and variable-length quantities -- parsing is
sequential host work (``read_midi``); merging tracks, tick -> second conversion, the one-second step index and the
point where the reference's event loop stops are vectorised numpy on the host (a few thousand messages per file); the
raster itself -- last-write-wins scatter of velocities, range fill of durations, per (file, note) row -- is the device
kernel (``ops.piano_roll_raster``, csrc/piano_roll.hip).

mido and pretty_midi are not importable here; their behaviour is restated (see oracle/piano_roll.py for the statement
of what is and is not pinned: PARITY UNPINNED).  The reference's control flow is kept as it is, including: the step
index is absolute although the planes are only ``end - start`` wide (a note_on beyond the width ends the event loop:
IndexError inside the reference's bare ``try``), messages at ``sequence_length`` seconds or later end it as well, and
the final slice is ``[:, start:end]`` of the already ``end - start`` wide planes (empty for start >= end - start).

``MaestroWindows`` is the dataset model 2 trains on, built the way data_viewing_and_processing.ipynb cell 11 builds
``preprocessed_data_50.pkl``: every file's (128, sample_size) planes of cell 10 cut into windows of ``sequence_length``
steps, window 0 dropped.  The host plans (``window_plan``: which windows a file yields, from the rounded running time
of the last message cell 10's loop looks at), the device rasterises all windows of all files in one launch
(``ops.piano_roll_windows``) and the result stays there; ``batches`` hands out views of it.  ``to_pickle`` writes the
reference's file, ``MaestroDatasetPickle`` reads one, ``MaestroDatasetTorch`` / ``write_torch_files`` are the per-file
``.pt`` route of notebook cell 9.

``InputSong`` reads a WAV file (``util.load_wav``, host), uploads its sample bytes once and computes the mel-dB windows
of the whole song on the device straight from them (``util.melspectrogram_db_from_pcm``): the decoded, overlapping
float windows the reference keeps in ``self.audio_files`` are never built.

``MaestroDataset`` is model 1's default data path upstream: a MIDI file of MAESTRO rendered to audio, cut into 5 s
windows, at most ``k`` of them kept, their mel-dB tensors stacked.  Upstream renders through FluidSynth and a WAV file
on disk; here the host turns the file into a note list in samples (``midi_notes``: exact integer time, FIFO pairing, the
sustain pedal) and the device renders only the chosen windows with the package's integer synth -- the renderer of the DES
bridge's fakes, so reals and fakes of a training run share one -- straight into the buffer the mel chain reads
(``ops.synth_windows``, ``util.melspectrogram_db_from_synth_windows``).  Nothing is written to disk; ``midi_to_wav``
writes the audio for whoever wants to hear it.  FluidSynth's sound font is not imitated: PARITY UNPINNED, as for the
bridge (include/gdm.h defines the synth and the MIDI rules).
"""
import collections
import glob
import json
import os
import pickle
import random
import struct

import numpy as np
import torch

from . import ops, util

DEFAULT_TEMPO = 500000
_K_OTHER, _K_ON, _K_OFF, _K_TEMPO, _K_TSIG, _K_EOT = 0, 1, 2, 3, 4, 5
_DATA_BYTES = {0x8: 2, 0x9: 2, 0xA: 2, 0xB: 2, 0xC: 1, 0xD: 1, 0xE: 2}
_SYS_BYTES = {0xF1: 1, 0xF2: 2, 0xF3: 1}


class MidiData:
    """Messages of all tracks as parallel arrays: absolute tick, track index, kind, two data values, and ``status``:
    the status byte of a channel or system message (running status resolved), 0xFF for a meta event, 0xF0 / 0xF7 for a
    system exclusive one (None if the producer did not record it)."""

    def __init__(self, fmt, ticks_per_beat, tick, track, kind, a, b, status=None):
        self.format, self.ticks_per_beat = fmt, ticks_per_beat
        self.tick, self.track, self.kind, self.a, self.b = tick, track, kind, a, b
        self.status = status


def read_midi(path_or_bytes):
    """Parse a Standard MIDI File (format 0/1; metrical time division) into a MidiData."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    if len(data) < 14 or data[:4] != b"MThd":
        raise ValueError("not a Standard MIDI File")
    hlen, fmt, ntrks, division = struct.unpack(">IHHH", data[4:14])
    if division & 0x8000:
        raise ValueError("SMPTE time division is not supported")
    pos = 8 + hlen
    tick, track, kind, av, bv, sv = [], [], [], [], [], []
    n_tr = 0
    while pos + 8 <= len(data) and n_tr < ntrks:
        tag = data[pos:pos + 4]
        size = struct.unpack(">I", data[pos + 4:pos + 8])[0]
        pos += 8
        end = min(pos + size, len(data))
        if tag != b"MTrk":
            pos = end
            continue
        now, status = 0, 0
        while pos < end:
            delta = 0
            while True:                                       # variable-length quantity
                byte = data[pos]
                pos += 1
                delta = (delta << 7) | (byte & 0x7F)
                if byte < 0x80:
                    break
            now += delta
            lead = data[pos]
            k, a, b, st = _K_OTHER, 0, 0, lead
            if lead == 0xFF:                                  # meta event: type, length, body
                mtype = data[pos + 1]
                pos += 2
                n = 0
                while True:
                    byte = data[pos]
                    pos += 1
                    n = (n << 7) | (byte & 0x7F)
                    if byte < 0x80:
                        break
                body = data[pos:pos + n]
                pos += n
                if mtype == 0x51 and n == 3:
                    k, a = _K_TEMPO, int.from_bytes(body, "big")
                elif mtype == 0x58 and n >= 2:
                    k, a, b = _K_TSIG, body[0], 1 << body[1]
                elif mtype == 0x2F:
                    k = _K_EOT
            elif lead in (0xF0, 0xF7):                        # system exclusive: length, body
                pos += 1
                n = 0
                while True:
                    byte = data[pos]
                    pos += 1
                    n = (n << 7) | (byte & 0x7F)
                    if byte < 0x80:
                        break
                pos += n
                status = 0
            else:
                if lead & 0x80:
                    status = lead
                    pos += 1
                elif not status:
                    raise ValueError("MIDI data byte without a running status")
                st = status
                if status >= 0xF0:
                    pos += _SYS_BYTES.get(status, 0)
                else:
                    nd = _DATA_BYTES[status >> 4]
                    a = data[pos]
                    b = data[pos + 1] if nd == 2 else 0
                    pos += nd
                    if status >> 4 == 0x9:
                        k = _K_ON                             # velocity 0 stays a note_on (as in mido)
                    elif status >> 4 == 0x8:
                        k = _K_OFF
            tick.append(now)
            track.append(n_tr)
            kind.append(k)
            av.append(a)
            bv.append(b)
            sv.append(st)
        pos = end
        n_tr += 1
    return MidiData(fmt, division, np.asarray(tick, dtype=np.int64), np.asarray(track, dtype=np.int32),
                    np.asarray(kind, dtype=np.int8), np.asarray(av, dtype=np.int64), np.asarray(bv, dtype=np.int64),
                    np.asarray(sv, dtype=np.uint8))


def message_seconds(md):
    """The stream ``for msg in mido.MidiFile(...)`` yields, as arrays: (delta seconds, kind, a, b) per message, tracks
    merged by absolute tick (stable: track order breaks ties), end_of_track messages dropped with their delta carried
    to the next message, each delta converted with the tempo in force before the message."""
    if md.format == 2:
        raise TypeError("can't merge tracks in type 2 (asynchronous) file")
    order = np.argsort(md.tick, kind="stable")                 # arrays are track-major already
    tick, kind, a, b = md.tick[order], md.kind[order], md.a[order], md.b[order]
    keep = kind != _K_EOT
    tick_k, kind_k, a_k, b_k = tick[keep], kind[keep], a[keep], b[keep]
    # dropping end_of_track and carrying its delta == deltas between the KEPT messages' absolute ticks
    dticks = np.diff(tick_k, prepend=0)
    tempo = np.full(len(tick_k), DEFAULT_TEMPO, dtype=np.int64)
    is_t = np.flatnonzero(kind_k == _K_TEMPO)
    for j, idx in enumerate(is_t):                             # tempo applies to the messages AFTER the set_tempo
        nxt = is_t[j + 1] + 1 if j + 1 < len(is_t) else len(tick_k)
        tempo[idx + 1:nxt] = a_k[idx]
    secs = np.where(dticks > 0, dticks * (tempo * 1e-6 / md.ticks_per_beat), 0.0)     # mido.tick2second's association
    return secs, kind_k, a_k, b_k


def _row_events(md, sequence_length, width):
    """Note messages the reference's loop processes, grouped by note: (row_ptr (129,), step, vel) as int32 arrays."""
    return _rows_of(message_seconds(md), sequence_length, width)


def _rows_of(stream, sequence_length, width):
    secs, kind, a, b = stream
    step = np.rint(np.cumsum(secs)).astype(np.int64)           # my_time += msg.time; int(round(my_time)) (half to even)
    stop = len(step)
    late = np.flatnonzero(step >= sequence_length)
    if len(late):
        stop = late[0]                                         # `break`
    wide = np.flatnonzero((kind == _K_ON) & (step >= width))
    if len(wide):
        stop = min(stop, wide[0])                              # piano_roll[note, step] raises: the bare except ends the loop
    sel = np.flatnonzero((kind[:stop] == _K_ON) | (kind[:stop] == _K_OFF))
    notes = a[sel]
    by_note = np.argsort(notes, kind="stable")                 # a note's messages stay in file order
    sel = sel[by_note]
    row_ptr = np.zeros(129, dtype=np.int32)
    np.cumsum(np.bincount(notes, minlength=128)[:128], out=row_ptr[1:])
    vel = np.where(kind[sel] == _K_ON, b[sel], -1).astype(np.int32)
    return row_ptr, step[sel].astype(np.int32), vel


def total_time_step(md, sample_size, stream=None):
    """``total_time`` of notebook cell 10's generate_piano_roll(midi, sample_size, ...): the rounded running time of the
    last message its loop looks at -- the one that triggers ``break`` included, so the value can reach or exceed
    ``sample_size`` -- over the stream mido yields, whose last message is ONE end_of_track carrying the deltas of all
    removed end_of_track messages behind the last kept message (``message_seconds`` drops it; its time is added here to
    the same float64 running sum, converted with the tempo then in force).  ``stream``: ``message_seconds(md)`` if the
    caller has it already."""
    secs, kind, a, _b = message_seconds(md) if stream is None else stream
    carry, tempo = 0, DEFAULT_TEMPO
    if len(md.tick):
        kept = md.tick[md.kind != _K_EOT]
        carry = int(md.tick.max()) - (int(kept.max()) if len(kept) else 0)
    is_t = np.flatnonzero(kind == _K_TEMPO)
    if len(is_t):
        tempo = int(a[is_t[-1]])
    last = carry * (tempo * 1e-6 / md.ticks_per_beat) if carry > 0 else 0.0     # mido.tick2second's association
    step = np.rint(np.cumsum(np.append(secs, last))).astype(np.int64)           # int(round(my_time)): half to even
    late = np.flatnonzero(step >= sample_size)
    return int(step[late[0]] if len(late) else step[-1])


def window_plan(midi_input, sample_size=300, sequence_length=50):
    """What notebook cell 11 keeps of one file: (total_time, kept window indices (int64 array), row events).

    ``nw = total_time // sequence_length`` windows are looked at; window i is kept iff ``1 <= i < nw`` (upstream's
    ``i != 0``) and ``(i + 1) * sequence_length <= sample_size`` (upstream's shape check on a slice of the
    ``sample_size`` wide plane): ``max(0, min(nw, sample_size // sequence_length) - 1)`` windows, contiguous from 1.
    The row events are ``_row_events(md, sample_size, sample_size)``, the CSR the raster kernels take."""
    if sequence_length <= 0 or sample_size <= 0:
        raise ValueError(f"sample_size={sample_size} and sequence_length={sequence_length} must be positive")
    md = midi_input if isinstance(midi_input, MidiData) else read_midi(midi_input)
    stream = message_seconds(md)
    total_time = total_time_step(md, sample_size, stream)
    nw = total_time // sequence_length
    kept = np.arange(1, max(1, min(nw, sample_size // sequence_length)), dtype=np.int64)
    return total_time, kept, _rows_of(stream, sample_size, sample_size)


def _qpm_to_bpm(qpm, num, den):
    """pretty_midi.utilities.qpm_to_bpm."""
    if den in (1, 2, 4):
        return qpm * den / 4.0
    if den in (8, 16, 32):
        scale = den / 4.0
        if num == 3:
            return scale * qpm
        if num % 3 == 0:
            return scale * qpm / 3.0
        return scale * qpm
    return qpm


def get_beats(md, start_time=0.0):
    """Beat times as pretty_midi.PrettyMIDI.get_beats computes them (restated): 60 / bpm apart from start_time to the end
    of the last note, bpm from the tempo map and the time signature's denominator, re-anchored at tempo and time-signature
    changes."""
    order = np.argsort(md.tick, kind="stable")
    tick, kind, a, b = md.tick[order], md.kind[order], md.a[order], md.b[order]
    t_ticks, t_us = [0], [DEFAULT_TEMPO]
    for tk, us in zip(tick[kind == _K_TEMPO], a[kind == _K_TEMPO]):
        if tk == 0:
            t_us[0] = int(us)
        elif int(us) != t_us[-1]:
            t_ticks.append(int(tk))
            t_us.append(int(us))
    scales = np.asarray(t_us, dtype=np.float64) * 1e-6 / md.ticks_per_beat
    seg_start = np.concatenate([[0.0], np.cumsum(np.diff(t_ticks) * scales[:-1])])

    def tick_time(tk):
        seg = np.searchsorted(t_ticks, tk, side="left") - 1
        seg = np.clip(seg, 0, len(t_ticks) - 1)
        return seg_start[seg] + (tk - np.asarray(t_ticks)[seg]) * scales[seg]

    tempo_times = seg_start
    tempi = 60.0 / (np.asarray(t_us, dtype=np.float64) * 1e-6)
    ts_mask = kind == _K_TSIG
    ts = sorted(zip(tick_time(tick[ts_mask]).tolist(), a[ts_mask].tolist(), b[ts_mask].tolist()))
    ends = tick[(kind == _K_OFF) | ((kind == _K_ON) & (b == 0))]
    end_time = float(tick_time(ends).max()) if len(ends) else 0.0
    beats = [start_time]
    ti = si = 0
    while ti < len(tempo_times) - 1 and beats[-1] > tempo_times[ti + 1]:
        ti += 1
    while si < len(ts) - 1 and beats[-1] >= ts[si + 1][0]:
        si += 1
    while beats[-1] < end_time:
        bpm = _qpm_to_bpm(tempi[ti], ts[si][1], ts[si][2]) if ts else tempi[ti]
        nxt = beats[-1] + 60.0 / bpm
        if ti < len(tempo_times) - 1 and nxt > tempo_times[ti + 1]:
            nxt, left = beats[-1], 1.0
            while ti < len(tempo_times) - 1 and nxt + left * 60.0 / bpm >= tempo_times[ti + 1]:
                part = (tempo_times[ti + 1] - nxt) / (60.0 / bpm)
                nxt += part * 60.0 / bpm
                left -= part
                ti += 1
                bpm = _qpm_to_bpm(tempi[ti], ts[si][1], ts[si][2]) if ts else tempi[ti]
            nxt += left * 60.0 / bpm
        if ts and si < len(ts) - 1 and (nxt > ts[si + 1][0] or np.isclose(nxt, ts[si + 1][0])):
            nxt = ts[si + 1][0]
            si += 1
        beats.append(nxt)
    return np.asarray(beats[:-1])


def _fit_beats(beats, beats_length):
    if len(beats) < beats_length:
        return np.pad(beats, (0, beats_length - len(beats)))
    return beats[:beats_length]


def generate_piano_rolls(midi_inputs, sequence_length=100, beats_length=50, start=0, end=50, device="cuda"):
    """Batched generate_piano_roll: list of paths (or bytes) -> (piano_roll, durations (F,128,W) fp32, beats
    (F,beats_length) fp32) on ``device``; W = what the reference's final slice leaves."""
    if sequence_length is None:
        sequence_length = end + 20
    width = end - start
    if width <= 0:
        raise ValueError("negative dimensions are not allowed")       # np.zeros((128, end - start)) upstream
    ptrs, steps, vels, beats = [np.zeros(1, dtype=np.int32)], [], [], []
    total = 0
    for item in midi_inputs:
        md = item if isinstance(item, MidiData) else read_midi(item)
        rp, st, ve = _row_events(md, sequence_length, width)
        ptrs.append(rp[1:] + total)
        total += int(rp[-1])
        steps.append(st)
        vels.append(ve)
        beats.append(_fit_beats(get_beats(md), beats_length))
    dev = torch.device(device)
    row_ptr = torch.from_numpy(np.concatenate(ptrs)).to(dev)
    ev_step = torch.from_numpy(np.concatenate(steps) if steps else np.zeros(0, np.int32)).to(dev)
    ev_vel = torch.from_numpy(np.concatenate(vels) if vels else np.zeros(0, np.int32)).to(dev)
    roll, dur = ops.piano_roll_raster(row_ptr, ev_step, ev_vel, len(beats), width)
    # `if end < len(piano_roll)` compares with 128 rows; both branches slice the (128, end - start) planes
    sl = slice(start, end) if end < 128 else slice(0, end)
    return roll[:, :, sl], dur[:, :, sl], torch.from_numpy(np.stack(beats)).float().to(dev)


def generate_piano_roll(midi_input, sequence_length=100, beats_length=50, start=0, end=50, device="cuda"):
    """Reference signature; returns numpy (piano_roll, durations, beats) like upstream (float64 planes)."""
    if not isinstance(midi_input, (str, os.PathLike, bytes, bytearray, MidiData)):
        raise ValueError("midi_input must be a file path or a mido.MidiFile object")
    roll, dur, beats = generate_piano_rolls([midi_input], sequence_length, beats_length, start, end, device)
    return (roll[0].double().cpu().numpy(), dur[0].double().cpu().numpy(),
            _fit_beats(get_beats(midi_input if isinstance(midi_input, MidiData) else read_midi(midi_input)),
                       beats_length))


class MaestroDatasetMidi(torch.utils.data.Dataset):
    """Raw-MIDI dataset of the reference (datasets.py:103-123): item = (piano_roll, durations (128,W), beats) fp32
    tensors on ``device``; ``pattern`` replaces the hard-wired Windows glob."""

    def __init__(self, root_dir, sequence_length=100, beats_length=50, device="cuda", pattern="**/*.mid*"):
        self.root_dir, self.sequence_length, self.beats_length, self.device = root_dir, sequence_length, beats_length, device
        self.file_list = sorted(glob.glob(os.path.join(root_dir, pattern), recursive=True))

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        roll, dur, beats = generate_piano_rolls([self.file_list[idx]], self.sequence_length, self.beats_length,
                                                device=self.device)
        return roll[0], dur[0], beats[0]


class _Batches:
    """One epoch per ``iter()``: (piano_roll, durations, beats) batches of a resident dataset."""

    def __init__(self, tensors, batch_size, drop_last, shuffle, generator):
        if batch_size <= 0:
            raise ValueError(f"batch_size={batch_size} must be positive")
        self.tensors, self.batch_size, self.drop_last = tensors, int(batch_size), drop_last
        self.shuffle, self.generator = shuffle, generator

    def __len__(self):
        n = len(self.tensors[0])
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        b = self.batch_size
        if not self.shuffle:
            for k in range(len(self)):                              # slices of the resident tensors: views, no copy
                yield tuple(t[k * b:(k + 1) * b] for t in self.tensors)
            return
        perm = torch.randperm(len(self.tensors[0]), generator=self.generator)      # host, as DataLoader's sampler
        perm = perm.to(self.tensors[0].device)
        for k in range(len(self)):
            idx = perm[k * b:(k + 1) * b]
            yield tuple(t.index_select(0, idx) for t in self.tensors)


class _ResidentWindows(torch.utils.data.Dataset):
    """piano_roll, durations (N,128,L) and beats (N,beats_length) fp32 stacked on one device; items are views."""

    piano_roll = durations = beats = None

    def __len__(self):
        return self.piano_roll.shape[0]

    def __getitem__(self, idx):
        n = len(self)
        i = int(idx)
        if not -n <= i < n:
            raise IndexError(f"item {idx} of a dataset with {n}")
        return self.piano_roll[i], self.durations[i], self.beats[i]

    def batches(self, batch_size, drop_last=True, shuffle=False, generator=None):
        """Re-iterable over (piano_roll, durations, beats) batches, one epoch per ``iter()``.  Unshuffled, the batches
        are contiguous slices of the resident tensors (views, nothing copied) and equal what the reference's
        ``DataLoader(dataset, batch_size, drop_last=True)`` collates; shuffled, each epoch draws a permutation from
        ``generator`` and gathers with one ``index_select`` per tensor."""
        return _Batches((self.piano_roll, self.durations, self.beats), batch_size, drop_last, shuffle, generator)


class MaestroWindows(_ResidentWindows):
    """The training set of model 2 as data_viewing_and_processing.ipynb cell 11 builds it, resident on the device:
    ``piano_roll``, ``durations`` (N,128,L) and ``beats`` (N,beats_length) fp32; the host arrays ``file_index`` and
    ``window_index`` (int64) say which input file and which window of it item n is (window i = steps i*L .. (i+1)*L).
    ``beats`` holds the file's first ``beats_length`` beat times, zero-padded, the same row for all windows of a file.

    Memory: two (128, L) fp32 planes and a beats row per window -- 51 KB at L = 50, about 280 MB for MAESTRO's
    ~5.4 k windows (1 276 files, sample_size 300)."""

    def __init__(self, piano_roll, durations, beats, file_index, window_index, sample_size, files=None):
        self.piano_roll, self.durations, self.beats = piano_roll, durations, beats
        self.file_index = np.asarray(file_index, dtype=np.int64)
        self.window_index = np.asarray(window_index, dtype=np.int64)
        self.sample_size, self.sequence_length, self.beats_length = int(sample_size), piano_roll.shape[2], beats.shape[1]
        self.files = files
        self.device = piano_roll.device

    @classmethod
    def from_midi(cls, root_dir_or_list, sample_size=300, sequence_length=50, beats_length=50, device="cuda",
                  pattern="**/*.mid*"):
        """Parse the files (a directory searched with ``pattern``, or a list of paths / bytes / MidiData), upload the
        concatenated row events once and rasterise every kept window in one launch.  Files that yield no window
        contribute nothing; if none does, ValueError."""
        if sequence_length <= 0 or sample_size <= 0:
            raise ValueError(f"sample_size={sample_size} and sequence_length={sequence_length} must be positive")
        if isinstance(root_dir_or_list, (str, os.PathLike)):
            files = sorted(glob.glob(os.path.join(root_dir_or_list, pattern), recursive=True))
        else:
            files = list(root_dir_or_list)
        ptrs, steps, vels, beats = [np.zeros(1, dtype=np.int32)], [], [], []
        win_file, file_index, window_index = [], [], []
        total = 0
        for idx, item in enumerate(files):
            md = item if isinstance(item, MidiData) else read_midi(item)
            _total_time, kept, (rp, st, ve) = window_plan(md, sample_size, sequence_length)
            if not len(kept):
                continue
            win_file.append(np.full(len(kept), len(beats), dtype=np.int32))      # index among the uploaded files
            file_index.append(np.full(len(kept), idx, dtype=np.int64))
            window_index.append(kept)
            ptrs.append(rp[1:] + total)
            total += int(rp[-1])
            steps.append(st)
            vels.append(ve)
            beats.append(_fit_beats(get_beats(md), beats_length))
        if not beats:
            raise ValueError(f"none of the {len(files)} files read yields a window: a file needs "
                             f"2 * sequence_length = {2 * sequence_length} seconds (window 0 is dropped) within "
                             f"sample_size = {sample_size}")
        dev = torch.device(device)
        win_file, window_index = np.concatenate(win_file), np.concatenate(window_index)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        roll, dur = ops.piano_roll_windows(up(np.concatenate(ptrs)), up(np.concatenate(steps)), up(np.concatenate(vels)),
                                           up(win_file), up((window_index * sequence_length).astype(np.int32)),
                                           sequence_length)
        rows = up(np.stack(beats).astype(np.float32))
        return cls(roll, dur, rows.index_select(0, up(win_file.astype(np.int64))), np.concatenate(file_index),
                   window_index, sample_size, files=[f for f in files if isinstance(f, (str, os.PathLike))] or None)

    def save(self, path):
        """Plain tensors (torch.save); ``load`` reads them back with ``weights_only=True``."""
        torch.save({"piano_roll": self.piano_roll.cpu(), "durations": self.durations.cpu(), "beats": self.beats.cpu(),
                    "file_index": torch.from_numpy(self.file_index), "window_index": torch.from_numpy(self.window_index),
                    "sample_size": torch.tensor(self.sample_size)}, path)

    @classmethod
    def load(cls, path, device="cuda"):
        d = torch.load(path, map_location="cpu", weights_only=True)
        dev = torch.device(device)
        return cls(d["piano_roll"].to(dev), d["durations"].to(dev), d["beats"].to(dev), d["file_index"].numpy(),
                   d["window_index"].numpy(), int(d["sample_size"]))

    def to_pickle(self, path):
        """The reference's ``preprocessed_data_{L}.pkl`` (notebook cell 11): a pickled list of (piano_roll, durations,
        beats) CPU float32 tensors, readable by the reference's own MaestroDatasetPickle."""
        roll, dur, beats = self.piano_roll.cpu(), self.durations.cpu(), self.beats.cpu()
        data = [(roll[i].clone(), dur[i].clone(), beats[i].clone()) for i in range(len(self))]
        with open(path, "wb") as f:
            pickle.dump(data, f)


class MaestroDatasetPickle(_ResidentWindows):
    """The reference's pickle dataset (datasets.py:73-87): ``data_dir/pickle_file_name`` holds the list of (piano_roll,
    durations, beats) tensors notebook cell 11 (or ``MaestroWindows.to_pickle``) writes; ``data_dir`` replaces the
    hard-wired ``'data\\'``.  The list is stacked once onto ``device`` and items are views of it; ``sequence_length``
    and ``beats_length`` are stored and otherwise unused, as upstream.  Works on the CPU and launches nothing.

    The file is read with ``pickle.load``, as upstream reads it: unpickling runs code the file names, so open only files
    you trust (``MaestroWindows.save`` / ``load`` is the format without that property)."""

    def __init__(self, pickle_file_name, sequence_length=100, beats_length=50, device="cpu", *, data_dir="data"):
        self.sequence_length, self.beats_length, self.device = sequence_length, beats_length, torch.device(device)
        with open(os.path.join(data_dir, pickle_file_name), "rb") as f:
            data = pickle.load(f)
        if not data:
            raise ValueError(f"{pickle_file_name} holds no item")
        self.piano_roll, self.durations, self.beats = (
            torch.stack([torch.as_tensor(item[k]) for item in data]).float().to(self.device) for k in range(3))


class MaestroDatasetTorch(torch.utils.data.Dataset):
    """The reference's per-file tensor dataset (datasets.py:90-100): item = ``torch.load`` of the (piano_roll,
    durations, beats) tuple notebook cell 9 (or ``write_torch_files``) saved for one MIDI file, moved to ``device``;
    ``pattern`` under ``root_dir`` replaces the hard-wired ``'data\\tensors\\*.pt'``."""

    def __init__(self, root_dir, sequence_length=100, beats_length=50, device="cpu", *, pattern="*.pt"):
        self.data_dir, self.sequence_length, self.beats_length, self.device = root_dir, sequence_length, beats_length, device
        self.file_list = sorted(glob.glob(os.path.join(root_dir, pattern)))

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        return tuple(t.to(self.device) for t in torch.load(self.file_list[idx], map_location="cpu", weights_only=True))


def write_torch_files(midi_inputs, out_dir, sequence_length=100, beats_length=50, start=0, end=50, device="cuda"):
    """Notebook cell 9: one ``data_{idx}.pt`` per MIDI file holding its (piano_roll, durations, beats) CPU float32
    tuple, all files rasterised by one ``generate_piano_rolls`` launch.  Returns the paths written."""
    midi_inputs = list(midi_inputs)
    roll, dur, beats = (t.cpu() for t in generate_piano_rolls(midi_inputs, sequence_length, beats_length, start, end,
                                                              device))
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for idx in range(len(midi_inputs)):
        paths.append(os.path.join(out_dir, f"data_{idx}.pt"))
        torch.save((roll[idx].clone(), dur[idx].clone(), beats[idx].clone()), paths[-1])
    return paths


class InputSong(torch.utils.data.Dataset):
    """One song cut into excerpts (GAN_DES/datasets.py:17-52): item i = the (128, frames) mel-dB tensor of window i, on
    ``device``.  As upstream, windows are ``hop_length_audio`` seconds long and apart (``window_size`` is stored and
    otherwise unused), the last one is taken from the end of the song, channel 0 is used and the file's sample rate
    goes to the filter bank (``util.song_windows`` lists the consequences).

    All windows are computed on first use, ``windows_per_chunk`` at a time so that the frame matrix of a long song stays
    bounded (64 windows of 216 frames x 2048 samples are 113 MB), and kept; items are views of that tensor."""

    def __init__(self, audio_file, window_size=5, hop_length_audio=5, *, device="cuda", windows_per_chunk=64):
        self._wav = util.load_wav(audio_file)
        self.sample_rate = self._wav.sample_rate
        self.audio_file_length = self._wav.n_frames / self.sample_rate
        self.window_size = window_size
        self.hop_length_audio = hop_length_audio
        self.device = torch.device(device)
        self.windows_per_chunk = max(1, int(windows_per_chunk))
        self.windows = util.song_windows(self._wav.n_frames, self.sample_rate, hop_length_audio, window_size,
                                         mode="input_song")
        self._pcm = util.upload_pcm(self._wav, self.device)
        self._spec = self._orig = None

    @property
    def orig_waveform(self):
        """(channels, n) fp32 on the device, what torchaudio.load(normalize=True) returns; decoded on first use."""
        if self._orig is None:
            w = self._wav
            self._orig = torch.empty((w.channels, w.n_frames), dtype=torch.float32, device=self.device)
            for c in range(w.channels):
                ops.pcm_to_float(self._pcm, w.fmt, w.channels, c, w.n_frames, out=self._orig[c])
        return self._orig

    def spectrograms(self):
        """(len(self), 128, frames) fp32 on the device: every window's mel-dB tensor (computed once)."""
        if self._spec is None:
            length = self.windows[0][1]                                # one length for all windows of a song
            hop, win_len = util.mel_geometry(length)
            starts = [s for s, _ in self.windows]
            k = self.windows_per_chunk
            parts = [util.melspectrogram_db_from_pcm(self._pcm, self._wav, 0, starts[a:a + k], win_len,
                                                     sr=self.sample_rate, hop=hop)
                     for a in range(0, len(starts), k)]
            self._spec = parts[0] if len(parts) == 1 else torch.cat(parts)
        return self._spec

    def __len__(self):
        return len(self.windows)

    def __getitem__(self, item):
        n = len(self.windows)
        i = int(item)
        if not -n <= i < n:
            raise IndexError(f"window {item} of a song with {n}")
        return self.spectrograms()[i]


# ---- model 1's MAESTRO route: MIDI file -> notes in samples -> windows of the integer synth -> mel dB ------------------
MAX_CLIP_SAMPLES = 1 << 40          # the synth's sample range (gdm_synth_pcm, GDM_DES_NOTES_ELONG)
MAX_CLIP_NOTES = 1 << 18            # the kernel's int32 voice sum is proven below that: 2^18 * 8128 < 2^31


def midi_notes(midi_input, *, pedal=True, programs=False):
    """A Standard MIDI File (path, bytes or MidiData) -> (notes (n, 4) int64, clip_len): rows (s_on, s_off, pitch,
    velocity) IN SAMPLES at 44 100 Hz, sorted by s_on (stable), as ``ops.synth_windows`` takes them.  The rules are
    defined here and in include/gdm.h, as the synth is:

    Time.  Tracks are merged as in ``message_seconds`` (stable by absolute tick; a tempo applies to the messages after
    its set_tempo, 500 000 before the first).  With U = the running sum of delta_ticks * tempo in force, a message
    sounds at sample ``U * 441 // (ticks_per_beat * 10000)``: Python integers, no float anywhere.  At tempo 1 000 000
    and 480 ticks per beat -- the bridge's own files -- that is ``(tick * 735) >> 3``.  ValueError if U * 441 reaches
    2^63.
    Pairing.  A note_on with velocity > 0 opens a note on its (channel, pitch); a note_off, or a note_on with velocity
    0, closes the OLDEST open note of that (channel, pitch); a close without an open note is ignored; notes still open
    at the end close at the file's last message (the latest end_of_track counts as one).
    Sustain pedal (controller 64 per channel, value >= 64 = down).  A close that arrives while the pedal is down is
    deferred: the note ends at the earliest of the pedal's release on its channel, the next note_on of its (channel,
    pitch), and the file's last message.  ``pedal=False`` ignores controller 64.
    All channels sound the same voice, program changes are ignored, pitch and velocity are kept as stored (0..127).
    clip_len = max(s_off) + the synth's release (8192), or 5 * 44100 for a file without notes (the bridge's blank clip).
    ValueError for a clip beyond 2^40 samples and for 2^18 notes or more.
    ``programs=True`` adds a fifth column: the program in force on the note's channel at its note_on (0 before the
    channel's first program_change) -- the rows ``ops.synth_windows_gm`` takes; everything else is unchanged."""
    md = midi_input if isinstance(midi_input, MidiData) else read_midi(midi_input)
    if md.format == 2:
        raise TypeError("can't merge tracks in type 2 (asynchronous) file")
    if md.status is None:
        raise ValueError("midi_notes needs MidiData.status (read_midi records it)")
    order = np.argsort(md.tick, kind="stable")
    ticks, kinds = md.tick[order].tolist(), md.kind[order].tolist()
    av, bv, sv = md.a[order].tolist(), md.b[order].tolist(), md.status[order].tolist()
    den = md.ticks_per_beat * 10000
    if den <= 0:
        raise ValueError("ticks_per_beat must be positive")
    rows = []                                            # [s_on, s_off or None, pitch, velocity] in note_on order
    open_rows = collections.defaultdict(collections.deque)      # (channel, pitch) -> rows waiting for their close
    held = collections.defaultdict(list)                 # channel -> rows whose close the pedal defers
    down = [False] * 16
    program = [0] * 16
    u = prev = s = 0
    tempo = DEFAULT_TEMPO
    for tk, k, a, b, st in zip(ticks, kinds, av, bv, sv):
        u += (tk - prev) * tempo
        prev = tk
        if u * 441 >= 1 << 63:
            raise ValueError("the file's running time passes 2^63 / 441 us * ticks per beat")
        s = u * 441 // den
        if k == _K_TEMPO:
            tempo = a
        elif k == _K_ON and b > 0:
            ch = st & 15
            if held[ch]:                                 # the key is struck again: its held notes end here
                for r in held[ch]:
                    if r[2] == a:
                        r[1] = s
                held[ch] = [r for r in held[ch] if r[2] != a]
            rows.append([s, None, a, b, program[ch]] if programs else [s, None, a, b])
            open_rows[ch, a].append(rows[-1])
        elif k in (_K_ON, _K_OFF):
            ch = st & 15
            if open_rows[ch, a]:
                r = open_rows[ch, a].popleft()
                if down[ch]:
                    held[ch].append(r)
                else:
                    r[1] = s
        elif programs and st >> 4 == 0xC:
            program[st & 15] = a
        elif pedal and st >> 4 == 0xB and a == 64:
            ch = st & 15
            down[ch] = b >= 64
            if not down[ch]:
                for r in held[ch]:
                    r[1] = s
                held[ch] = []
    for r in rows:                                       # open or held at the end: the file's last message
        if r[1] is None:
            r[1] = s
    if len(rows) >= MAX_CLIP_NOTES:
        raise ValueError(f"{len(rows)} notes in one file (fewer than 2^18 keep the synth's int32 voice sum exact)")
    if not rows:
        return np.zeros((0, 5 if programs else 4), dtype=np.int64), 5 * ops.SYNTH_RATE
    clip_len = max(r[1] for r in rows) + ops.SYNTH_RELEASE
    if clip_len > MAX_CLIP_SAMPLES:
        raise ValueError(f"a clip of {clip_len} samples (2^40 at most)")
    notes = np.asarray(rows, dtype=np.int64)
    return notes[np.argsort(notes[:, 0], kind="stable")], int(clip_len)


def running_off_max(notes):
    """The ``off_max`` column of ``ops.synth_windows`` for ONE clip's rows: the running maximum of s_off."""
    return np.maximum.accumulate(np.asarray(notes, dtype=np.int64).reshape(-1, 4)[:, 1])


def _upload_clips(clips, device):
    """[(n_i, 4) note rows] -> (notes, off_max, note_ptr) device tensors of ``ops.synth_windows``."""
    notes = np.concatenate([c.reshape(-1, 4) for c in clips]) if clips else np.zeros((0, 4), np.int64)
    off_max = np.concatenate([running_off_max(c) for c in clips]) if clips else np.zeros(0, np.int64)
    note_ptr = np.zeros(len(clips) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clips], out=note_ptr[1:])
    dev = torch.device(device)
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(dev) for x in (notes, off_max, note_ptr))


def midi_to_wav(midi_input, wav_path, *, pedal=True, max_seconds=None, device="cuda"):
    """Stands where ``FluidSynth.midi_to_audio`` stands upstream (GAN_DES/datasets.py:82): the whole clip of
    ``midi_notes`` as a mono 16-bit 44 100 Hz WAV file, rendered by the integer synth in bounded chunks (one
    ``ops.synth_windows`` window of 2^22 samples per launch); ``max_seconds`` cuts it.  Returns the samples written."""
    notes, clip_len = midi_notes(midi_input, pedal=pedal)
    rows, off_max, note_ptr = _upload_clips([notes], device)
    win_clip = torch.zeros(1, dtype=torch.int32, device=rows.device)

    def render(first, count):
        start = torch.full((1,), first, dtype=torch.int64, device=rows.device)
        return ops.synth_windows(rows, off_max, note_ptr, win_clip, start, count)[0, :count]
    return util.write_wav_chunks(wav_path, clip_len, render, max_seconds=max_seconds)


def choose_windows(n, k):
    """Which of a file's n windows an item keeps: all of them, or -- if there are more than k -- the k that upstream's
    ``random.sample(splits, k)`` picks, in its order.  Sampling positions instead of the list draws the same numbers
    from Python's global ``random`` stream and leaves it in the same state."""
    return random.sample(range(n), k) if n > k else list(range(n))


class MaestroDataset(torch.utils.data.Dataset):
    """The reference's MAESTRO dataset (GAN_DES/datasets.py:55-100): item ``index`` = the (n, 128, 216) fp32 mel-dB
    tensor, on ``device``, of at most ``k = batch_size`` five-second windows of MIDI file ``data[str(index)]`` of the
    metadata JSON (``meta_data_file``, default ``{input_folder}/maestro-v3.0.0.json``).  ``INPUT_FOLDER``,
    ``meta_data_file``, ``k`` and ``data`` are upstream's attributes; ``input_folder`` replaces the hard-wired path.

    Per item: ``midi_notes`` on the file, ``util.song_windows(clip_len, 44100, 5, 5, mode="split")`` (upstream's
    split_audio_data: the last window twice when the length is a multiple of five seconds, one short window for a clip
    under five seconds), ``choose_windows``, then one synth launch for the chosen windows only and the mel chain of the
    WAV route.  The audio is the package's integer synth, not FluidSynth's sound font (see the module docstring).
    Use ``num_workers=0`` in a DataLoader: the items are device tensors."""

    def __init__(self, batch_size, *, input_folder="../data/maestro-v3.0.0", meta_data_file=None, device="cuda",
                 pedal=True, windows_per_chunk=64):
        self.INPUT_FOLDER = input_folder
        self.meta_data_file = meta_data_file if meta_data_file is not None else f"{input_folder}/maestro-v3.0.0.json"
        self.k = batch_size
        self.device, self.pedal = torch.device(device), pedal
        self.windows_per_chunk = max(1, int(windows_per_chunk))
        with open(self.meta_data_file) as json_file:
            self.data = json.load(json_file)["midi_filename"]

    def __len__(self):
        return len(self.data)

    def plan(self, index):
        """(note rows, [(start, length) of the windows item ``index`` keeps]); draws from ``random`` as the item does."""
        notes, clip_len = midi_notes(f"{self.INPUT_FOLDER}/{self.data[str(index)]}", pedal=self.pedal)
        windows = util.song_windows(clip_len, ops.SYNTH_RATE, 5, 5, mode="split")
        return notes, [windows[i] for i in choose_windows(len(windows), self.k)]

    def spectrograms(self, indices=None):
        """The items of ``indices`` (default: every file) concatenated -- what ``my_collate`` builds of them -- with ONE
        synth launch for all windows of all files; the windows are drawn per file, in order."""
        indices = range(len(self)) if indices is None else indices
        plans = [self.plan(int(i)) for i in indices]
        if not plans:
            raise ValueError("spectrograms() of no file")
        lengths = [length for _notes, wins in plans for _start, length in wins]
        win_clip = np.concatenate([np.full(len(wins), c, dtype=np.int32) for c, (_n, wins) in enumerate(plans)])
        win_start = np.asarray([start for _notes, wins in plans for start, _length in wins], dtype=np.int64)
        rows, off_max, note_ptr = _upload_clips([notes for notes, _wins in plans], self.device)
        # one launch renders every window at the longest length: what a shorter clip has beyond its end is silence
        pcm = ops.synth_windows(rows, off_max, note_ptr, torch.from_numpy(win_clip).to(self.device),
                                torch.from_numpy(win_start).to(self.device), max(lengths))
        parts, a = [], 0
        while a < len(lengths):                          # runs of one window length, bounded for the frame matrix
            b = a + 1
            while b < len(lengths) and lengths[b] == lengths[a] and b - a < self.windows_per_chunk:
                b += 1
            parts.append(util.melspectrogram_db_from_synth_windows(pcm[a:b], b - a, lengths[a], pcm.shape[1]))
            a = b
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def __getitem__(self, index):
        return self.spectrograms([index])


def my_collate(batch):
    """The reference's collate function (GAN_DES/datasets.py:94-100): items of different window counts, concatenated."""
    return torch.cat(batch)
