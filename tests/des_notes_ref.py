"""Plain-Python / numpy restatement of model 1's DES bridge -- TEST INFRASTRUCTURE ONLY.

Stage A (csrc/des_notes.hip): the reader of process_adjsim_log and MidiGenerator.process_line of the reference's
GAN_DES/sim_log_process_music.py:65-133,159-185 over EVENT_DTYPE-like records -> the (type, note, velocity, time) rows
the reference appends to its track, and the note list (on_tick, off_tick, pitch, velocity) cut from them.  Pinned by
tests/golden/des_notes.npz (rows recorded from the reference's own MidiGenerator).

Stages B and C (csrc/synth.hip): the integer synth defined in include/gdm.h, evaluated per sample, as the (216, 2048)
frame matrix of the mel featuriser and as 16-bit PCM.  Nothing upstream pins it (the reference renders through
FluidSynth and a sound font); the package defines it, and the kernels are held to this mirror bit for bit.
"""
import struct

import numpy as np

ARRIVAL, DEPARTURE = 0, 1
MAX_LINES = 5000
NOTE_ON, NOTE_OFF = 0, 1                    # row types of the fixture
OK, ENODE, EPITCH, ELONG = 0, 1, 2, 3       # GDM_DES_NOTES_E*
# synth constants (include/gdm.h: GDM_SYNTH_*)
ATTACK, RELEASE, SHIFT = 256, 8192, 30
WAVE_LEN, FRAMES, N_FFT, RATE = 2048, 216, 2048, 44100
MAX_SAMPLES = 1 << 40
MAX_TICK = ((MAX_SAMPLES - RELEASE) << 3) // 735        # the last tick whose sample + RELEASE stays within 2^40
FAULTS = ("fold_boundary", "c_modulo", "clear_future", "read_5001")


class LogError(ValueError):
    """What escapes from the reference's MidiGenerator (KeyError for a node without note level, mido's ValueError)."""


def line_matches(value, event_id, node, kind):
    """Does the reference's regex match ``INFO:root:{value!r} - {event_id} - {node} - {kind name}``?  'processing' is
    not in its alternation; a float's repr is plain digits iff it is +0.0 or in [1e-4, 1e16)."""
    value = float(value)
    if kind not in (ARRIVAL, DEPARTURE) or event_id < 0 or node < 0:
        return False
    if not np.isfinite(value) or np.signbit(value):
        return False
    return value == 0.0 or 1e-4 <= value < 1e16


def _c_mod(a, m):
    r = abs(a) % abs(m)
    return -r if a < 0 else r


def log_rows(log, note_levels, fault=None):
    """-> list of (type, note, velocity, time) as the reference's track receives them.  ``fault``: one of FAULTS plants
    a deliberate error (tests show that the fixture catches each); None is the reference's behaviour."""
    assert fault is None or fault in FAULTS
    notes = [int(x) for x in note_levels]
    value, event_id, node, kind = log["value"], log["event_id"], log["node"], log["kind"]
    n = min(len(value), MAX_LINES + (1 if fault == "read_5001" else 0))
    lo_fold = 126 if fault == "fold_boundary" else 127
    mod = _c_mod if fault == "c_modulo" else (lambda a, m: a % m)
    queue, future, rows = {}, {}, []
    for r in range(n):
        eid, nd, kd = int(event_id[r]), int(node[r]), int(kind[r])
        if not line_matches(value[r], eid, nd, kd):
            continue
        if not (eid % 3 == 0 or eid % 5 == 0 or eid % 7 == 0):
            continue
        midi_time = max(0, int(float(value[r])))
        if kd == ARRIVAL:
            q = queue[nd] = queue.get(nd, 0) + 1
            if lo_fold <= q < 254:
                q = min(127, max(0, 254 - q))
            elif q >= 254:
                q = min(127, max(0, q % 127))
            max_id = max(1, mod(30 + q, 127))
            cid = eid
            if max_id <= cid < 2 * max_id:
                cid = min(max_id, max(0, 2 * max_id - cid))
            elif cid >= 2 * max_id:
                cid = min(max_id, max(0, cid % max_id))
            future[nd] = (midi_time, 60 + cid % 67, q)
        else:
            if nd in future:
                t0, vel, service = future[nd]
                if not 0 <= nd < len(notes):
                    raise LogError(f"node {nd} has no note level")
                if not 0 <= notes[nd] <= 127:
                    raise LogError(f"note {notes[nd]} out of range")
                rows.append((NOTE_ON, notes[nd], vel, max(0, t0)))
                rows.append((NOTE_OFF, notes[nd], vel, max(0, t0 + (midi_time - t0) + max(0, service))))
                if fault == "clear_future":
                    del future[nd]
            queue[nd] = queue[nd] - 1 if nd in queue else 0
    return rows


def tick_to_sample(tick):
    """1 tick = 1/480 s (set_tempo 1 000 000, 480 ticks per beat) at 44 100 Hz: 91.875 samples."""
    return (int(tick) * 735) >> 3


def rows_to_notes(rows):
    """Rows (a strictly sequential note_on / note_off track, times = delta ticks) -> (notes (n, 4) int64 of (on_tick,
    off_tick, pitch, velocity), clip_len in samples, status).  An overlong clip is blank: no notes, length 0."""
    out, t = [], 0
    for k in range(0, len(rows), 2):
        on, off = rows[k], rows[k + 1]
        assert on[0] == NOTE_ON and off[0] == NOTE_OFF and on[1:3] == off[1:3]
        if on[3] > MAX_TICK - t:
            return np.zeros((0, 4), np.int64), 0, ELONG
        t += on[3]
        t_on = t
        if off[3] > MAX_TICK - t:
            return np.zeros((0, 4), np.int64), 0, ELONG
        t += off[3]
        out.append((t_on, t, on[1], on[2]))
    notes = np.asarray(out, dtype=np.int64).reshape(-1, 4)
    clip_len = tick_to_sample(notes[-1, 1]) + RELEASE if len(out) else 0
    return notes, clip_len, OK


def log_to_notes(log, note_levels):
    """Stage A for one sample -> (notes, clip_len, status); raises LogError where the reference would raise."""
    return rows_to_notes(log_rows(log, note_levels))


# ---- the synth -------------------------------------------------------------------------------------------------------
def tables():
    """(wave int16[2048], inc uint32[128]) as the host builds them, in float64."""
    i = np.arange(WAVE_LEN, dtype=np.float64)
    wave = np.round(32767.0 * np.sin(2.0 * np.pi * i / WAVE_LEN)).astype(np.int16)
    p = np.arange(128, dtype=np.float64)
    inc = np.round(2.0 ** 32 * 440.0 * 2.0 ** ((p - 69.0) / 12.0) / RATE).astype(np.uint32)
    return wave, inc


def voices(notes, s, wave=None, inc=None):
    """(len(notes), len(s)) int64: every voice's contribution at the samples ``s`` (0 where it is silent)."""
    if wave is None:
        wave, inc = tables()
    s = np.asarray(s, dtype=np.int64)[None, :]
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    s_on = ((notes[:, 0] * 735) >> 3)[:, None]
    s_off = ((notes[:, 1] * 735) >> 3)[:, None]
    pitch, vel = (notes[:, 2] & 127), (notes[:, 3] & 127)[:, None]
    d = s - s_on
    live = (d >= 0) & (s < s_off + RELEASE)
    d = np.where(live, d, 0)
    phase = (inc.astype(np.uint64)[pitch][:, None] * d.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    e_att = np.minimum(d + 1, ATTACK)
    e_rel = np.where(s < s_off, RELEASE, RELEASE - (s - s_off))
    v = (wave.astype(np.int64)[(phase >> np.uint64(21)).astype(np.int64)] * vel * e_att * e_rel) >> SHIFT
    return np.where(live, v, 0)


def synth(notes, s, wave=None, inc=None, chunk=1 << 16):
    """int32 samples at the positions ``s``: the sum of the voices, clamped to the 16-bit range."""
    s = np.asarray(s, dtype=np.int64)
    flat = s.ravel()
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(flat.size, dtype=np.int64)
    if len(notes):
        s_on = (notes[:, 0] * 735) >> 3
        s_end = ((notes[:, 1] * 735) >> 3) + RELEASE
        for a in range(0, flat.size, chunk):
            part = flat[a:a + chunk]
            near = (s_on <= part.max()) & (s_end > part.min())
            if near.any():
                total = voices(notes[near], part, wave, inc).sum(axis=0)
                assert np.abs(total).max() < 1 << 31
                out[a:a + chunk] = total
    return np.clip(out, -32768, 32767).astype(np.int32).reshape(s.shape)


def frame_positions(clip_len):
    """(216, 2048) sample positions of the centred frames, reflected inside [0, clip_len)."""
    hop = clip_len // (FRAMES - 1)
    idx = np.arange(FRAMES, dtype=np.int64)[:, None] * hop + np.arange(N_FFT, dtype=np.int64)[None, :] - N_FFT // 2
    idx = np.abs(idx)
    idx = np.where(idx >= clip_len, 2 * (clip_len - 1) - idx, idx)
    assert idx.min() >= 0 and idx.max() < clip_len
    return idx


def frames(notes, clip_len, wave=None, inc=None):
    """(216, 2048) fp32: stage B for one clip.  A blank clip (no notes) is all zero."""
    if len(notes) == 0 or clip_len <= N_FFT // 2:
        return np.zeros((FRAMES, N_FFT), dtype=np.float32)
    return synth(notes, frame_positions(clip_len), wave, inc).astype(np.float32) * np.float32(2.0 ** -15)


def pcm(notes, first, count, wave=None, inc=None):
    """int16 samples [first, first + count): stage C."""
    return synth(notes, np.arange(first, first + count, dtype=np.int64), wave, inc).astype(np.int16)


def wav_bytes(samples, rate=RATE):
    """The mono 16-bit RIFF file generate_song writes around ``samples``."""
    data = np.asarray(samples).astype("<i2").tobytes()
    head = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def track_of(rows):
    """The (kind, a, b, time) track process_adjsim_log writes: generate_midi's four header messages, then the rows
    (kinds as include/gdm.h's GDM_MIDI_*: note_on 4, note_off 5)."""
    head = [(0, 1000000, 0, 0), (1, 4, 4, 0), (2, 0, 0, 0), (3, 0, 0, 0)]
    return head + [(4 + r[0], r[1], r[2], r[3]) for r in rows]
