"""Pure-Python mirror of how the reference builds model 2's training set (MMGAN_MIDI_DES/data_viewing_and_processing.ipynb):
cell 10's four-value ``generate_piano_roll(midi, sample_size, beats_length)`` and cell 11's loop that cuts its planes
into windows, both restated with upstream's control flow, over ``oracle.midi_events.merged_seconds`` (the stream
``for msg in mido.MidiFile(path)`` yields, final end_of_track included) and ``oracle.piano_roll.get_beats``.

PARITY UNPINNED, like the piano-roll path it extends: mido and pretty_midi are absent, the reference ships neither its
pickle nor a MAESTRO file, so this mirror is the yardstick and nothing pins the mirror itself but the notebook's text.
Everything compared is an integer, or a float32 cast of the same float64 value: the checks ask for equal bits.

``faults`` switches on planted faults, one at a time, for the tests that show the checker rejects them.
"""
import struct

import numpy as np

from oracle import midi_events as ome, piano_roll as opr

FAULTS = ("keep_window_0", "drop_final_eot", "floor")


def _data(src):
    if isinstance(src, (bytes, bytearray)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def generate_piano_roll(src, sequence_length=300, beats_length=50, faults=()):
    """Notebook cell 10: (piano_roll, durations (128, sequence_length) float64, beats, total_time)."""
    fmt, tpb, tracks = ome.read_tracks(_data(src))
    midi = ome.merged_seconds(fmt, tpb, tracks)
    if "drop_final_eot" in faults:
        midi = midi[:-1]
    piano_roll = np.zeros((128, sequence_length))
    durations = np.zeros((128, sequence_length))
    total_time = 0
    my_time = 0
    note_on_time = np.zeros(128)
    for (msg_time, msg_type, msg_note, msg_velocity) in midi:
        my_time += msg_time
        time_step = int(np.floor(my_time)) if "floor" in faults else int(round(my_time))
        total_time = time_step
        if time_step >= sequence_length:
            break
        if msg_type == "note_on":
            piano_roll[msg_note, time_step] = msg_velocity
            note_on_time[msg_note] = time_step
        elif msg_type == "note_off":
            note_off_time = int(round(note_on_time[msg_note]))
            durations[msg_note, note_off_time:time_step] = time_step - note_off_time
    beats = opr.get_beats(fmt, tpb, tracks)
    if len(beats) < beats_length:
        beats = np.pad(beats, (0, beats_length - len(beats)))
    elif len(beats) > beats_length:
        beats = beats[:beats_length]
    return piano_roll, durations, beats, total_time


def file_windows(src, sample_size=300, sequence_length=50, beats_length=50, faults=()):
    """Notebook cell 11 for one file: (total_time, [window index], [(roll, dur, beats) float32 arrays])."""
    piano_roll, durations, beats, total_time = generate_piano_roll(src, sample_size, beats_length, faults)
    beats32 = beats.astype(np.float32)
    kept, items = [], []
    number_of_training_samples = int(np.floor(total_time / sequence_length))
    for i in range(number_of_training_samples):
        start = i * sequence_length
        piano_roll_slice = piano_roll[:, start:start + sequence_length]
        durations_slice = durations[:, start:start + sequence_length]
        if piano_roll_slice.shape[1] == sequence_length and durations_slice.shape[1] == sequence_length and \
                (i != 0 or "keep_window_0" in faults):
            kept.append(i)
            items.append((piano_roll_slice.astype(np.float32), durations_slice.astype(np.float32), beats32))
    return total_time, kept, items


def dataset(sources, sample_size=300, sequence_length=50, beats_length=50):
    """Cell 11 over a file list: (items, file_index, window_index), items in the order ``preprocessed_data`` has."""
    items, file_index, window_index = [], [], []
    for idx, src in enumerate(sources):
        _t, kept, its = file_windows(src, sample_size, sequence_length, beats_length)
        items += its
        file_index += [idx] * len(kept)
        window_index += kept
    return items, np.asarray(file_index, dtype=np.int64), np.asarray(window_index, dtype=np.int64)


def write_pickle(items, path):
    """``preprocessed_data_{L}.pkl`` as cell 11 dumps it: a list of (piano_roll, durations, beats) float32 tensors."""
    import pickle

    import torch
    with open(path, "wb") as f:
        pickle.dump([tuple(torch.from_numpy(np.ascontiguousarray(a)).float() for a in it) for it in items], f)


# ---- synthetic Standard MIDI Files, assembled from bytes --------------------------------------------------------------
def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def smf(tracks, tpb=480, fmt=1, eot_gap=0):
    """tracks: lists of (delta ticks, raw message bytes); every track ends with end_of_track ``eot_gap`` ticks (a number,
    or one per track) behind its last message.  An empty list is an empty track (no message at all, not even that)."""
    gaps = eot_gap if isinstance(eot_gap, (list, tuple)) else [eot_gap] * len(tracks)
    body = b""
    for ev, gap in zip(tracks, gaps):
        tr = b"".join(_vlq(d) + raw for d, raw in ev) + (_vlq(gap) + b"\xff\x2f\x00" if ev else b"")
        body += b"MTrk" + struct.pack(">I", len(tr)) + tr
    return b"MThd" + struct.pack(">IHHH", 6, fmt, len(tracks), tpb) + body


def _tempo(us):
    return b"\xff\x51\x03" + us.to_bytes(3, "big")


def _notes(pairs):
    """(delta seconds at tempo 500000 / tpb 480, note, velocity or None for note_off) -> track events."""
    return [(int(round(sec * 960)), bytes([0x90 if vel is not None else 0x80, note, vel or 0]))
            for sec, note, vel in pairs]


def synthetic_files():
    """name -> SMF bytes.  Times: tpb 480 and tempo 500000 make one second 960 ticks."""
    out = {}
    # two tracks, a tempo change (one tick costs twice as much after 3 s), running status, a note_on of velocity 0,
    # a re-struck note, notes spread over ~40 s
    t0 = [(0, _tempo(500000)), (0, b"\xff\x58\x04\x04\x02\x18\x08"), (960 * 3, _tempo(1000000))]
    t1 = [(0, b"\x90\x3c\x40"), (480, b"\x3e\x50"), (480, b"\x80\x3c\x00"), (960, b"\x90\x3c\x7f"),
          (960, b"\x90\x3e\x00"), (480, b"\x80\x3c\x10")]
    for k in range(36):                                            # 480 ticks = 1 s at the slow tempo
        t1 += [(480, bytes([0x90, 40 + k, 30 + k])), (240 + 40 * (k % 5), bytes([0x80, 40 + k, 0]))]
    out["two_tracks_tempo_running_status"] = smf([t0, t1])
    # the same notes, end_of_track 5000 ticks behind the last note (and without): total_time must grow with the gap
    held = _notes([(3, 60, 64), (20, 60, None), (1, 62, 90), (2, 62, None), (4, 60, 33), (5, 60, None)])
    out["eot_gap_0"] = smf([held])
    out["eot_gap_5000"] = smf([held], eot_gap=5000)
    # format 0, one note, a long gap before end_of_track
    out["format0_one_note_long_gap"] = smf([_notes([(1, 72, 100), (2, 72, None)])], fmt=0, eot_gap=960 * 50)
    # an empty track beside a real one
    out["empty_track"] = smf([[], _notes([(2, 50, 70), (9, 50, None), (12, 51, 71), (3, 51, None)])], eot_gap=[0, 960])
    # a message that jumps from below sample_size to beyond it: total_time > sample_size for sample_size <= 300
    out["jump_beyond_sample_size"] = smf([_notes([(2, 64, 80), (3, 64, None), (400, 65, 81), (1, 65, None)])])
    # running times at exactly x.5: 6.5 -> 6, 7.5 -> 8 (half to even), last message at 24.5 -> 24
    # (tempo 1000000 and tpb 2 make one tick 1000000 * 1e-6 / 2 = 0.5 s exactly, and sums of halves are exact)
    out["half_steps"] = smf([[(0, _tempo(1000000)), (1, b"\x90\x3c\x0a"), (12, b"\x80\x3c\x00"), (2, b"\x90\x3d\x14"),
                              (10, b"\x80\x3d\x00"), (24, b"\x90\x3e\x1e")]], tpb=2)
    return out
