"""Plain-Python restatement of the DES log -> MIDI track -> piano-roll consumer (MMGAN_MIDI_DES/sim_log_to_midi.py:14-277
and datasets.py:13-54) -- TEST INFRASTRUCTURE ONLY.  It states, record for record, what csrc/des_midi.hip computes, and is
itself pinned by tests/golden/des_midi.npz (tracks recorded from the reference's own MidiGenerator).

A track is a list of (kind, a, b, time) integer tuples, kinds as in include/gdm.h (GDM_MIDI_*).
"""
import numpy as np

SET_TEMPO, TIME_SIGNATURE, KEY_SIGNATURE, PROGRAM_CHANGE, NOTE_ON, NOTE_OFF, END_OF_TRACK = range(7)
KIND_NAMES = ("set_tempo", "time_signature", "key_signature", "program_change", "note_on", "note_off", "end_of_track")
KEYS = ('C', 'C#', 'D', 'E', 'F', 'F#', 'G', 'G#m', 'A', 'A#m', 'B')
ARRIVAL, DEPARTURE = 0, 1
MAX_LINES = 5000


class LogError(ValueError):
    """What the reference turns into ValueError("Error in processing log file") or lets escape from MidiGenerator."""


def line_matches(value, event_id, node, kind):
    """Does the reference's regex match the text ``INFO:root:{value!r} - {event_id} - {node} - {kind name}``?  The
    integers print as digits when non-negative; a float's repr is plain digits iff it is finite, not negative (the sign
    bit prints, also for -0.0) and either zero or in [1e-4, 1e16) -- outside that range repr switches to an exponent."""
    value = float(value)
    if kind not in (ARRIVAL, DEPARTURE) or event_id < 0 or node < 0:
        return False
    if not np.isfinite(value) or np.signbit(value):
        return False
    return value == 0.0 or 1e-4 <= value < 1e16


def parameters(tail):
    """MidiGenerator.__init__ on gen2_output[10:]: float32 scalars times Python ints stay float32 (NumPy >= 2 promotion,
    which the fixtures were recorded under), int() truncates.  The np.random.randint fallbacks (skip == 0) are
    unreachable behind max(2, .)."""
    g = np.asarray(tail, dtype=np.float32)
    if not np.isfinite(g[:6]).all():
        raise LogError("non-finite MIDI parameters")
    p = {"skip": tuple(max(2, int(g[i] * np.float32(10))) for i in range(3))}
    base = int(g[3] * np.float32(90))
    p["base"] = 80 if base < 50 else base
    tempo = min(int(g[4] * np.float32(1000000)), 16777215)
    p["tempo"] = 500000 if tempo == 0 else tempo
    if p["tempo"] < 0:
        raise LogError("set_tempo out of range")
    var = int(g[5] * np.float32(63))
    p["var"] = 30 if var == 0 else var
    p["key"] = int(g[5] * np.float32(11)) % 11
    return p


def header(p):
    return [(SET_TEMPO, p["tempo"], 0, 0), (TIME_SIGNATURE, 4, 4, 0), (KEY_SIGNATURE, p["key"], 0, 0),
            (PROGRAM_CHANGE, 0, 0, 0)]


def lines_read(n_records):
    """``count`` after the reader's loop: it breaks on the 5001st line."""
    return min(int(n_records), MAX_LINES + 1)


def build_track(log, tail, instruments, note_levels, fold=(True, True), seen=None):
    """process_adjsim_log's reader + MidiGenerator.process_line over an EVENT_DTYPE-like record array -> track (before
    save_midi).  fold: switches for the two queue-count folding branches (127 <= q < 254, q >= 254) -- False leaves the
    count as it is, which is NOT the reference; tests use it to show that a fixture depends on the branch.  seen: a
    dict that receives how many arrivals took each branch."""
    p = parameters(tail)
    inst = [int(x) for x in instruments]
    notes = [int(x) for x in note_levels]
    track = header(p)
    previous_time, current_instrument = 0, 0
    queue_lengths, future = {}, {}
    s1, s2, s3 = p["skip"]
    value, event_id, node, kind = log["value"], log["event_id"], log["node"], log["kind"]
    n = min(len(value), MAX_LINES)
    for r in range(n):
        eid, nd, kd = int(event_id[r]), int(node[r]), int(kind[r])
        if not line_matches(value[r], eid, nd, kd):
            continue
        midi_time = max(0, int(float(value[r])))
        if not (midi_time < 200 and len(track) < 500):
            continue
        if previous_time > midi_time:
            midi_time = previous_time
        if not (eid % s1 == 0 or eid % s2 == 0 or eid % s3 == 0):
            continue
        if kd == ARRIVAL:
            q = queue_lengths[nd] = queue_lengths.get(nd, 0) + 1
            if 127 <= q < 254:
                if seen is not None:
                    seen["fold_127"] = seen.get("fold_127", 0) + 1
                if fold[0]:
                    q = min(127, max(0, 254 - q))
            elif q >= 254:
                if seen is not None:
                    seen["fold_254"] = seen.get("fold_254", 0) + 1
                if fold[1]:
                    q = min(127, max(0, q % 127))
            max_id = p["base"] + p["var"]
            cid = p["base"] - p["var"] + eid
            if cid > max_id:
                if max_id == 0:
                    raise LogError("customer_id % 0")
                cid = max_id - (cid % max_id)
            future[nd] = (midi_time, cid % 126, q)
            on_time = max(previous_time, midi_time)
            previous_time = on_time
            if nd >= len(inst) or nd >= len(notes):
                raise LogError("node without instrument / note level")
            if current_instrument != inst[nd]:
                current_instrument = inst[nd]
                if not 0 <= inst[nd] <= 127:
                    raise LogError("program out of range")
                track.append((PROGRAM_CHANGE, inst[nd], 0, on_time))
            if not 0 <= notes[nd] <= 127:
                raise LogError("note out of range")
            track.append((NOTE_ON, notes[nd], future[nd][1], on_time))
        else:
            if nd in future:
                t0, vel, service = future[nd]
                off_time = max(previous_time, t0 + (midi_time - t0) + max(0, service))
                previous_time = off_time
                if current_instrument != inst[nd]:
                    current_instrument = inst[nd]
                    track.append((PROGRAM_CHANGE, inst[nd], 0, off_time))
                track.append((NOTE_OFF, notes[nd], vel, off_time))
            queue_lengths[nd] = queue_lengths[nd] - 1 if nd in queue_lengths else 0
    return track


def save_track(track):
    """MidiGenerator.save_midi without the file: the remove-while-iterating loop (the element after a removed one is
    never looked at), end_of_track, clean_midi_file."""
    out, r = [], 0
    while r < len(track):
        if track[r][3] > 200:
            if r + 1 < len(track):
                out.append(track[r + 1])
            r += 2
        else:
            out.append(track[r])
            r += 1
    out.append((END_OF_TRACK, 0, 0, 0))
    on_times, keep = {}, []
    for m in out:
        drop = False
        if m[0] == NOTE_ON:
            if on_times.get(m[1], 0) > 0:
                drop = True
            else:
                on_times[m[1]] = m[3]
        elif m[0] == NOTE_OFF:
            if on_times.get(m[1], 0) == 0:
                drop = True
            else:
                on_times[m[1]] = 0
        if m[3] > 200:
            drop = True
        if not drop:
            keep.append(m)
    return keep


def track_to_planes(track, start, end, sequence_length=100, ticks_per_beat=480):
    """generate_piano_roll on a one-track file holding ``track`` (None: a MidiFile without tracks) -> (roll, dur)."""
    width = end - start
    roll, dur = np.zeros((128, width)), np.zeros((128, width))
    on_time = [0] * 128
    tempo, my_time = 500000, 0.0
    for (kind, a, b, ticks) in (track or []):
        if kind == END_OF_TRACK:
            continue                        # time 0 at the end of the track: nothing is carried
        my_time += ticks * (tempo * 1e-6 / ticks_per_beat) if ticks > 0 else 0.0
        if kind == SET_TEMPO:
            tempo = a
        step = int(round(my_time))
        if step >= sequence_length:
            break
        if kind == NOTE_ON:
            if step >= width:
                break
            roll[a, step] = b
            on_time[a] = step
        elif kind == NOTE_OFF:
            dur[a, on_time[a]:step] = step - on_time[a]
    sl = slice(start, end) if end < 128 else slice(0, end)
    return roll[:, sl], dur[:, sl]


def consume(log, tail, instruments, note_levels, generate=False, start=0, end=30, sequence_length=100):
    """-> (track as it stands at the end, saved?, roll, dur)."""
    track = build_track(log, tail, instruments, note_levels)
    saved = bool(generate) or lines_read(len(log["value"])) % 100 == 0
    if saved:
        track = save_track(track)
    roll, dur = track_to_planes(track if saved else None, start, end, sequence_length)
    return track, saved, roll, dur
