#!/usr/bin/env python
"""Record tests/golden/des_midi.npz: the tracks the REFERENCE's own MidiGenerator / process_adjsim_log
(MMGAN_MIDI_DES/sim_log_to_midi.py) build from the model-2 event logs of tests/golden/des_core.npz.

    python tests/golden/make_des_midi_golden.py <path to the reference checkout>

The reference module is imported as it lies there, at record time only; nothing of its text is copied.  mido is not
needed to BUILD a track (only to write the file), so a stand-in module of this project's own provides the four names the
reference touches: Message / MetaMessage (objects with ``type``, ``time`` = 0 by default and keyword fields, range-checked
like mido's), MidiTrack (a list) and MidiFile (``tracks``, a ``save`` that writes nothing).  ``datasets`` (which pulls in
pretty_midi) is replaced by a stub whose generate_piano_roll hands the MidiFile back.

Per case the file holds the inputs (log name, number of lines, transform, gen2 tail, instruments, note levels, generate)
and the results: the track before save_midi, the track after it (empty when save_midi did not run) and the save decision.
A track is an (n, 4) int32 array of (kind, a, b, time) with the kinds of include/gdm.h (GDM_MIDI_*).

Transforms (so that no derived log needs storing): 0 = the log as recorded; 1 = its arrival records only, all moved to
node (event_id % 2) -- two nodes that only ever fill up (note_on messages only: the folded queue count is never consumed);
2 = its arrival records only, all moved to node 0: the first ``fill`` stay arrivals, the following ones alternate
departure / arrival.  The node's queue count then sits where the fill left it -- in [127, 254) or at >= 254, one case
each per log -- and every later note_off time carries the FOLDED count as the note's service time.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("set_tempo", "time_signature", "key_signature", "program_change", "note_on", "note_off", "end_of_track")
KEYS = ('C', 'C#', 'D', 'E', 'F', 'F#', 'G', 'G#m', 'A', 'A#m', 'B')
KIND_NAMES = ("arrival", "departure", "processing")


class _Msg:
    _RANGES = {"program": 127, "note": 127, "velocity": 127, "channel": 15, "tempo": 0xFFFFFF}

    def __init__(self, type, time=0, **fields):
        for k, v in fields.items():
            if k in self._RANGES and not 0 <= v <= self._RANGES[k]:
                raise ValueError(f"{k} {v} out of range")
        self.type, self.time = type, time
        self.__dict__.update(fields)

    def __eq__(self, other):                      # mido compares every field, the time included
        return isinstance(other, _Msg) and self.__dict__ == other.__dict__


class _File:
    def __init__(self):
        self.tracks, self.filename = [], None

    def save(self, filename):
        self.filename = filename


def install_stand_ins():
    mido = types.ModuleType("mido")
    mido.Message, mido.MetaMessage, mido.MidiTrack, mido.MidiFile = _Msg, _Msg, type("MidiTrack", (list,), {}), _File
    sys.modules["mido"] = mido
    datasets = types.ModuleType("datasets")
    datasets.generate_piano_roll = lambda mid, start=0, end=50: mid
    sys.modules["datasets"] = datasets


def as_rows(track):
    rows = []
    for m in track:
        k = KINDS.index(m.type)
        a, b = {"set_tempo": lambda: (m.tempo, 0), "time_signature": lambda: (m.numerator, m.denominator),
                "key_signature": lambda: (KEYS.index(m.key), 0), "program_change": lambda: (m.program, 0),
                "note_on": lambda: (m.note, m.velocity), "note_off": lambda: (m.note, m.velocity),
                "end_of_track": lambda: (0, 0)}[m.type]()
        rows.append((k, int(a), int(b), int(m.time)))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def transformed(log, transform, n_lines, fill=0):
    value, event_id, node, kind = (log[k] for k in ("value", "event_id", "node", "kind"))
    if transform in (1, 2):
        keep = kind == 0
        value, event_id, kind = value[keep], event_id[keep], kind[keep]
        node = (event_id % 2).astype(np.int32)
    if transform == 2:
        node = np.zeros_like(node)
        kind = kind.copy()
        kind[fill::2] = 1
    return value[:n_lines], event_id[:n_lines], node[:n_lines], kind[:n_lines]


def cases():
    """(name, log, n_lines (None = all), transform, tail, instrument (None = per node), generate[, fill])."""
    rng = np.random.default_rng(20240607)
    t = lambda *v: np.asarray(list(v) + [0.5] * (10 - len(v)), dtype=np.float32)
    out = []
    for log in ("midi0", "midi1"):
        for j in range(3):                                             # sigmoid-like tails, per-node instruments
            out.append((f"{log}_rand{j}", log, None, 0, rng.random(10).astype(np.float32), None, True))
        out.append((f"{log}_one_instrument", log, None, 0, rng.random(10).astype(np.float32), 7, True))
        out.append((f"{log}_low_base_var0_tempo0", log, None, 0, t(0.31, 0.52, 0.77, 0.2, 0.0000004, 0.01), None, True))
        out.append((f"{log}_tempo_capped", log, None, 0, t(0.05, 0.11, 0.93, 0.99, 17.5, 0.97), None, True))
        out.append((f"{log}_3000_lines_simulation", log, 3000, 0, t(0.23, 0.41, 0.35, 0.8, 0.6, 0.7), None, False))
        out.append((f"{log}_1234_lines_generate", log, 1234, 0, t(0.23, 0.41, 0.35, 0.8, 0.6, 0.7), 0, True))
        out.append((f"{log}_1234_lines_not_saved", log, 1234, 0, t(0.23, 0.41, 0.35, 0.8, 0.6, 0.7), None, False))
        out.append((f"{log}_all_lines_not_saved", log, None, 0, t(0.9, 0.2, 0.3, 0.7, 0.25, 0.4), None, False))
        out.append((f"{log}_queues_fill", log, None, 1, t(0.2, 0.3, 0.5, 0.75, 0.3, 0.6), None, True))
        out.append((f"{log}_slow_tempo", log, None, 0, t(0.2, 0.3, 0.5, 0.75, 9.7, 0.45), 3, True))
    # appended, so that the cases above keep their random draws; fills chosen so that about 150 / 275 of the leading
    # arrivals match the regex and pass the skip moduli (midi1 opens with negative times, which do not match)
    for log, fill_127, fill_254 in (("midi0", 195, 378), ("midi1", 290, 484)):
        out.append((f"{log}_queue_fold_127", log, None, 2, t(0.2, 0.3, 0.5, 0.75, 0.3, 0.6), None, True, fill_127))
        out.append((f"{log}_queue_fold_254", log, None, 2, t(0.2, 0.3, 0.5, 0.75, 0.3, 0.6), None, True, fill_254))
    return out


def main(ref_dir):
    install_stand_ins()
    sys.path.insert(0, os.path.join(ref_dir, "MMGAN_MIDI_DES"))
    import sim_log_to_midi as M                       # the reference's module, imported where it lies
    sys.path.pop(0)
    before = {}
    original_save = M.MidiGenerator.save_midi

    def recording_save(self, filename):
        before["track"] = as_rows(self.track)
        original_save(self, filename)

    M.MidiGenerator.save_midi = recording_save
    made, original_init = [], M.MidiGenerator.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        original_init(self, *a, **k)

    M.MidiGenerator.__init__ = recording_init
    core = np.load(os.path.join(HERE, "des_core.npz"))
    rng = np.random.default_rng(7)
    store, names = {}, []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs("logs")
        try:
            for (name, log, n_lines, transform, tail, instrument, generate, *rest) in cases():
                fill = rest[0] if rest else 0
                rec = {k: core[f"{log}/{k}"] for k in ("value", "event_id", "node", "kind")}
                dim = int(core[f"{log}/sim_matrix"].shape[0])
                v, e, nd, kd = transformed(rec, transform, n_lines, fill)
                with open("logs/simulation.log", "w") as f:     # the line format of simulation_v3's 'Music' logging
                    for i in range(len(v)):
                        f.write(f"INFO:root:{float(v[i])!r} - {int(e[i])} - {int(nd[i])} - {KIND_NAMES[kd[i]]}\n")
                instruments = np.array([instrument] * dim) if instrument is not None else \
                    rng.integers(0, 127, dim).astype(np.float64)
                note_levels = rng.integers(0, 128, dim).astype(np.float64)
                before.clear()
                mid = M.process_adjsim_log(instruments=instruments, note_levels=note_levels, gen2_output=tail,
                                           count=1, start=0, end=50, generate=generate)
                saved = len(mid.tracks) == 1
                if not saved:                            # save_midi did not run: the track as process_line left it
                    before["track"] = as_rows(made[-1].track)
                names.append(name)
                store[f"{name}/log"] = np.asarray(log)
                store[f"{name}/n_lines"] = np.asarray(-1 if n_lines is None else n_lines, dtype=np.int64)
                store[f"{name}/transform"] = np.asarray(transform, dtype=np.int64)
                store[f"{name}/fill"] = np.asarray(fill, dtype=np.int64)
                store[f"{name}/tail"] = tail
                store[f"{name}/instruments"] = np.asarray(instruments, dtype=np.float64)
                store[f"{name}/note_levels"] = note_levels
                store[f"{name}/generate"] = np.asarray(bool(generate))
                store[f"{name}/saved"] = np.asarray(saved)
                store[f"{name}/before"] = before["track"]
                store[f"{name}/after"] = as_rows(mid.tracks[0]) if saved else np.zeros((0, 4), np.int32)
                print(name, "lines", len(v), "saved", saved, "before", len(before["track"]), "after",
                      len(store[f"{name}/after"]), "max time", int(before["track"][:, 3].max()))
        finally:
            os.chdir(cwd)
    store["names"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "des_midi.npz"), **store)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
