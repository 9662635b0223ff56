#!/usr/bin/env python
"""Record tests/golden/des_notes.npz: the note_on / note_off messages the REFERENCE's own reader and MidiGenerator
(GAN_DES/sim_log_process_music.py) build from model-1 event logs.

    python tests/golden/make_des_notes_golden.py <path to the reference checkout>

The reference module is imported as it lies there, at record time only; nothing of its text is copied.  mido is not
needed to BUILD a track, so a stand-in module of this project's own provides the names the reference touches: Message /
MetaMessage (objects with ``type``, ``time`` and keyword fields; ``note`` and ``velocity`` must be integers in 0..127 and
``time`` a real number, as mido demands), MidiTrack (a list) and MidiFile (``tracks``, a ``save`` that writes nothing).

Each case writes its records to ./logs/simulation.log in the line format of the simulator's 'Music' logging and calls the
reference's process_adjsim_log with PLAIN LISTS for ``instruments`` and ``note_levels`` (its ``note_levels != []`` test is
written for lists; on an array it raises under NumPy >= 2), so the reader's regex, its 5000-line limit and
MidiGenerator.process_line are all the reference's own.  Stored per case: the records (or, for the recorded DES logs,
their name in des_core.npz and the number of lines), the two lists and the emitted (type, note, velocity, time) rows with
type 0 = note_on, 1 = note_off.
"""
import numbers
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_NAMES = ("arrival", "departure", "processing")
FIELDS = ("value", "event_id", "node", "kind")


class _Msg:
    def __init__(self, type, time=0, **fields):
        for k in ("note", "velocity"):
            if k in fields and not (isinstance(fields[k], numbers.Integral) and 0 <= fields[k] <= 127):
                raise ValueError(f"{k} {fields[k]!r} must be an integer in 0..127")
        if not isinstance(time, numbers.Real):
            raise TypeError("time must be a number")
        self.type, self.time = type, time
        self.__dict__.update(fields)


class _File:
    def __init__(self):
        self.tracks = []

    def save(self, filename):
        pass


def install_stand_in():
    mido = types.ModuleType("mido")
    mido.Message, mido.MetaMessage, mido.MidiTrack, mido.MidiFile = _Msg, _Msg, type("MidiTrack", (list,), {}), _File
    sys.modules["mido"] = mido


def records(rows):
    """[(value, event_id, node, kind)] -> the four field arrays."""
    v, e, n, k = zip(*rows) if rows else ((), (), (), ())
    return {"value": np.asarray(v, np.float64), "event_id": np.asarray(e, np.int64), "node": np.asarray(n, np.int32),
            "kind": np.asarray(k, np.int32)}


def crafted():
    """name -> record rows: every branch of process_line and of the reader."""
    A, D, P = 0, 1, 2
    out = {}
    # a departure before any arrival on its node (the queue count goes negative: 40 of them, so that 30 + q < 0 and
    # Python's % differs from C's), then the arrival / departure pair that sounds
    rows = [(1.0 + i, 3 * i, 0, D) for i in range(40)]
    rows += [(50.5, 15, 0, A), (53.0, 15, 0, D), (55.0, 21, 1, D), (56.0, 45, 0, A), (57.25, 45, 0, D)]
    out["departures_first"] = rows
    # repeated departures after ONE arrival: future_events is never cleared
    out["repeated_departures"] = [(2.0, 9, 2, A), (4.0, 9, 2, D), (5.0, 10, 2, D), (9.5, 14, 2, D), (9.75, 12, 3, D)]
    # >= 255 unanswered arrivals on one node: two arrivals per departure, 300 times -- the count climbs through both
    # folds (127, 254) and every note's off time carries the folded count of its second arrival
    rows = []
    for i in range(300):
        t = 3.0 * i
        rows += [(t, 105 * i, 1, A), (t + 1.0, 105 * i + 15, 1, A), (t + 2.0, 105 * i + 30, 1, D)]
    out["queue_folds"] = rows
    # event ids on both sides of the customer-id folds (queue count 1: max_customer_id = 31, folds at 31 and 62)
    rows = []
    for j, eid in enumerate((0, 3, 30, 33, 35, 60, 63, 65, 70, 93, 126, 1005, 123456789)):
        rows += [(10.0 * j, eid, 2, A), (10.0 * j + 4.0, eid, 2, D)]
    out["customer_id_folds"] = rows
    # ids failing all three moduli between an audible pair: no state changes
    rows = [(1.0, 6, 0, A)]
    rows += [(2.0 + i, eid, 0, (A, D)[i % 2]) for i, eid in enumerate((1, 2, 4, 8, 11, 13, 16, 17, 19, 22))]
    rows += [(20.0, 6, 0, D)]
    out["ids_filtered"] = rows
    # values: 0, 0.5 (midi_time 0), an exponent in the repr and a sign (both unmatched), 'processing' lines
    out["values"] = [(0.0, 3, 0, A), (0.5, 3, 0, D), (1e-05, 5, 1, A), (2.5, 5, 1, D), (-1.0, 7, 2, A), (3.0, 7, 2, D),
                     (4.0, 9, 3, P), (1e16, 9, 3, A), (6.0, 9, 3, D), (1234.75, 10, 3, A), (1300.0, 10, 3, D),
                     (0.0001, 12, 0, A), (7.0, 12, 0, D)]
    # 5003 lines: the reader stops after 5000; line 5000 is an arrival, the last three are departures of its node
    rows = [(0.25 * i, 1 + 105 * i, 0, (A, D)[i % 2]) for i in range(4999)]            # ids = 1 mod 105: all filtered
    rows += [(1250.5, 15, 2, A), (1253.0, 15, 2, D), (1254.0, 15, 2, D), (1255.0, 21, 2, D)]
    out["lines_5003"] = rows
    return out


def main(ref_dir):
    install_stand_in()
    sys.path.insert(0, os.path.join(ref_dir, "GAN_DES"))
    import sim_log_process_music as M                 # the reference's module, imported where it lies
    sys.path.pop(0)
    made, original_init = [], M.MidiGenerator.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        original_init(self, *a, **k)

    M.MidiGenerator.__init__ = recording_init
    core = np.load(os.path.join(HERE, "des_core.npz"))
    rng = np.random.default_rng(20241019)
    cases = []
    for log in ("wav0", "wav1"):
        rec = {k: core[f"{log}/{k}"][:5001] for k in FIELDS}
        dim = int(core[f"{log}/sim_matrix"].shape[0])
        cases.append((f"{log}_5001_lines", rec, dim, log))
    for name, rows in crafted().items():
        cases.append((name, records(rows), 4, None))
    store, names = {}, []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs("logs")
        os.makedirs("adj_sim_outputs/midi")
        try:
            for name, rec, dim, source in cases:
                v, e, nd, kd = (rec[k] for k in FIELDS)
                with open("logs/simulation.log", "w") as f:
                    for i in range(len(v)):
                        f.write(f"INFO:root:{float(v[i])!r} - {int(e[i])} - {int(nd[i])} - {KIND_NAMES[kd[i]]}\n")
                instruments = [int(x) for x in rng.integers(0, 100, dim)]
                note_levels = [int(x) for x in rng.integers(36, 96, dim)]
                M.process_adjsim_log(instruments=instruments, note_levels=note_levels)
                track = made[-1].track
                assert track.pop().type == "end_of_track"          # save_midi's; generate_midi is never called
                rows = np.asarray([(("note_on", "note_off").index(m.type), m.note, m.velocity, m.time) for m in track],
                                  dtype=np.int64).reshape(-1, 4)
                names.append(name)
                if source is None:
                    for k in FIELDS:
                        store[f"{name}/{k}"] = rec[k]
                else:
                    store[f"{name}/log"] = np.asarray(source)
                    store[f"{name}/n_lines"] = np.asarray(len(v), dtype=np.int64)
                store[f"{name}/instruments"] = np.asarray(instruments, dtype=np.int64)
                store[f"{name}/note_levels"] = np.asarray(note_levels, dtype=np.int64)
                store[f"{name}/rows"] = rows
                print(name, "lines", len(v), "notes", len(rows) // 2, "velocities",
                      (int(rows[:, 2].min()), int(rows[:, 2].max())) if len(rows) else None,
                      "ticks", int(rows[:, 3].sum()) if len(rows) else 0)
        finally:
            os.chdir(cwd)
    store["names"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "des_notes.npz"), **store)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
