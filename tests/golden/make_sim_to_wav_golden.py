#!/usr/bin/env python
"""Record tests/golden/sim_to_wav.npz: what the REFERENCE's stand-alone demo (SIMULATOR/simulation_to_wav.py) computes
between ``np.random.seed(k)`` and the MIDI track it saves.

    python tests/golden/make_sim_to_wav_golden.py <path to the reference checkout>

The reference modules are imported as they lie there, at record time only; nothing of their text is copied.  Two
packages the demo imports are not needed to BUILD a track and are replaced by stand-ins of this project's own, in the
way make_des_notes_golden.py does it: ``mido`` (Message / MetaMessage objects with ``type``, ``time`` and keyword
fields -- ``note``, ``velocity`` and ``program`` must be integers in 0..127 and ``time`` a real number, as mido demands
--, MidiTrack, and a MidiFile whose ``save`` only notes how many tracks it was given) and ``midi2audio`` (a FluidSynth
that renders nothing).

The demo hands ``instruments`` and ``note_levels`` to process_adjsim_log as arrays, and MidiGenerator tests
``note_levels != []``, which raises under NumPy >= 2: the lists of the same values are passed instead (the behaviour of
the NumPy the demo was written for), as make_des_notes_golden.py does.

Every case runs in an interpreter of its own (only the first Sim of a process gets a log file
on this Python); inside a case the root logger's handlers are cleared before every ``Sim`` so that the second matrix of
a two-matrix call logs too.  Per sample the file holds:

    matrix        the (size, size) input: the given one, or the drawn one rebuilt from the reference's own
                  ``np.random.rand`` results (they are intercepted, not re-drawn)
    sim_matrix, dist (dim, 2), queue_list, seeds, customers      what ``Sim`` was constructed / run with
    instruments, note_levels                                      what process_adjsim_log was given
    value, event_id, node, kind   the first 5000 'Music' records; n_records and sha256 cover the complete arrays
                                  (little-endian value | event_id | node | kind bytes, in this order)
    rows          the channel messages of the saved track: (type, a, velocity, time), type 0 note_on, 1 note_off,
                  2 program_change (a = program, velocity 0)
    meta          the names of the track's meta messages in order; n_tracks: the tracks of the saved file
and per case ``seed``, ``size``, ``instrument`` (-1: None), ``count`` and ``rng_after`` (one global randint after the
call: where the stream stands).
"""
import hashlib
import json
import numbers
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"arrival": 0, "departure": 1, "processing": 2}
HEAD = 5000
# name -> (seed, size, matrices ("none" | "params" | "nosource" per entry), use_same_instrument)
CASES = {
    "size8": (5, 8, ["none"], None),
    "size13": (3, 13, ["none"], None),
    "size32": (7, 32, ["none"], None),
    "two_size13": (2, 13, ["none", "none"], None),
    "instrument91": (5, 13, ["none"], 91),
    "given_params": (17, 12, ["params"], None),
    "no_source": (19, 10, ["nosource"], None),
}


def given_matrix(kind, size, seed):
    """The two given matrices, from a generator of their own (numpy's global stream is the demo's)."""
    rng = np.random.default_rng(1000 + seed)
    dim = size - 5
    m = rng.random((size, size))
    if kind == "params":              # nonzero parameter columns: they enter the row sums, two of them as "sources"
        m[dim, :dim] = rng.random(dim) * 0.7
        m[dim, [1, 4]] = (0.9, 0.8)
        m[dim, dim:] = (0.95, 0.1, 0.8, 0.2, 0.76)
    else:                             # no entry of the source row above 0.75
        m[dim] = rng.random(size) * 0.75
    return m


class _Msg:
    def __init__(self, type, time=0, **fields):
        for k in ("note", "velocity", "program"):
            if k in fields and not (isinstance(fields[k], numbers.Integral) and 0 <= fields[k] <= 127):
                raise ValueError(f"{k} {fields[k]!r} must be an integer in 0..127")
        if not isinstance(time, numbers.Real):
            raise TypeError("time must be a number")
        self.type, self.time = type, time
        self.__dict__.update(fields)


class _File:
    saved = []

    def __init__(self):
        self.tracks = []

    def save(self, filename):
        _File.saved.append(len(self.tracks))


def install_stand_ins():
    mido = types.ModuleType("mido")
    mido.Message, mido.MetaMessage, mido.MidiTrack, mido.MidiFile = _Msg, _Msg, type("MidiTrack", (list,), {}), _File
    sys.modules["mido"] = mido
    m2a = types.ModuleType("midi2audio")
    m2a.FluidSynth = type("FluidSynth", (), {"__init__": lambda self, *a, **k: None,
                                             "midi_to_audio": lambda self, *a, **k: None})
    sys.modules["midi2audio"] = m2a
    if "IPython" not in sys.modules:                    # imported at the simulator's top level, touched by animations only
        try:
            import IPython.display  # noqa: F401
        except ImportError:
            ipy, disp = types.ModuleType("IPython"), types.ModuleType("IPython.display")
            disp.HTML, ipy.display = object, disp
            sys.modules["IPython"], sys.modules["IPython.display"] = ipy, disp


def read_log(path):
    line_re = re.compile(r"INFO:root:(\S+) - (\S+) - (\S+) - (arrival|departure|processing)$")
    v, e, n, k = [], [], [], []
    for ln in open(path):
        m = line_re.match(ln.strip())
        assert m, ln
        v.append(float(m.group(1)))
        e.append(int(m.group(2)))
        n.append(int(m.group(3)))
        k.append(KINDS[m.group(4)])
    return (np.asarray(v, np.float64), np.asarray(e, np.int64), np.asarray(n, np.int32), np.asarray(k, np.int32))


def records_sha256(value, event_id, node, kind):
    h = hashlib.sha256()
    for a, dt in ((value, "<f8"), (event_id, "<i8"), (node, "<i4"), (kind, "<i4")):
        h.update(np.ascontiguousarray(a).astype(dt).tobytes())
    return h.hexdigest()


def run_case(ref_dir, name, out_path):
    """Worker: one case in this interpreter -> out_path (.npz)."""
    import logging
    seed, size, kinds, instrument = CASES[name]
    install_stand_ins()
    sys.path.insert(0, os.path.join(ref_dir, "SIMULATOR"))
    import simulation_to_wav as M                      # the reference's module, imported where it lies
    sys.path.pop(0)
    real_sim, real_process, real_rand = M.Sim, M.process_adjsim_log, np.random.rand
    sims, calls, tracks, draws = [], [], [], []

    class RecordingSim:
        def __init__(self, adj, distributions, queue_list, **kw):
            for h in list(logging.root.handlers):
                logging.root.removeHandler(h)
            sims.append({"sim_matrix": np.array(adj, dtype=np.float64),
                         "dist": np.array([[float(d[1]), float(d[2])] for d in distributions], np.float64).reshape(-1, 2),
                         "queue_list": np.asarray(queue_list, np.int64), "seeds": np.asarray(kw["seeds"], np.int64),
                         "kinds": [d[0] for d in distributions], "kw": {k: v for k, v in kw.items() if k != "seeds"}})
            self.sim = real_sim(adj, distributions, queue_list, **kw)

        def run(self, number_of_customers=50, **kw):
            sims[-1]["customers"] = np.int64(number_of_customers)
            self.sim.run(number_of_customers=number_of_customers, **kw)
            logging.shutdown()
            sims[-1]["log"] = read_log("logs/simulation.log")

    made, original_init = [], M.MidiGenerator.__init__

    def recording_init(self, *a, **k):
        made.append(self)
        original_init(self, *a, **k)

    def recording_process(**kw):
        calls.append({k: np.array([int(x) for x in kw[k]], np.int64) for k in ("instruments", "note_levels")})
        path = real_process(**{k: list(v) for k, v in kw.items()})     # plain lists: see the docstring
        tracks.append(list(made[-1].track))
        return path

    def recording_rand(*shape):
        out = real_rand(*shape)
        draws.append(np.array(out))
        return out

    M.Sim, M.process_adjsim_log, M.MidiGenerator.__init__ = RecordingSim, recording_process, recording_init
    given = [None if k == "none" else given_matrix(k, size, seed) for k in kinds]
    inputs = [None if g is None else g.copy() for g in given]
    os.makedirs("logs")
    os.makedirs("adj_sim_outputs/midi")
    np.random.seed(seed)
    np.random.rand = recording_rand
    try:
        M.sim_to_wav(matrices=inputs, size=size, use_same_instrument=instrument)
    finally:
        np.random.rand = real_rand
    rng_after = np.int64(np.random.randint(0, 2 ** 31 - 1))
    assert len(sims) == len(calls) == len(tracks) == len(kinds) and _File.saved == [1] * len(kinds), _File.saved
    store = {"seed": np.int64(seed), "size": np.int64(size), "count": np.int64(len(kinds)),
             "instrument": np.int64(-1 if instrument is None else instrument), "rng_after": rng_after}
    dim, d = size - 5, 0
    for j, kind in enumerate(kinds):
        if given[j] is None:                           # rebuilt from the demo's own six draws
            m = draws[d].copy()
            assert m.shape == (size, size) and all(x.shape == (dim,) for x in draws[d + 1:d + 6])
            m[dim:, :] = 0
            m[:, dim:] = 0
            for r in range(5):
                m[dim + r, :dim] = draws[d + 1 + r]
            d += 6
        else:
            m = given[j]
        s = sims[j]
        assert s["kinds"] == ["normal"] * dim and s["kw"] == {"generate_log": True, "animation": False,
                                                                "record_history": False, "logging_mode": "Music"}, s["kw"]
        value, event_id, node, kd = s["log"]
        rows, meta = [], []
        for msg in tracks[j]:
            if msg.type in ("note_on", "note_off"):
                assert msg.channel == 0
                rows.append((("note_on", "note_off").index(msg.type), msg.note, msg.velocity, msg.time))
            elif msg.type == "program_change":
                rows.append((2, msg.program, 0, msg.time))
            else:
                meta.append(msg.type)
        pre = f"{j}/"
        store.update({pre + "matrix": m, pre + "given": np.bool_(given[j] is not None),
                      pre + "sim_matrix": s["sim_matrix"], pre + "dist": s["dist"], pre + "queue_list": s["queue_list"],
                      pre + "seeds": s["seeds"], pre + "customers": s["customers"],
                      pre + "instruments": calls[j]["instruments"], pre + "note_levels": calls[j]["note_levels"],
                      pre + "value": value[:HEAD], pre + "event_id": event_id[:HEAD], pre + "node": node[:HEAD],
                      pre + "kind": kd[:HEAD], pre + "n_records": np.int64(len(value)),
                      pre + "sha256": np.asarray(records_sha256(value, event_id, node, kd)),
                      pre + "rows": np.asarray(rows, np.int64).reshape(-1, 4), pre + "meta": np.asarray(meta, dtype=str),
                      pre + "n_tracks": np.int64(_File.saved[j])})
        print(json.dumps({"case": name, "sample": j, "sources": int((s["sim_matrix"].diagonal() > 0).sum()),
                          "records": len(value), "notes": sum(r[0] == 0 for r in rows), "meta": meta}))
    assert d == len(draws)
    np.savez(out_path, **store)


def main(ref_dir):
    store, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            work = os.path.join(tmp, name)
            os.makedirs(work)
            out = os.path.join(work, "case.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), os.path.abspath(ref_dir), name, out], cwd=work,
                           check=True)
            with np.load(out) as z:
                for k in z.files:
                    store[f"{name}/{k}"] = z[k]
            names.append(name)
    store["names"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "sim_to_wav.npz"), **store)


if __name__ == "__main__":
    if len(sys.argv) == 4:
        run_case(*sys.argv[1:])
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        sys.exit(__doc__)
