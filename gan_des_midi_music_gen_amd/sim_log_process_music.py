"""Drop-in surface of model 1's DES log -> MIDI consumer (GAN_DES/sim_log_process_music.py) on MI355X.

    process_adjsim_log(n=5000, baseline=70, range=50, instruments=..., note_levels=..., *, log=None, midi_path=None)
                                                                        sim_log_process_music.py:159-185
    log_to_notes(logs, instruments, note_levels, device=...)            batched device form: B samples, ONE launch

The reference reads ``./logs/simulation.log`` line by line (5000 lines at most), feeds the lines its regex matches to
``MidiGenerator.process_line`` (:65-133) and saves the track as ``./adj_sim_outputs/midi/output.mid``, which FluidSynth
then renders.  Here reader and process_line are one HIP kernel over the DES core's event RECORDS
(``simulation_v3.EVENT_DTYPE``; csrc/des_notes.hip, ``ops.des_log_to_notes``): one workgroup per sample, and the result
is the NOTE LIST the synth kernels consume (csrc/synth.hip) -- per note (on_tick, off_tick, pitch, velocity), the ticks
being the cumulative delta times of the track as mido reads it.  On the batched path nothing returns to the host but
the B status words.

Kept as upstream: only the first 5000 lines are looked at; the event-id filter is the fixed 3 / 5 / 7; a node's
``future_events`` entry is never cleared, so every later departure of the node sounds its note again; ``queue_lengths``
goes negative; message times are absolute-looking values that mido reads as DELTA ticks; ``n`` / ``baseline`` /
``range`` are accepted and unused, and so is ``instruments`` beyond ``int()`` (its program_change lines are commented
out upstream).  The reference tests ``note_levels != []`` on a numpy array, which raises under NumPy >= 2: the behaviour
of the NumPy it was written for is followed, the lists are used (both are required here; the ``random.randint``
fallbacks for empty lists are not built).  The written file holds generate_midi's four header messages (set_tempo
1 000 000, 4/4, key C, program 0) in front of the notes -- the tempo the synth's tick length assumes.
"""
import numpy as np

from . import ops, sim_log_to_midi

MAX_LINES = sim_log_to_midi.MAX_LINES
HEADER = ((sim_log_to_midi.SET_TEMPO, 1000000, 0, 0), (sim_log_to_midi.TIME_SIGNATURE, 4, 4, 0),
          (sim_log_to_midi.KEY_SIGNATURE, 0, 0, 0), (sim_log_to_midi.PROGRAM_CHANGE, 0, 0, 0))


def stage_notes(logs, instruments, note_levels, device="cuda"):
    """``log_to_notes`` without its read-back: -> (notes, n_notes, clip_len, status) device tensors, nothing waited for.
    The caller enqueues what consumes them and calls ``raise_for_status(status)`` afterwards (a sample with an error
    status has no notes, so it is a blank clip to every later stage)."""
    logs, _dev, up, records = sim_log_to_midi._upload_logs(logs, device, "log_to_notes")
    inst = sim_log_to_midi._int_rows(instruments, "instruments")        # int() of every entry, as upstream; unused after
    notes = sim_log_to_midi._int_rows(note_levels, "note_levels")
    if inst.shape[0] != len(logs) or notes.shape[0] != len(logs):
        raise ops.GdmError("log_to_notes: instruments and note_levels must hold one list per sample")
    return ops.des_log_to_notes(*records(), up(notes))


def raise_for_status(status):
    """ValueError for the first sample the reference would raise for (the one read-back of the path: B status words)."""
    for i, code in enumerate(status.cpu().tolist()):
        if code in ops.DES_NOTES_ERRORS:
            raise ValueError(f"Error in processing log file (sample {i}: {ops.DES_NOTES_ERRORS[code]})")


def log_to_notes(logs, instruments, note_levels, device="cuda"):
    """B event logs -> (notes (B, 5000, 4) int64, n_notes (B,) int32, clip_len (B,) int64): one ``des_log_to_notes``
    launch, everything stays on the device.

    logs: B ``EVENT_DTYPE`` arrays (``Sim.music_log``); instruments, note_levels: B lists of ``dim`` numbers (``int()``
    is applied, as upstream).  clip_len is the clip's length in samples at 44 100 Hz (0: a blank clip -- no notes, or
    a clip that would pass 2^40 samples).  A sample the reference would raise for raises ValueError here."""
    notes, n_notes, clip_len, status = stage_notes(logs, instruments, note_levels, device)
    raise_for_status(status)
    return notes, n_notes, clip_len


def notes_to_track(notes):
    """(n, 4) (on_tick, off_tick, pitch, velocity) -> the (kind, a, b, delta time) track ``write_midi`` takes: the four
    header messages, then note_on / note_off per note."""
    track, t = list(HEADER), 0
    for on, off, pitch, vel in np.asarray(notes, dtype=np.int64).reshape(-1, 4).tolist():
        track.append((sim_log_to_midi.NOTE_ON, pitch, vel, on - t))
        track.append((sim_log_to_midi.NOTE_OFF, pitch, vel, off - on))
        t = off
    return track


def process_adjsim_log(n=5000, baseline=70, range=50, instruments=None, note_levels=None, *, log=None, device="cuda",
                       midi_path=None):
    """Reference signature + ``log`` (an EVENT_DTYPE array; None: ``./logs/simulation.log`` is parsed with the
    reference's regex) and ``midi_path`` (default: upstream's ``./adj_sim_outputs/midi/output.mid``).  Writes the MIDI
    file and returns its path."""
    if instruments is None or note_levels is None:
        raise ops.GdmError("process_adjsim_log: instruments and note_levels are required")
    if log is None:
        log = sim_log_to_midi.parse_log("./logs/simulation.log")
    notes, n_notes, _clip_len = log_to_notes([log], [instruments], [note_levels], device=device)
    path = midi_path or "./adj_sim_outputs/midi/output.mid"
    return sim_log_to_midi.write_midi(notes_to_track(notes[0, :int(n_notes[0])].cpu().numpy()), path)
