"""Drop-in surface of the DES log -> MIDI -> piano-roll consumer (MMGAN_MIDI_DES/sim_log_to_midi.py) on MI355X.

    process_adjsim_log(n=5000, baseline=70, range=50, instruments=..., note_levels=..., gen2_output=None, count=0,
                       start=0, end=30, generate=False, *, log=None)                    sim_log_to_midi.py:241-277
    log_to_rolls(logs, gen2_tails, instruments, note_levels, ...)      batched device form: B samples, ONE launch
    write_midi(track, path, ticks_per_beat=480) / track_bytes(track)   Standard MIDI File writer (what mido's save does)

The reference reads ``./logs/simulation.log`` line by line, feeds the lines its regex matches to ``MidiGenerator``,
saves a ``.mid`` file when ``generate`` is set or the line count is a multiple of 100, and runs ``generate_piano_roll``
on the in-memory file.  Here the whole chain -- reader, MidiGenerator.process_line, save_midi / clean_midi_file, the
tick -> second -> step conversion and the raster -- is one HIP kernel over the DES core's event RECORDS
(``simulation_v3.EVENT_DTYPE``; csrc/des_midi.hip, ``ops.des_log_to_roll``): one workgroup per sample, the planes
written straight into the discriminator's (B, 2, 128, W) input.  The host only packs the records and, where a file is
wanted, writes the returned track out.

Kept as upstream: only the first 5000 lines are looked at; a sample whose file is not saved has a MidiFile without
tracks and therefore all-zero planes; message times are absolute-looking values that mido reads as DELTA ticks;
``range`` / ``baseline`` / ``n`` are accepted and unused (the reference only uses them for random note levels when
``note_levels`` is None -- here both lists are required).  ``float32 * int`` products of the parameter block are
rounded to float32 before ``int()`` (NumPy >= 2 scalar promotion; tests/golden/des_midi.npz was recorded under it).
The ``np.random.randint`` fallbacks of MidiGenerator.__init__ are unreachable and not built.

``beats`` (third return value) is ``pretty_midi.PrettyMIDI(...).get_beats()`` of the saved file padded to 50, through
``datasets.get_beats`` -- pretty_midi is not available to check against: PARITY UNPINNED, as for datasets.py.
"""
import os
import re
import struct

import numpy as np
import torch

from . import datasets, ops
from .simulation_v3 import EVENT_DTYPE, KIND_NAMES

SET_TEMPO, TIME_SIGNATURE, KEY_SIGNATURE, PROGRAM_CHANGE, NOTE_ON, NOTE_OFF, END_OF_TRACK = range(7)   # GDM_MIDI_*
KEYS = ('C', 'C#', 'D', 'E', 'F', 'F#', 'G', 'G#m', 'A', 'A#m', 'B')
# key name -> (sharps (+) / flats (-), minor) of the key_signature meta message
_KEY_BYTES = {'C': (0, 0), 'C#': (7, 0), 'D': (2, 0), 'E': (4, 0), 'F': (-1, 0), 'F#': (6, 0), 'G': (1, 0),
              'G#m': (5, 1), 'A': (3, 0), 'A#m': (7, 1), 'B': (5, 0)}
MAX_LINES = 5000
LOG_REGEX = r"INFO:root:([0-9]*\.[0-9]+|[0-9]+) - ([0-9]*\.[0-9]+|[0-9]+) - ([0-9]*\.[0-9]+|[0-9]+) - (arrival|departure)"
_UNMATCHED = -1          # kind of a text line the regex does not match: counted as a line, never processed


def lines_read(n_lines):
    """``count`` after the reference's reader loop: it breaks on the 5001st line."""
    return min(int(n_lines), MAX_LINES + 1)


def parse_log(path="./logs/simulation.log"):
    """Text log -> EVENT_DTYPE records, one per line (so the line count survives); lines the reference's regex does not
    match get kind -1.  Only the first 5001 lines are read.

    The regex decision is made HERE for a text log; the kernel decides again, numerically, from the record's value
    (for records straight from the DES core there is no text).  The two agree for values printed by ``repr``, which is
    what the simulator writes.  A hand-written line may spell a value the regex accepts although ``repr`` would have
    used an exponent for it -- ``0.00001`` or a 17-digit integer: upstream processes it with
    ``midi_time = int(float(text))``, so such a value is replaced by one the kernel accepts with the same outcome
    (below 1e-4: 0.0, midi_time 0; from 1e16 up: 1e15, which fails ``midi_time < 200`` like the original).  An event
    id or node spelt with a decimal point makes upstream raise as soon as the line is processed (``int('3.0')``, a
    dict key '3.0'); here it raises ValueError when the file is read."""
    rx = re.compile(LOG_REGEX)
    rows = []
    with open(path, "r") as f:
        for line in f:
            m = rx.match(line)
            if m:
                if "." in m.group(2) or "." in m.group(3):
                    raise ValueError(f"Error in processing log file (event id / node not an integer: {line.strip()!r})")
                value = float(m.group(1))
                if 0.0 < value < 1e-4:
                    value = 0.0
                elif value >= 1e16:
                    value = 1e15
                rows.append((value, int(m.group(2)), int(m.group(3)), KIND_NAMES.index(m.group(4))))
            else:
                rows.append((0.0, 0, 0, _UNMATCHED))
            if len(rows) > MAX_LINES:
                break
    return np.array(rows, dtype=EVENT_DTYPE)


def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def track_bytes(track, ticks_per_beat=480):
    """(kind, a, b, time) messages -> the bytes of a type-1, one-track Standard MIDI File, laid out as mido's
    ``MidiFile.save`` does: delta time as a variable-length quantity, meta messages in full, channel messages with
    running status, an end_of_track appended if the track does not end in one."""
    track = [tuple(int(x) for x in m) for m in np.asarray(track).reshape(-1, 4)]
    if not track or track[-1][0] != END_OF_TRACK:
        track = track + [(END_OF_TRACK, 0, 0, 0)]
    body, running = bytearray(), None
    for kind, a, b, time in track:
        if time < 0:
            raise ValueError("message time must be non-negative")
        body += _vlq(time)
        if kind == SET_TEMPO:
            body += b"\xff\x51\x03" + a.to_bytes(3, "big")
        elif kind == TIME_SIGNATURE:
            body += bytes([0xFF, 0x58, 4, a, b.bit_length() - 1, 24, 8])
        elif kind == KEY_SIGNATURE:
            sf, minor = _KEY_BYTES[KEYS[a]]
            body += bytes([0xFF, 0x59, 2, sf & 0xFF, minor])
        elif kind == END_OF_TRACK:
            body += b"\xff\x2f\x00"
        else:
            status, data = {PROGRAM_CHANGE: (0xC0, (a,)), NOTE_ON: (0x90, (a, b)), NOTE_OFF: (0x80, (a, b))}[kind]
            if status != running:
                body.append(status)
            body += bytes(data)
            running = status
            continue
        running = None
    return b"MThd" + struct.pack(">IHHH", 6, 1, 1, ticks_per_beat) + b"MTrk" + struct.pack(">I", len(body)) + bytes(body)


def write_midi(track, path, ticks_per_beat=480):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(track_bytes(track, ticks_per_beat))
    return path


def _int_rows(rows, dim_name):
    out = np.ascontiguousarray([[int(x) for x in np.asarray(r).reshape(-1)] for r in rows], dtype=np.int32)
    if out.ndim != 2 or out.shape[1] == 0:
        raise ops.GdmError(f"{dim_name} must hold one equally long list per sample")
    return out


def _upload_logs(logs, device, who):
    """What both batched consumers do with B event logs (``who`` names the caller in messages): checks, then
    -> (logs as arrays, device, ``up`` (host array -> device tensor), ``records``).  ``records()`` uploads the CSR form
    the kernels take -- value, event_id, node, kind of the lines the reader looks at, and rec_ptr (B + 1)."""
    if len(logs) == 0:
        raise ops.GdmError(f"{who}: no samples")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ops.GdmError(f"{who} runs on a HIP device; there is no CPU path")
    logs = [np.asarray(lg) for lg in logs]
    for lg in logs:
        if lg.dtype != EVENT_DTYPE or lg.ndim != 1:
            raise ops.GdmError(f"{who}: every log must be a 1-d simulation_v3.EVENT_DTYPE array")

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def records():
        heads = [lg[:MAX_LINES] for lg in logs]              # what the reader looks at; the rest never crosses
        rec_ptr = np.zeros(len(logs) + 1, dtype=np.int64)
        np.cumsum([len(h) for h in heads], out=rec_ptr[1:])
        rec = np.concatenate(heads) if rec_ptr[-1] else np.zeros(0, dtype=EVENT_DTYPE)
        return up(rec["value"]), up(rec["event_id"]), up(rec["node"]), up(rec["kind"]), up(rec_ptr)

    return logs, dev, up, records


def log_to_rolls(logs, gen2_tails, instruments, note_levels, *, start=0, end=30, generate=False, save=None,
                 sequence_length=100, device="cuda", return_saved=False, return_status=False, raise_for_status=True):
    """B event logs -> (rolls (B, 2, 128, W) fp32 DEVICE tensor, tracks): one ``des_log_to_roll`` launch.

    logs: B ``EVENT_DTYPE`` arrays (``Sim.music_log``); gen2_tails: (B, >= 6) ``gen2_output[:, 10:]``; instruments,
    note_levels: B lists of ``dim`` numbers (``int()`` is applied, as upstream).  save: per-sample override of the
    reference's decision ``generate or line count % 100 == 0``.  tracks[i]: (n, 4) int32 (kind, a, b, time) -- the saved
    track, or the track as process_line left it when sample i is not saved (its planes are zero then).
    A sample the reference would raise for raises ValueError here -- unless raise_for_status is False; return_status
    adds the (B,) status words (error code in bits 8 and up, ``ops.DES_MIDI_ERRORS``) to the result."""
    logs, dev, up, records = _upload_logs(logs, device, "log_to_rolls")
    b = len(logs)
    tails = np.ascontiguousarray(gen2_tails.detach().float().cpu().numpy() if torch.is_tensor(gen2_tails)
                                 else np.asarray(gen2_tails, dtype=np.float32))
    if tails.ndim != 2 or tails.shape[0] != b or tails.shape[1] < 6:
        raise ops.GdmError("log_to_rolls: gen2_tails must be (B, >= 6): gen2_output[:, 10:]")
    inst, notes = _int_rows(instruments, "instruments"), _int_rows(note_levels, "note_levels")
    if inst.shape != notes.shape or inst.shape[0] != b:
        raise ops.GdmError("log_to_rolls: instruments and note_levels must both be (B, dim)")
    if save is None:
        save = [bool(generate) or lines_read(len(lg)) % 100 == 0 for lg in logs]
    save = np.ascontiguousarray(save, dtype=np.int32)
    if save.shape != (b,):
        raise ops.GdmError("log_to_rolls: save must hold one flag per sample")
    planes, track, track_len, status = ops.des_log_to_roll(*records(), up(tails), up(inst), up(notes), up(save), start,
                                                           end, sequence_length)
    status, track_len, track = status.cpu().numpy(), track_len.cpu().numpy(), track.cpu().numpy()
    for i in range(b):
        if status[i] >> 8 and raise_for_status:
            raise ValueError(f"Error in processing log file (sample {i}: {ops.DES_MIDI_ERRORS[int(status[i]) >> 8]})")
    tracks = [track[i, :track_len[i]].copy() for i in range(b)]
    if return_status:
        return planes, tracks, status
    if return_saved:
        return planes, tracks, [bool(s & 1) for s in status]
    return planes, tracks


def process_adjsim_log(n=5000, baseline=70, range=50, instruments=None, note_levels=None, gen2_output=None, count=0,
                       start=0, end=30, generate=False, *, log=None, device="cuda", midi_path=None):
    """Reference signature + ``log`` (an EVENT_DTYPE array; None: ``./logs/simulation.log`` is parsed with the
    reference's regex).  Returns numpy (piano_roll, durations (128, W) float64, beats (50,)) like upstream, and writes
    ``./adj_sim_outputs/midi/generation.mid`` (generate) or ``.../simulation.mid`` (line count a multiple of 100) --
    ``midi_path`` overrides the location."""
    if gen2_output is None or instruments is None or note_levels is None:
        raise ops.GdmError("process_adjsim_log: gen2_output (gen2_output[10:]), instruments and note_levels are required")
    if log is None:
        log = parse_log("./logs/simulation.log")
    tail = np.asarray(gen2_output.detach().cpu().numpy() if torch.is_tensor(gen2_output) else gen2_output,
                      dtype=np.float32).reshape(1, -1)
    planes, tracks, saved = log_to_rolls([log], tail, [instruments], [note_levels], start=start, end=end,
                                         generate=generate, device=device, return_saved=True)
    beats = np.zeros(0)
    if saved[0]:
        data = track_bytes(tracks[0])
        path = midi_path or ("./adj_sim_outputs/midi/generation.mid" if generate else
                             "./adj_sim_outputs/midi/simulation.mid")
        write_midi(tracks[0], path)
        beats = datasets.get_beats(datasets.read_midi(data))
    p = planes[0].double().cpu().numpy()
    return p[0], p[1], datasets._fit_beats(beats, 50)
