"""numpy / pure-Python restatement of the stand-alone demo path (gan_des_midi_music_gen_amd.simulation_to_wav) -- TEST
INFRASTRUCTURE ONLY.

  * the draws and the matrix prologue of SIMULATOR/simulation_to_wav.py:12-77 in numpy float64 (pinned by
    tests/golden/sim_to_wav.npz, recorded from the reference itself);
  * the demo's MidiGenerator.process_line (:162-214) over event records -> the message rows it appends, program_change
    lines included, and the five-column note rows cut from them (pinned by the same file);
  * the integer synth with 16 timbres as include/gdm.h defines it (gdm_synth_windows_gm), per sample in int64.  Nothing
    upstream pins the synth; the kernels are held to this mirror bit for bit.

``fault=`` plants a deliberate error so that the tests can show the fixture catches it.
"""
import hashlib

import numpy as np

import des_notes_ref

NUM_AUG = 5
NOTE_ON, NOTE_OFF, PROGRAM_CHANGE = 0, 1, 2          # row types of the fixture
OK, ENODE, EPITCH, ELONG, EPROGRAM = 0, 1, 2, 3, 4   # GDM_DES_NOTES_E*
RATE, WAVE_LEN, SHIFT = 44100, 2048, 30
TICK_MUL, TICK_DIV = 735, 16                         # tempo 500 000 (no set_tempo in the file), 480 ticks per beat
MAX_SAMPLES = 1 << 40
FAMILIES = (  # (w1..w4 in sixteenths, a_f): include/gdm.h / the issue's table
    ((16, 8, 4, 2), 8), ((16, 0, 6, 0), 6), ((16, 12, 8, 4), 10), ((16, 10, 6, 3), 7), ((16, 5, 0, 0), 8),
    ((16, 8, 5, 4), 12), ((16, 6, 4, 2), 12), ((16, 12, 10, 6), 10), ((16, 2, 10, 1), 9), ((16, 2, 0, 0), 10),
    ((16, 8, 6, 4), 6), ((16, 4, 0, 2), 13), ((16, 0, 0, 8), 11), ((16, 9, 2, 6), 7), ((16, 3, 9, 1), 5),
    ((8, 16, 4, 12), 9))
TAIL = max(1 << (21 - a) for _w, a in FAMILIES)      # samples a clip lasts beyond its last note_off
PROLOGUE_FAULTS = ("mul_126", "sum_dim")
ROW_FAULTS = ("single_delta",)


class Refused(ValueError):
    """A row sum is zero or not finite: the package refuses the sample (status 1)."""


# ---- draws and prologue ----------------------------------------------------------------------------------------------
def draw_matrix(size, rand=None):
    """Lines 12-22 on ``rand`` (default: numpy's global ``np.random.rand``)."""
    rand = np.random.rand if rand is None else rand
    dim = size - NUM_AUG
    m = rand(size, size)
    m[dim:, :] = 0
    m[:, dim:] = 0
    for r in range(NUM_AUG):
        m[dim + r, :dim] = rand(dim)
    return m


def reseed_pair(rs=None):
    """Lines 76-77.  rs=None: on the global stream (which is reseeded); a RandomState: on it, returning the state the
    simulation starts from as well -> (seeds, state or None)."""
    if rs is None:
        np.random.seed(np.random.randint(0, 99999, size=1))
        return np.random.randint(0, 99999, size=1), None
    inner = np.random.RandomState(rs.randint(0, 99999, size=1))
    seeds = inner.randint(0, 99999, size=1)
    return seeds, inner.get_state()


def prologue(matrix, use_same_instrument=None, fault=None):
    """Lines 25-71 for one (size, size) float64 matrix (not modified) -> dict of src (dim) bool, instruments,
    note_levels (dim) int64, loc, scale (dim) float64, queue_list, adj (dim, dim) float64.  Raises Refused."""
    assert fault is None or fault in PROLOGUE_FAULTS
    m = np.array(matrix, dtype=np.float64)
    size = m.shape[0]
    assert m.shape == (size, size)
    dim = size - NUM_AUG
    mul = 126 if fault == "mul_126" else 127
    col_src = m[dim] > 0.75                                   # every column, the parameter columns included
    src = col_src[:dim].copy()
    if use_same_instrument is None:
        instruments = np.array([int(m[dim + 1, i] * mul) for i in range(dim)], dtype=np.int64)
    else:
        instruments = np.array([use_same_instrument] * dim, dtype=np.int64)
    note_levels = np.array([int(m[dim + 2, i] * mul) for i in range(dim)], dtype=np.int64)
    loc = np.array([(10 if src[i] else 3) * m[dim + 3, i] for i in range(dim)], dtype=np.float64)
    scale = np.array([(5 if src[i] else 2) * m[dim + 4, i] for i in range(dim)], dtype=np.float64)
    m[:, col_src] = 0
    for i in range(size):
        m[i, i] = 0
    for i in range(dim):
        row = m[i, :dim] if fault == "sum_dim" else m[i]
        total = 0
        for x in row:                                         # Python's sum(): sequential, left to right
            total = total + x
        if total == 0 or not np.isfinite(total):
            raise Refused(f"row {i} sums to {total!r}")
        m[i] = m[i] / total
    for i in range(dim):
        m[i, i] = 1.0 if src[i] else -1.0
    return {"src": src, "instruments": instruments, "note_levels": note_levels, "loc": loc, "scale": scale,
            "queue_list": [127] * size, "adj": np.ascontiguousarray(m[:dim, :dim])}


# ---- log -> messages -> notes ----------------------------------------------------------------------------------------
def log_rows(log, instruments, note_levels, fault=None):
    """Event records -> the (type, a, velocity, time) rows the demo's MidiGenerator appends (:162-214): per sounded
    departure program_change(on), note_on(on), program_change(off), note_off(off).  The reader (5000 lines, the regex
    decided numerically by des_notes_ref.line_matches) and the queue / customer-id folds are those of the GAN_DES copy."""
    assert fault is None or fault in ROW_FAULTS
    progs, notes = [int(x) for x in instruments], [int(x) for x in note_levels]
    value, event_id, node, kind = log["value"], log["event_id"], log["node"], log["kind"]
    queue, future, rows = {}, {}, []
    for r in range(min(len(value), des_notes_ref.MAX_LINES)):
        eid, nd, kd = int(event_id[r]), int(node[r]), int(kind[r])
        if not des_notes_ref.line_matches(value[r], eid, nd, kd):
            continue
        if not (eid % 3 == 0 or eid % 5 == 0 or eid % 7 == 0):
            continue
        midi_time = max(0, int(float(value[r])))
        if kd == des_notes_ref.ARRIVAL:
            q = queue[nd] = queue.get(nd, 0) + 1
            if 127 <= q < 254:
                q = min(127, max(0, 254 - q))
            elif q >= 254:
                q = min(127, max(0, q % 127))
            max_id = max(1, (30 + q) % 127)
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
                    raise des_notes_ref.LogError(f"node {nd} has no instrument")
                if not 0 <= progs[nd] <= 127:
                    raise des_notes_ref.LogError(f"program {progs[nd]} out of range")
                if not 0 <= notes[nd] <= 127:
                    raise des_notes_ref.LogError(f"note {notes[nd]} out of range")
                on, off = max(0, t0), max(0, t0 + (midi_time - t0) + max(0, service))
                if fault != "single_delta":
                    rows.append((PROGRAM_CHANGE, progs[nd], 0, on))
                rows.append((NOTE_ON, notes[nd], vel, on))
                if fault != "single_delta":
                    rows.append((PROGRAM_CHANGE, progs[nd], 0, off))
                rows.append((NOTE_OFF, notes[nd], vel, off))
            queue[nd] = queue[nd] - 1 if nd in queue else 0
    return rows


def tick_to_sample(tick):
    return int(tick) * TICK_MUL // TICK_DIV


MAX_TICK = (MAX_SAMPLES - TAIL) * TICK_DIV // TICK_MUL


def rows_to_notes(rows):
    """Message rows (delta ticks) -> (notes (n, 5) int64 of (on_tick, off_tick, pitch, velocity, program), clip_len in
    samples, status): the program in force at the note_on, every delta counted."""
    out, t, prog, on_tick = [], 0, 0, None
    for typ, a, vel, delta in rows:
        if delta > MAX_TICK - t:
            return np.zeros((0, 5), np.int64), 0, ELONG
        t += delta
        if typ == PROGRAM_CHANGE:
            prog = a
        elif typ == NOTE_ON:
            on_tick, on_prog = t, prog
        else:
            out.append((on_tick, t, a, vel, on_prog))
    notes = np.asarray(out, dtype=np.int64).reshape(-1, 5)
    return notes, (tick_to_sample(notes[-1, 1]) + TAIL if len(out) else 0), OK


def track_of(rows):
    """The (kind, a, b, time) track of the demo's file: no header (generate_midi is never called), kinds as
    include/gdm.h's GDM_MIDI_*."""
    kinds = {PROGRAM_CHANGE: 3, NOTE_ON: 4, NOTE_OFF: 5}
    return [(kinds[r[0]], r[1], r[2], r[3]) for r in rows]


def notes_in_samples(notes):
    """Tick rows -> the rows gdm_synth_windows_gm takes."""
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 5).copy()
    notes[:, 0] = notes[:, 0] * TICK_MUL // TICK_DIV
    notes[:, 1] = notes[:, 1] * TICK_MUL // TICK_DIV
    return notes


def records_sha256(log):
    h = hashlib.sha256()
    for name, dt in (("value", "<f8"), ("event_id", "<i8"), ("node", "<i4"), ("kind", "<i4")):
        h.update(np.ascontiguousarray(log[name]).astype(dt).tobytes())
    return h.hexdigest()


# ---- the synth with timbres --------------------------------------------------------------------------------------------
def gm_tables():
    """(waves int16 (16, 2048), env int64 (16, 2) = (A_f, R_f), inc uint32[128]) in float64, as include/gdm.h says."""
    i = np.arange(WAVE_LEN, dtype=np.float64)
    waves, env = [], []
    for weights, a in FAMILIES:
        s = np.zeros(WAVE_LEN, dtype=np.float64)
        for k, w in enumerate(weights, start=1):
            s = s + float(w) * np.sin(2.0 * np.pi * k * i / WAVE_LEN)
        waves.append(np.rint(32767.0 * s / np.abs(s).max()).astype(np.int16))
        env.append((1 << a, 1 << (21 - a)))
    return np.stack(waves), np.asarray(env, dtype=np.int64), des_notes_ref.tables()[1]


_TABLES = gm_tables()


def end_max(notes, env=None):
    """The running maximum of s_off + R_family over one clip's rows."""
    env = _TABLES[1] if env is None else np.clip(np.asarray(env, dtype=np.int64), 1, 1 << 21)
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 5)
    return np.maximum.accumulate(notes[:, 1] + env[(notes[:, 4] & 127) >> 3, 1]) if len(notes) else np.zeros(0, np.int64)


def voice_sum(notes, start, count, tables=None):
    """int64 (count,): the unclamped sum of the voices at samples start .. start + count (rows in samples)."""
    waves, env, inc = _TABLES if tables is None else tables
    waves = np.asarray(waves).astype(np.int64)
    env = np.clip(np.asarray(env, dtype=np.int64), 1, 1 << 21)
    s = np.arange(start, start + count, dtype=np.int64)
    total = np.zeros(count, dtype=np.int64)
    for s_on, s_off, pitch, vel, prog in np.asarray(notes, dtype=np.int64).reshape(-1, 5).tolist():
        f = (prog & 127) >> 3
        att, rel = int(env[f, 0]), int(env[f, 1])
        a, b = max(s_on, start), min(s_off + rel, start + count)
        if a >= b:
            continue
        t = s[a - start:b - start]
        d = t - s_on
        phase = (d * int(inc[pitch & 127])) & 0xFFFFFFFF
        e_att = np.minimum(d + 1, att)
        e_rel = np.where(t < s_off, rel, rel - (t - s_off))
        total[a - start:b - start] += (waves[f][phase >> 21] * (vel & 127) * e_att * e_rel) >> SHIFT
    return total


def window(notes, start, count, tables=None):
    total = voice_sum(notes, start, count, tables)
    assert np.abs(total).max(initial=0) < 1 << 31, "the kernel's int32 sum would overflow"
    return np.clip(total, -32768, 32767).astype(np.int16)


def render(notes_ticks, clip_len, max_seconds=None):
    """The samples of the WAV file sim_to_wav writes for a clip: its notes in ticks, its length; a clip without notes is
    the blank clip of datasets.midi_notes (5 s of silence)."""
    total = clip_len if len(notes_ticks) else 5 * RATE
    if max_seconds is not None:
        total = max(1, min(total, int(max_seconds * RATE)))
    if not len(notes_ticks):
        return np.zeros(total, dtype=np.int16)
    return window(notes_in_samples(notes_ticks), 0, total)
