"""GPU: the GdmError texts of the wrappers over the DES-log and synth kernels (ops.des_log_to_roll, des_log_to_notes,
des_log_to_notes_pc, synth_windows, synth_windows_gm, and the plain tables check of synth_frames / synth_pcm).

The texts below were recorded with this file on the commit before the wrappers' checks were gathered into shared
helpers (``PYTHONPATH=. python tests/test_ops_error_texts_gpu.py`` prints the table), so they pin every message, and the
order of the checks, across that change and any later one.  Each case breaks one argument of a good call on tensors of
a few elements.  Every case is refused on the host: ``ops._call`` is wrapped and must not be reached.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402

N, B, DIM, ROWS, W, WIN = 4, 2, 3, 3, 2, 16


def _t(x, dtype):
    return torch.tensor(x, dtype=dtype, device="cuda")


def _strided(t):
    """The same values, not contiguous."""
    return torch.stack([t, t], dim=-1)[..., 0]


def _records():
    return dict(value=_t([0.5, 1.5, 2.5, 3.5], torch.float64), event_id=_t([3, 3, 5, 5], torch.int64),
                node=_t([0, 0, 1, 1], torch.int32), kind=_t([0, 1, 0, 1], torch.int32),
                rec_ptr=_t([0, 2, 4], torch.int64))


def _roll_args():
    return dict(_records(), tails=torch.full((B, 6), 0.5, dtype=torch.float32, device="cuda"),
                instruments=torch.zeros((B, DIM), dtype=torch.int32, device="cuda"),
                note_levels=torch.full((B, DIM), 60, dtype=torch.int32, device="cuda"),
                save=torch.ones(B, dtype=torch.int32, device="cuda"), start=0, end=50)


def _notes_args():
    return dict(_records(), note_levels=torch.full((B, DIM), 60, dtype=torch.int32, device="cuda"))


def _notes_pc_args():
    return dict(_records(), instruments=torch.zeros((B, DIM), dtype=torch.int32, device="cuda"),
                note_levels=torch.full((B, DIM), 60, dtype=torch.int32, device="cuda"))


def _windows_args(cols, bound):
    rows = [[10, 20, 60, 100, 0], [12, 30, 64, 90, 9], [40, 50, 67, 80, 17]]
    return {"notes": _t([r[:cols] for r in rows], torch.int64), bound: _t([20, 30, 50], torch.int64),
            "note_ptr": _t([0, ROWS], torch.int64), "win_clip": _t([0, 0], torch.int32),
            "win_start": _t([0, 8], torch.int64), "win_len": WIN}


def _frames_args():
    return dict(notes=torch.zeros((1, 2, 4), dtype=torch.int64, device="cuda"), n_notes=_t([0], torch.int32),
                clip_len=_t([0], torch.int64))


def _pcm_args():
    return dict(notes=torch.zeros((1, 2, 4), dtype=torch.int64, device="cuda"), n_notes=_t([0], torch.int32), first=0,
                count=8)


GOOD = {"des_log_to_roll": _roll_args, "des_log_to_notes": _notes_args, "des_log_to_notes_pc": _notes_pc_args,
        "synth_windows": lambda: _windows_args(4, "off_max"), "synth_windows_gm": lambda: _windows_args(5, "end_max"),
        "synth_frames": _frames_args, "synth_pcm": _pcm_args}


def _plain_tables(**bad):
    wave, inc = ops.synth_tables(torch.device("cuda"))
    return bad.get("wave", wave), bad.get("inc", inc)


def _gm_tables(**bad):
    waves, env, inc = ops.synth_gm_tables(torch.device("cuda"))
    return bad.get("waves", waves), bad.get("env", env), bad.get("inc", inc)


# what each case does to the good arguments: name -> (argument, function of the good value)
RECORD_BREAKS = {
    "value-dtype": ("value", lambda t: t.float()),
    "event_id-length": ("event_id", lambda t: t[:-1]),
    "node-noncontiguous": ("node", _strided),
    "kind-dtype": ("kind", lambda t: t.long()),
    "rec_ptr-dtype": ("rec_ptr", lambda t: t.int()),
    "rec_ptr-one-offset": ("rec_ptr", lambda t: t[:1]),
    "rec_ptr-noncontiguous": ("rec_ptr", _strided),
    "rec_ptr-descending": ("rec_ptr", lambda t: _t([0, 3, 2], torch.int64)),
    "rec_ptr-negative": ("rec_ptr", lambda t: _t([-1, 2, 4], torch.int64)),
    "rec_ptr-beyond": ("rec_ptr", lambda t: _t([0, 2, 5], torch.int64)),
}
ROLL_BREAKS = {
    "tails-dtype": ("tails", lambda t: t.double()),
    "tails-columns": ("tails", lambda t: t[:, :5].contiguous()),
    "instruments-dtype": ("instruments", lambda t: t.long()),
    "note_levels-rows": ("note_levels", lambda t: t[:1]),
    "save-shape": ("save", lambda t: t[:1]),
    "no-columns": ("end", lambda e: 0),
}
NOTES_BREAKS = {
    "note_levels-dtype": ("note_levels", lambda t: t.long()),
    "note_levels-rows": ("note_levels", lambda t: t[:1]),
    "note_levels-noncontiguous": ("note_levels", _strided),
}
NOTES_PC_BREAKS = dict(NOTES_BREAKS, **{
    "instruments-dtype": ("instruments", lambda t: t.long()),
    "instruments-shape": ("instruments", lambda t: t[:, :2].contiguous()),
})


def _window_breaks(bound, tables, table_breaks):
    breaks = {
        "notes-columns": ("notes", lambda t: t[:, :3].contiguous()),
        "notes-dtype": ("notes", lambda t: t.int()),
        "notes-noncontiguous": ("notes", _strided),
        "notes-1d": ("notes", lambda t: t.reshape(-1)),
        bound + "-length": (bound, lambda t: t[:-1]),
        bound + "-dtype": (bound, lambda t: t.int()),
        bound + "-noncontiguous": (bound, _strided),
        "note_ptr-dtype": ("note_ptr", lambda t: t.int()),
        "note_ptr-one-offset": ("note_ptr", lambda t: t[:1]),
        "note_ptr-noncontiguous": ("note_ptr", _strided),
        "win_clip-dtype": ("win_clip", lambda t: t.long()),
        "win_start-length": ("win_start", lambda t: t[:1]),
        "win_start-dtype": ("win_start", lambda t: t.int()),
        "win_clip-noncontiguous": ("win_clip", _strided),
        "out-dtype": ("out", lambda _: torch.zeros((W, WIN), dtype=torch.int32, device="cuda")),
        "out-rows": ("out", lambda _: torch.zeros((W + 1, WIN), dtype=torch.int16, device="cuda")),
        "out-1d": ("out", lambda _: torch.zeros(W * WIN, dtype=torch.int16, device="cuda")),
        "out-noncontiguous": ("out", lambda _: torch.zeros((W, 2 * WIN), dtype=torch.int16, device="cuda")[:, ::2]),
    }
    for name, bad in table_breaks.items():
        breaks["tables-" + name] = ("tables", lambda _, bad=bad: tables(**bad()))
    return breaks


_i16 = lambda *shape: torch.zeros(shape, dtype=torch.int16, device="cuda")  # noqa: E731
_i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
PLAIN_TABLE_BREAKS = {
    "wave-length": lambda: dict(wave=_i16(2047)),
    "wave-dtype": lambda: dict(wave=_i32(2048)),
    "wave-noncontiguous": lambda: dict(wave=_i16(4096)[::2]),
    "inc-length": lambda: dict(inc=_i32(127)),
    "inc-dtype": lambda: dict(inc=_i16(128)),
}
GM_TABLE_BREAKS = {
    "waves-shape": lambda: dict(waves=_i16(15, 2048)),
    "waves-dtype": lambda: dict(waves=_i32(16, 2048)),
    "env-shape": lambda: dict(env=_i32(16, 3)),
    "env-dtype": lambda: dict(env=_i16(16, 2)),
    "inc-length": lambda: dict(inc=_i32(127)),
    "waves-noncontiguous": lambda: dict(waves=_i16(16, 4096)[:, ::2]),
}
SYNTH_BREAKS = {"tables-" + name: ("tables", lambda _, bad=bad: _plain_tables(**bad()))
                for name, bad in PLAIN_TABLE_BREAKS.items()}

BREAKS = {
    "des_log_to_roll": dict(RECORD_BREAKS, **ROLL_BREAKS),
    "des_log_to_notes": dict(RECORD_BREAKS, **NOTES_BREAKS),
    "des_log_to_notes_pc": dict(RECORD_BREAKS, **NOTES_PC_BREAKS),
    "synth_windows": _window_breaks("off_max", _plain_tables, PLAIN_TABLE_BREAKS),
    "synth_windows_gm": _window_breaks("end_max", _gm_tables, GM_TABLE_BREAKS),
    "synth_frames": SYNTH_BREAKS,
    "synth_pcm": SYNTH_BREAKS,
}
CASES = [(wrapper, name) for wrapper, breaks in BREAKS.items() for name in breaks]

EXPECTED = {
    ('des_log_to_roll', 'value-dtype'):
        'des_log_to_roll: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_roll', 'event_id-length'):
        'des_log_to_roll: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_roll', 'node-noncontiguous'):
        'des_log_to_roll: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_roll', 'kind-dtype'):
        'des_log_to_roll: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_roll', 'rec_ptr-dtype'):
        'des_log_to_roll: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_roll', 'rec_ptr-one-offset'):
        'des_log_to_roll: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_roll', 'rec_ptr-noncontiguous'):
        'des_log_to_roll: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_roll', 'rec_ptr-descending'):
        'des_log_to_roll: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_roll', 'rec_ptr-negative'):
        'des_log_to_roll: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_roll', 'rec_ptr-beyond'):
        'des_log_to_roll: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_roll', 'tails-dtype'):
        'des_log_to_roll: tails must be (B, >= 6) fp32',
    ('des_log_to_roll', 'tails-columns'):
        'des_log_to_roll: tails must be (B, >= 6) fp32',
    ('des_log_to_roll', 'instruments-dtype'):
        'des_log_to_roll: instruments / note_levels must be contiguous (B, dim) int32',
    ('des_log_to_roll', 'note_levels-rows'):
        'des_log_to_roll: instruments / note_levels must be contiguous (B, dim) int32',
    ('des_log_to_roll', 'save-shape'):
        'des_log_to_roll: save must be a contiguous (B,) int32 tensor',
    ('des_log_to_roll', 'no-columns'):
        'des_log_to_roll: start=0, end=0 leave no columns',
    ('des_log_to_notes', 'value-dtype'):
        'des_log_to_notes: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes', 'event_id-length'):
        'des_log_to_notes: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes', 'node-noncontiguous'):
        'des_log_to_notes: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes', 'kind-dtype'):
        'des_log_to_notes: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes', 'rec_ptr-dtype'):
        'des_log_to_notes: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes', 'rec_ptr-one-offset'):
        'des_log_to_notes: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes', 'rec_ptr-noncontiguous'):
        'des_log_to_notes: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes', 'rec_ptr-descending'):
        'des_log_to_notes: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes', 'rec_ptr-negative'):
        'des_log_to_notes: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes', 'rec_ptr-beyond'):
        'des_log_to_notes: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes', 'note_levels-dtype'):
        'des_log_to_notes: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes', 'note_levels-rows'):
        'des_log_to_notes: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes', 'note_levels-noncontiguous'):
        'des_log_to_notes: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes_pc', 'value-dtype'):
        'des_log_to_notes_pc: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes_pc', 'event_id-length'):
        'des_log_to_notes_pc: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes_pc', 'node-noncontiguous'):
        'des_log_to_notes_pc: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes_pc', 'kind-dtype'):
        'des_log_to_notes_pc: records must be contiguous f64 / i64 / i32 / i32 arrays of one length',
    ('des_log_to_notes_pc', 'rec_ptr-dtype'):
        'des_log_to_notes_pc: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes_pc', 'rec_ptr-one-offset'):
        'des_log_to_notes_pc: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes_pc', 'rec_ptr-noncontiguous'):
        'des_log_to_notes_pc: rec_ptr must be a contiguous int64 tensor of B + 1 offsets',
    ('des_log_to_notes_pc', 'rec_ptr-descending'):
        'des_log_to_notes_pc: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes_pc', 'rec_ptr-negative'):
        'des_log_to_notes_pc: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes_pc', 'rec_ptr-beyond'):
        'des_log_to_notes_pc: rec_ptr must ascend within [0, 4] (the number of records)',
    ('des_log_to_notes_pc', 'note_levels-dtype'):
        'des_log_to_notes_pc: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes_pc', 'note_levels-rows'):
        'des_log_to_notes_pc: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes_pc', 'note_levels-noncontiguous'):
        'des_log_to_notes_pc: note_levels must be contiguous (B, dim) int32',
    ('des_log_to_notes_pc', 'instruments-dtype'):
        'des_log_to_notes_pc: instruments must be contiguous (B, dim) int32',
    ('des_log_to_notes_pc', 'instruments-shape'):
        'des_log_to_notes_pc: instruments must be contiguous (B, dim) int32',
    ('synth_windows', 'notes-columns'):
        'synth_windows: notes must be a contiguous (n, 4) int64 tensor',
    ('synth_windows', 'notes-dtype'):
        'synth_windows: notes must be a contiguous (n, 4) int64 tensor',
    ('synth_windows', 'notes-noncontiguous'):
        'synth_windows: notes must be a contiguous (n, 4) int64 tensor',
    ('synth_windows', 'notes-1d'):
        'synth_windows: notes must be a contiguous (n, 4) int64 tensor',
    ('synth_windows', 'off_max-length'):
        'synth_windows: off_max must be a contiguous (n,) int64 tensor',
    ('synth_windows', 'off_max-dtype'):
        'synth_windows: off_max must be a contiguous (n,) int64 tensor',
    ('synth_windows', 'off_max-noncontiguous'):
        'synth_windows: off_max must be a contiguous (n,) int64 tensor',
    ('synth_windows', 'note_ptr-dtype'):
        'synth_windows: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows', 'note_ptr-one-offset'):
        'synth_windows: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows', 'note_ptr-noncontiguous'):
        'synth_windows: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows', 'win_clip-dtype'):
        'synth_windows: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows', 'win_start-length'):
        'synth_windows: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows', 'win_start-dtype'):
        'synth_windows: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows', 'win_clip-noncontiguous'):
        'synth_windows: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows', 'out-dtype'):
        'synth_windows: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows', 'out-rows'):
        'synth_windows: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows', 'out-1d'):
        'synth_windows: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows', 'out-noncontiguous'):
        'synth_windows: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows', 'tables-wave-length'):
        'synth_windows: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_windows', 'tables-wave-dtype'):
        'synth_windows: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_windows', 'tables-wave-noncontiguous'):
        'synth_windows: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_windows', 'tables-inc-length'):
        'synth_windows: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_windows', 'tables-inc-dtype'):
        'synth_windows: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'notes-columns'):
        'synth_windows_gm: notes must be a contiguous (n, 5) int64 tensor',
    ('synth_windows_gm', 'notes-dtype'):
        'synth_windows_gm: notes must be a contiguous (n, 5) int64 tensor',
    ('synth_windows_gm', 'notes-noncontiguous'):
        'synth_windows_gm: notes must be a contiguous (n, 5) int64 tensor',
    ('synth_windows_gm', 'notes-1d'):
        'synth_windows_gm: notes must be a contiguous (n, 5) int64 tensor',
    ('synth_windows_gm', 'end_max-length'):
        'synth_windows_gm: end_max must be a contiguous (n,) int64 tensor',
    ('synth_windows_gm', 'end_max-dtype'):
        'synth_windows_gm: end_max must be a contiguous (n,) int64 tensor',
    ('synth_windows_gm', 'end_max-noncontiguous'):
        'synth_windows_gm: end_max must be a contiguous (n,) int64 tensor',
    ('synth_windows_gm', 'note_ptr-dtype'):
        'synth_windows_gm: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows_gm', 'note_ptr-one-offset'):
        'synth_windows_gm: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows_gm', 'note_ptr-noncontiguous'):
        'synth_windows_gm: note_ptr must be a contiguous int64 tensor of F + 1 offsets',
    ('synth_windows_gm', 'win_clip-dtype'):
        'synth_windows_gm: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows_gm', 'win_start-length'):
        'synth_windows_gm: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows_gm', 'win_start-dtype'):
        'synth_windows_gm: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows_gm', 'win_clip-noncontiguous'):
        'synth_windows_gm: win_clip (W,) int32 and win_start (W,) int64 must be contiguous and of one length',
    ('synth_windows_gm', 'out-dtype'):
        'synth_windows_gm: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows_gm', 'out-rows'):
        'synth_windows_gm: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows_gm', 'out-1d'):
        'synth_windows_gm: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows_gm', 'out-noncontiguous'):
        'synth_windows_gm: out must be a contiguous (2, out_stride) int16 tensor',
    ('synth_windows_gm', 'tables-waves-shape'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'tables-waves-dtype'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'tables-env-shape'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'tables-env-dtype'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'tables-inc-length'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_windows_gm', 'tables-waves-noncontiguous'):
        'synth_windows_gm: tables must be (waves int16 (16, 2048), env int32 (16, 2), inc int32[128] holding uint32 bits)',
    ('synth_frames', 'tables-wave-length'):
        'synth_frames: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_frames', 'tables-wave-dtype'):
        'synth_frames: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_frames', 'tables-wave-noncontiguous'):
        'synth_frames: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_frames', 'tables-inc-length'):
        'synth_frames: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_frames', 'tables-inc-dtype'):
        'synth_frames: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_pcm', 'tables-wave-length'):
        'synth_pcm: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_pcm', 'tables-wave-dtype'):
        'synth_pcm: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_pcm', 'tables-wave-noncontiguous'):
        'synth_pcm: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_pcm', 'tables-inc-length'):
        'synth_pcm: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
    ('synth_pcm', 'tables-inc-dtype'):
        'synth_pcm: tables must be (wave int16[2048], inc int32[128] holding uint32 bits)',
}


def _message(wrapper, name):
    """The text of the GdmError the broken call raises; nothing may reach ``ops._call``."""
    args = GOOD[wrapper]()
    key, how = BREAKS[wrapper][name]
    args[key] = how(args.get(key))
    launched = []
    call = ops._call
    ops._call = lambda fn, *a: launched.append(fn)
    try:
        with pytest.raises(ops.GdmError) as caught:
            getattr(ops, wrapper)(**args)
    finally:
        ops._call = call
    assert not launched, f"{wrapper} / {name}: {launched} was launched"
    return str(caught.value)


def test_the_good_calls_are_accepted():
    """The arguments the cases start from pass every check (the launch itself is not made here)."""
    call = ops._call
    try:
        for wrapper, good in GOOD.items():
            launched = []
            ops._call = lambda fn, *a, launched=launched: launched.append(fn)
            getattr(ops, wrapper)(**good())
            assert launched == ["gdm_" + wrapper], wrapper
    finally:
        ops._call = call


@pytest.mark.parametrize("wrapper,name", CASES, ids=[f"{w}-{n}" for w, n in CASES])
def test_error_text(wrapper, name):
    assert _message(wrapper, name) == EXPECTED[wrapper, name]


def test_every_shared_check_is_covered():
    """Dtype, length, contiguity and descending offsets of the records; column count and bound-column length of the
    windows; tables and out: each has a case for every wrapper that makes the check."""
    assert set(EXPECTED) == set(CASES) and len(CASES) == len(set(CASES))
    for wrapper in ("des_log_to_roll", "des_log_to_notes", "des_log_to_notes_pc"):
        assert set(RECORD_BREAKS) <= set(BREAKS[wrapper])
    for wrapper, bound in (("synth_windows", "off_max"), ("synth_windows_gm", "end_max")):
        assert {"notes-columns", bound + "-length", "out-dtype"} <= set(BREAKS[wrapper])
        assert any(name.startswith("tables-") for name in BREAKS[wrapper])
    assert len({text for text in EXPECTED.values()}) >= 30


if __name__ == "__main__":                       # record: prints the EXPECTED table of the checked-out commit
    print("EXPECTED = {")
    for wrapper, name in CASES:
        print(f"    ({wrapper!r}, {name!r}):\n        {_message(wrapper, name)!r},")
    print("}")
    test_the_good_calls_are_accepted()
