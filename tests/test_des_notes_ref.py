"""CPU: the restatement of model 1's DES bridge (tests/des_notes_ref.py).  Its note stage is held to rows recorded from
the reference's own reader and MidiGenerator (tests/golden/des_notes.npz, recorder: make_des_notes_golden.py); its synth
is checked for the properties the kernels rely on (frames = PCM cut by the reflect rule, the overflow bounds)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import des_notes_ref as N  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "des_notes.npz"))
CORE = np.load(os.path.join(HERE, "golden", "des_core.npz"))
NAMES = [str(n) for n in GOLD["names"]]
FIELDS = ("value", "event_id", "node", "kind")


def case_log(name):
    if f"{name}/log" in GOLD.files:
        log, n = str(GOLD[f"{name}/log"]), int(GOLD[f"{name}/n_lines"])
        return {k: CORE[f"{log}/{k}"][:n] for k in FIELDS}
    return {k: GOLD[f"{name}/{k}"] for k in FIELDS}


def rows_of(name, fault=None):
    return np.asarray(N.log_rows(case_log(name), GOLD[f"{name}/note_levels"], fault), dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("name", NAMES)
def test_note_mirror_equals_recorded_rows(name):
    assert np.array_equal(rows_of(name), GOLD[f"{name}/rows"])


def test_fixture_reaches_the_branches():
    n = {name: len(GOLD[f"{name}/rows"]) // 2 for name in NAMES}
    assert n["wav0_5001_lines"] == 870 and n["wav1_5001_lines"] == 955          # the figures of the design note
    assert int(GOLD["wav0_5001_lines/rows"][:, 3].sum()) == 66514 and int(GOLD["wav1_5001_lines/rows"][:, 3].sum()) == 72011
    assert n["repeated_departures"] == 3 and n["lines_5003"] == 0 and len(case_log("lines_5003")["value"]) == 5003
    folds = GOLD["queue_folds/rows"]
    service = folds[1::2, 3] - (3 * np.arange(300) + 2)         # off time = departure time + folded count (i + 2)
    assert n["queue_folds"] == 300 and service.max() == 127
    assert service[[124, 125, 126, 251, 252, 253]].tolist() == [126, 127, 126, 1, 0, 1]
    assert n["values"] == 3 and n["ids_filtered"] == 1 and n["customer_id_folds"] == 13
    assert len(set(GOLD["customer_id_folds/rows"][::2, 2].tolist())) > 6


@pytest.mark.parametrize("fault,where", [("fold_boundary", "queue_folds"), ("c_modulo", "departures_first"),
                                         ("clear_future", "repeated_departures"), ("read_5001", "lines_5003")])
def test_planted_faults_are_caught(fault, where):
    assert not np.array_equal(rows_of(where, fault), GOLD[f"{where}/rows"])
    caught = [name for name in NAMES if not np.array_equal(rows_of(name, fault), GOLD[f"{name}/rows"])]
    assert where in caught


def test_rows_to_notes_and_limits():
    rows = [tuple(int(x) for x in r) for r in GOLD["departures_first/rows"]]
    notes, clip_len, status = N.rows_to_notes(rows)
    assert status == N.OK and notes.shape == (2, 4) and (np.diff(notes[:, :2].ravel()) >= 0).all()
    assert notes[-1, 1] == sum(r[3] for r in rows) and clip_len == N.tick_to_sample(notes[-1, 1]) + N.RELEASE
    none, none_len, none_status = N.rows_to_notes([])
    assert none.shape == (0, 4) and none_len == 0 and none_status == N.OK
    assert N.tick_to_sample(N.MAX_TICK) + N.RELEASE <= N.MAX_SAMPLES < N.tick_to_sample(N.MAX_TICK + 1) + N.RELEASE + 92
    long_rows = [(0, 60, 100, N.MAX_TICK), (1, 60, 100, 0)]
    assert N.rows_to_notes(long_rows)[2] == N.OK
    for bad in ([(0, 60, 100, N.MAX_TICK + 1), (1, 60, 100, 0)], [(0, 60, 100, N.MAX_TICK), (1, 60, 100, 1)]):
        notes, clip_len, status = N.rows_to_notes(bad)
        assert status == N.ELONG and len(notes) == 0 and clip_len == 0
    with pytest.raises(N.LogError):
        N.log_rows(case_log("repeated_departures"), [60, 64])                   # node 2 has no note level
    with pytest.raises(N.LogError):
        N.log_rows(case_log("repeated_departures"), [60, 64, 128, 0])           # mido refuses note 128
    assert N.log_rows(case_log("ids_filtered"), [60]) != []                     # an unused node may be missing


CLIPS = {
    "one_note": [(10, 40, 69, 100)],
    "chord_short": [(0, 0, 60, 127), (0, 3, 64, 90), (2, 5, 67, 60), (5, 5, 72, 126)],
    "sparse": [(100, 220, 45, 80), (3000, 3100, 81, 110), (3100, 3100, 33, 64)],
}


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_frames_equal_pcm_cut_by_the_reflect_rule(name):
    notes = np.asarray(CLIPS[name], dtype=np.int64)
    clip_len = N.tick_to_sample(notes[-1, 1]) + N.RELEASE
    pcm = N.pcm(notes, 0, clip_len)
    assert pcm.dtype == np.int16 and pcm.any() and not N.pcm(notes, clip_len, 4096).any()
    hop = clip_len // 215
    idx = np.arange(216)[:, None] * hop + np.arange(2048)[None, :] - 1024
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= clip_len, 2 * (clip_len - 1) - idx, idx)
    want = pcm[idx].astype(np.float32) * np.float32(2.0 ** -15)
    got = N.frames(notes, clip_len)
    assert got.dtype == np.float32 and got.shape == (216, 2048) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not N.frames(np.zeros((0, 4), np.int64), 0).any()


def test_tables_and_voice_bounds():
    """|wave * v * e_att * e_rel| >> 30 is at most 8127; the arithmetic shift floors, so the one negative extreme
    (wave -32767 at velocity 127, both envelopes full) is -8128.  5000 such voices stay far below 2^31 (and 2^26)."""
    wave, inc = N.tables()
    assert wave.dtype == np.int16 and wave.max() == 32767 and wave.min() == -32767 and wave[0] == 0 and wave[512] == 32767
    assert inc.dtype == np.uint32 and inc[69] == round(2 ** 32 * 440 / 44100) and inc[127] < 2 ** 31
    top = 32767 * 127 * N.ATTACK * N.RELEASE
    assert top >> N.SHIFT == 8127 and (-top) >> N.SHIFT == -8128 and 5000 * 8128 < 1 << 26
    # 5000 voices stacked on one tick, loudest pitch-independent case: same pitch, velocity 127
    notes = np.tile(np.asarray([[4, 4, 69, 127]], dtype=np.int64), (5000, 1))
    s0 = N.tick_to_sample(4)
    s = np.arange(s0, s0 + 2048, dtype=np.int64)
    v = N.voices(notes[:1], s)
    assert v.max() <= 8127 and v.min() >= -8128 and np.abs(v).max() > 7000
    total = N.voices(notes, s).sum(axis=0)
    assert np.array_equal(total, 5000 * v[0]) and np.abs(total).max() < 1 << 26
    out = N.synth(notes, s)
    assert out.max() == 32767 and out.min() == -32768                            # the clamp, not a wrap
