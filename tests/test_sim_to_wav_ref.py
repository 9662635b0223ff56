"""CPU: the stand-alone demo path (gan_des_midi_music_gen_amd.simulation_to_wav) against the reference recording
tests/golden/sim_to_wav.npz (made by tests/golden/make_sim_to_wav_golden.py from SIMULATOR/simulation_to_wav.py itself).

Bar: equal bits everywhere -- integers, or float64 values computed by the same operations in the same order.
  * the numpy mirror (tests/sim_to_wav_ref.py) reproduces the recorded draws, Sim arguments and message rows;
  * "des" mode's host pieces (numpy's global stream + gdm_des_run, the prologue taken from the mirror so that no device
    is needed) give the recorded Sim arguments and the recorded event records: the first 5000 and the SHA-256 of all;
  * the MIDI writer's bytes read back as the recorded messages; midi_notes(programs=True) on them equals the mirror's
    five-column rows; midi_notes() without the keyword is what it was;
  * planted faults are caught; the three C entries refuse bad arguments on the host.
"""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_to_wav_ref as R  # noqa: E402

FIELDS = ("value", "event_id", "node", "kind")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "sim_to_wav.npz")) as z:
        return {k: z[k] for k in z.files}


CASES = ("size8", "size13", "size32", "two_size13", "instrument91", "given_params", "no_source")


def _case(golden, name):
    seed, size, count, inst = (int(golden[f"{name}/{k}"]) for k in ("seed", "size", "count", "instrument"))
    return seed, size, count, (None if inst < 0 else inst)


def _sample(golden, name, j):
    pre = f"{name}/{j}/"
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


def test_fixture_lists_the_cases(golden):
    assert tuple(str(n) for n in golden["names"]) == CASES
    for name in CASES:
        _seed, _size, count, _inst = _case(golden, name)
        for j in range(count):
            s = _sample(golden, name, j)
            # the demo never calls generate_midi: one track, no header message, hence the default tempo
            assert list(s["meta"]) == ["end_of_track"] and int(s["n_tracks"]) == 1
            if name != "no_source":
                assert (s["sim_matrix"].diagonal() > 0).any() and (s["rows"][:, 0] == R.NOTE_ON).any()
    assert len(_sample(golden, "no_source", 0)["rows"]) == 0 and int(golden["no_source/0/n_records"]) == 0
    assert bool(golden["given_params/0/given"]) and not bool(golden["size13/0/given"])


@pytest.mark.parametrize("name", CASES)
def test_mirror_prologue_and_rows_equal_the_recording(golden, name):
    _seed, size, count, inst = _case(golden, name)
    for j in range(count):
        s = _sample(golden, name, j)
        before = s["matrix"].copy()
        p = R.prologue(s["matrix"], inst)
        assert np.array_equal(s["matrix"], before)
        assert np.array_equal(p["adj"].view(np.int64), s["sim_matrix"].view(np.int64))
        assert np.array_equal(p["loc"].view(np.int64), np.ascontiguousarray(s["dist"][:, 0]).view(np.int64))
        assert np.array_equal(p["scale"].view(np.int64), np.ascontiguousarray(s["dist"][:, 1]).view(np.int64))
        assert p["queue_list"] == list(s["queue_list"]) == [127] * size
        assert np.array_equal(p["instruments"], s["instruments"]) and np.array_equal(p["note_levels"], s["note_levels"])
        assert np.array_equal(p["src"], s["sim_matrix"].diagonal() > 0)
        assert int(s["customers"]) == 1000
        rows = R.log_rows({k: s[k] for k in FIELDS}, p["instruments"], p["note_levels"])
        assert np.array_equal(np.asarray(rows, np.int64).reshape(-1, 4), s["rows"])


def _des_host(golden, name):
    """"des" mode's host pieces under the recorded seed: numpy's global stream, the mirror's prologue, gdm_des_run."""
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W, simulation_v3
    seed, size, count, inst = _case(golden, name)
    dim = size - 5
    np.random.seed(seed)
    out = []
    for j in range(count):
        s = _sample(golden, name, j)
        m = s["matrix"].copy() if bool(s["given"]) else S2W.draw_matrix(size)
        p = R.prologue(m, inst)
        np.random.seed(np.random.randint(0, 99999, size=1))
        seeds = np.random.randint(0, 99999, size=1)
        sim = simulation_v3.Sim(p["adj"], [["normal", p["loc"][i], p["scale"][i]] for i in range(dim)], [127] * dim,
                                seeds=seeds, logging_mode='Music', max_events=10 ** 7)
        sim.run(number_of_customers=1000)
        out.append((m, p, seeds, sim.music_log))
    return out, np.int64(np.random.randint(0, 2 ** 31 - 1))


@pytest.mark.parametrize("name", CASES)
def test_des_mode_host_pieces_equal_the_recording(golden, name):
    runs, rng_after = _des_host(golden, name)
    for j, (m, p, seeds, log) in enumerate(runs):
        s = _sample(golden, name, j)
        assert np.array_equal(m.view(np.int64), s["matrix"].view(np.int64))            # the draws of lines 12-22
        assert np.array_equal(p["adj"].view(np.int64), s["sim_matrix"].view(np.int64))
        assert np.array_equal(np.asarray(seeds, np.int64), s["seeds"])                   # the reseed pair
        assert len(log) == int(s["n_records"])
        for k in FIELDS:
            a, b = np.ascontiguousarray(log[k][:5000]), s[k]
            assert np.array_equal(a.view(np.int64) if k == "value" else a, b.view(np.int64) if k == "value" else b), k
        assert R.records_sha256(log) == str(s["sha256"])
    assert rng_after == golden[f"{name}/rng_after"]                                      # the stream is carried along


@pytest.mark.parametrize("name", CASES)
def test_writer_bytes_read_back_as_the_recorded_messages(golden, name):
    from gan_des_midi_music_gen_amd import datasets, sim_log_to_midi, simulation_to_wav as S2W
    _seed, _size, count, _inst = _case(golden, name)
    for j in range(count):
        s = _sample(golden, name, j)
        rows = [tuple(int(x) for x in r) for r in s["rows"]]
        notes, clip_len, status = R.rows_to_notes(rows)
        assert status == R.OK
        track = S2W.notes_to_track_pc(notes)
        assert track == R.track_of(rows)
        data = sim_log_to_midi.track_bytes(track)
        md = datasets.read_midi(data)
        assert md.ticks_per_beat == 480 and md.format == 1
        kinds = {0xC: R.PROGRAM_CHANGE, 0x9: R.NOTE_ON, 0x8: R.NOTE_OFF}
        back, prev = [], 0
        for tick, st, a, b in zip(md.tick.tolist(), md.status.tolist(), md.a.tolist(), md.b.tolist()):
            if st == 0xFF:
                continue
            assert st & 15 == 0
            back.append((kinds[st >> 4], a, b, tick - prev))
            prev = tick
        assert back == rows
        assert md.status.tolist().count(0xFF) == 1 and md.kind[-1] == datasets._K_EOT
        got, got_len = datasets.midi_notes(data, programs=True)
        want = R.notes_in_samples(notes)
        assert np.array_equal(got, want[np.argsort(want[:, 0], kind="stable")]) and got.shape[1] == 5
        if len(notes):
            assert clip_len == R.tick_to_sample(notes[-1, 1]) + R.TAIL
            assert got_len == int(want[:, 1].max()) + 8192
            plain, plain_len = datasets.midi_notes(data)
            assert np.array_equal(plain, got[:, :4]) and plain_len == got_len
        else:
            assert clip_len == 0 and got_len == 5 * 44100 and got.shape == (0, 5)


def test_midi_notes_without_the_keyword_is_unchanged(golden_dir):
    """programs=True only adds the column; the default call returns what it returned before on the shipped files (whose
    expected rows other tests pin): the first four columns, the same order, the same length."""
    from gan_des_midi_music_gen_amd import datasets
    files = sorted(glob.glob(os.path.join(golden_dir, "midi", "*.mid")))
    assert len(files) >= 9
    for path in files:
        plain, plain_len = datasets.midi_notes(path)
        with_prog, length = datasets.midi_notes(path, programs=True)
        assert plain.shape[1] == 4 and plain.dtype == np.int64
        assert np.array_equal(with_prog[:, :4], plain) and length == plain_len
        assert with_prog.shape == (len(plain), 5) and ((with_prog[:, 4] >= 0) & (with_prog[:, 4] <= 127)).all()


def test_midi_notes_program_in_force_per_channel():
    import synth_windows_ref as SW
    from gan_des_midi_music_gen_amd import datasets
    data = SW.midi_bytes([[(0, ("on", 0, 60, 100)), (10, ("pc", 0, 91)), (0, ("pc", 1, 27)), (0, ("on", 0, 62, 90)),
                           (5, ("on", 1, 64, 80)), (5, ("pc", 0, 5)), (0, ("off", 0, 60, 0)), (0, ("off", 0, 62, 0)),
                           (0, ("on", 0, 65, 70)), (10, ("off", 1, 64, 0)), (0, ("off", 0, 65, 0))]])
    notes, _ = datasets.midi_notes(data, programs=True)
    assert notes[:, 2].tolist() == [60, 62, 64, 65] and notes[:, 4].tolist() == [0, 91, 27, 5]


@pytest.mark.parametrize("fault", R.PROLOGUE_FAULTS)
def test_planted_prologue_faults_are_caught(golden, fault):
    s = _sample(golden, "given_params", 0)
    p = R.prologue(s["matrix"], None, fault=fault)
    if fault == "mul_126":
        assert not np.array_equal(p["instruments"], s["instruments"]) or \
            not np.array_equal(p["note_levels"], s["note_levels"])
    else:       # the parameter columns of this matrix are not zero: a sum over dim columns gives other probabilities
        assert not np.array_equal(p["adj"].view(np.int64), s["sim_matrix"].view(np.int64))


def test_planted_single_delta_fault_is_caught(golden):
    s = _sample(golden, "size13", 0)
    rows = R.log_rows({k: s[k] for k in FIELDS}, s["instruments"], s["note_levels"], fault="single_delta")
    assert len(rows) * 2 == len(s["rows"])
    good, _len, _st = R.rows_to_notes([tuple(int(x) for x in r) for r in s["rows"]])
    # single deltas: every tick of the track halves -- the notes the GAN_DES copy would cut from the same log
    on = np.cumsum([r[3] for r in rows])
    assert np.array_equal(2 * on[0::2], good[:, 0]) and np.array_equal(2 * on[1::2], good[:, 1])
    assert not np.array_equal(on[0::2], good[:, 0])


def test_batch_draws_follow_the_documented_streams():
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W
    base = np.array([5, 2 ** 32 - 1, 77], dtype=np.int64)
    given = np.random.default_rng(3).random((9, 9))
    ms, seed, states = S2W.batch_draws([None, given, None], 9, base)
    for b in range(3):
        rs = np.random.RandomState(int(base[b]))
        want = given if b == 1 else R.draw_matrix(9, rs.rand)
        seeds, state = R.reseed_pair(rs)
        assert np.array_equal(ms[b], want) and seed[b] == int(seeds[0])
        assert np.array_equal(states[b][1], state[1]) and states[b][2:] == state[2:]


def test_sizes_and_back_ends_are_checked_on_the_host():
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W
    for size in (5, 257, 1000):
        with pytest.raises(ValueError, match="valid sizes"):
            S2W.sim_to_wav([None], size=size)
    with pytest.raises(ValueError, match="des_batch"):
        S2W.sim_to_wav([None], size=13, simulate="fluidsynth")


# ---- argument checks of the C entries: on the host, before any launch ----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gan_des_midi_music_gen_amd import _lib, build
    build.build()
    return _lib.load()


def _buf(n=4096):
    b = ctypes.create_string_buffer(n + 64)
    a = ctypes.addressof(b)
    return b, (a + 63) // 64 * 64


def test_s2w_prologue_refuses_bad_arguments(lib):
    keep, p = _buf()
    ok = [p] * 8
    assert lib.gdm_s2w_prologue(None, 1, 8, None, *ok, None) == -1 and b"null pointer" in lib.gdm_last_error()
    assert lib.gdm_s2w_prologue(p, 1, 8, None, *ok[:7], None, None) == -1 and b"null pointer" in lib.gdm_last_error()
    for size in (5, 257):
        assert lib.gdm_s2w_prologue(p, 1, size, None, *ok, None) == -1 and b"size" in lib.gdm_last_error()
    assert lib.gdm_s2w_prologue(p, 0, 8, None, *ok, None) == -1 and b"B = 0" in lib.gdm_last_error()
    assert lib.gdm_s2w_prologue(p + 4, 1, 8, None, *ok, None) == -1 and b"aligned" in lib.gdm_last_error()
    assert lib.gdm_s2w_prologue(p, 1, 8, p + 2, *ok, None) == -1 and b"aligned" in lib.gdm_last_error()
    del keep


def test_des_log_to_notes_pc_refuses_bad_arguments(lib):
    keep, p = _buf()
    rec, out = [p] * 5, [p, 5000, p, p, p]
    call = lib.gdm_des_log_to_notes_pc
    assert call(*rec, 1, None, p, 4, 1, 735, 16, 65536, *out, None) == -1 and b"null pointer" in lib.gdm_last_error()
    assert call(None, p, p, p, p, 1, p, p, 4, 1, 735, 16, 65536, *out, None) == -1 and b"records" in lib.gdm_last_error()
    assert call(*rec, 1, p, p, 300, 1, 735, 16, 65536, *out, None) == -1 and b"dim" in lib.gdm_last_error()
    assert call(*rec, 1, p, p, 4, 1, 735, 16, 65536, p, 4999, p, p, p, None) == -1 and b"5000" in lib.gdm_last_error()
    assert call(*rec, 1, p, p, 4, 1, 0, 16, 65536, *out, None) == -1 and b"sample(tick)" in lib.gdm_last_error()
    assert call(*rec, 1, p, p, 4, 1, 735, 1 << 21, 65536, *out, None) == -1 and b"sample(tick)" in lib.gdm_last_error()
    assert call(p + 4, p, p, p, p, 1, p, p, 4, 1, 735, 16, 65536, *out, None) == -1 and b"aligned" in lib.gdm_last_error()
    assert call(*rec, 1, p + 2, p, 4, 1, 735, 16, 65536, *out, None) == -1 and b"aligned" in lib.gdm_last_error()
    del keep


def test_synth_windows_gm_refuses_bad_arguments(lib):
    keep, p = _buf()
    call = lib.gdm_synth_windows_gm
    good = dict(notes=p, end_max=p, n=1, ptr=p, F=1, clip=p, start=p, W=1, win_len=100, stride=104, waves=p, env=p,
                inc=p, out=p)

    def run(**kw):
        a = dict(good, **kw)
        return call(a["notes"], a["end_max"], a["n"], a["ptr"], a["F"], a["clip"], a["start"], a["W"], a["win_len"],
                    a["stride"], a["waves"], a["env"], a["inc"], a["out"], None)

    assert run(waves=None) == -1 and b"null pointer" in lib.gdm_last_error()
    assert run(notes=None) == -1 and b"null pointer" in lib.gdm_last_error()
    assert run(env=p + 2) == -1 and b"aligned" in lib.gdm_last_error()
    assert run(waves=p + 8) == -1 and b"16-byte" in lib.gdm_last_error()
    assert run(out=p + 8) == -1 and b"16-byte" in lib.gdm_last_error()
    assert run(stride=100) == -1 and b"out_stride" in lib.gdm_last_error()
    assert run(W=0) == -1 and run(F=0) == -1 and run(win_len=0) == -1 and run(n=-1) == -1
    del keep


def test_gm_mirror_with_the_plain_tables_is_the_plain_mirror():
    """The identity tests/test_synth_windows_gpu.py demands of the two kernel instances, on the two mirrors and the same
    clips and windows: with the plain wave and (A, R) for every family the programs do not matter."""
    import synth_windows_ref as SW
    import test_synth_windows_gpu as G
    tables = SW.plain_gm_tables()
    assert np.array_equal(tables[2], R.gm_tables()[2]) and (tables[1][:, 0] * tables[1][:, 1] == 1 << 21).all()
    for i, c in ((0, 1), (1, 2)):
        rows, end_max = SW.as_gm(G.CLIPS[c], 31 + i)
        assert np.array_equal(end_max, R.end_max(rows, tables[1])) and len(set(rows[:, 4].tolist())) > 16
        for start in (s for w, s in zip(G.WIN_CLIP, G.WIN_START) if w == c):
            plain = SW.window(G.CLIPS[c], start, G.WIN)
            assert plain.any() and np.array_equal(R.window(rows, start, G.WIN, tables), plain)


def test_ops_tables_and_tick_rule():
    from gan_des_midi_music_gen_amd import ops
    assert ops.tick_rule() == (R.TICK_MUL, R.TICK_DIV) and ops.tick_rule(1000000, 480) == (735, 8)
    assert tuple((w, a) for _n, w, a in ops.SYNTH_GM_FAMILY_TABLE) == R.FAMILIES and len(R.FAMILIES) == 16
    waves, env, _inc = R.gm_tables()
    assert (env[:, 0] * env[:, 1] == 1 << 21).all() and np.abs(waves.astype(np.int64)).max(axis=1).tolist() == [32767] * 16
    assert ops.DES_NOTES_ERRORS[ops.DES_NOTES_EPROGRAM] == "program outside 0..127" and ops.DES_NOTES_EPROGRAM == R.EPROGRAM
