"""GPU: the kernels of the stand-alone demo path against their mirrors (tests/sim_to_wav_ref.py) and the reference
recording (tests/golden/sim_to_wav.npz), and sim_to_wav end to end.

Bar: equal bits.  gdm_s2w_prologue repeats numpy's float64 operations in numpy's order, gdm_des_log_to_notes_pc and
gdm_synth_windows_gm are integer only: every comparison below is of integers or of float64 bit patterns.
"""
import os
import struct
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import des_notes_ref as DR  # noqa: E402
import sim_to_wav_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("value", "event_id", "node", "kind")
GUARD = 64
NONE = -2 ** 31


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "sim_to_wav.npz")) as z:
        return {k: z[k] for k in z.files}


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- gdm_s2w_prologue --------------------------------------------------------------------------------------------------
def _matrix(kind, size, g):
    dim = size - 5
    m = g.random((size, size))
    if kind == "random":                # as the demo draws it: zero parameter columns, random parameter rows
        m[dim:, :] = 0
        m[:, dim:] = 0
        m[dim:, :dim] = g.random((5, dim))
    elif kind == "no_source":
        m[dim] = g.random(size) * 0.75
    elif kind == "all_sources":         # every node a source: only the parameter columns are left in a row's sum
        m[dim, :dim] = 0.75 + g.random(dim) * 0.25 + 1e-9
        m[dim, dim:] = g.random(5) * 0.5
    elif kind == "params":              # nonzero parameter columns, two of them above the threshold, negative entries
        m[dim, dim:] = (0.95, 0.1, 0.8, 0.2, 0.76)
        m[0, dim + 1] = -0.125
    elif kind == "zero_row":            # row 0 sums to zero: refused
        m[0, :] = 0
    return m


BATCHES = {1: ("params",), 3: ("random", "zero_row", "params"), 5: ("random", "no_source", "all_sources", "params",
                                                                    "zero_row")}


@pytest.mark.parametrize("size", (6, 8, 13, 32, 133, 256))
@pytest.mark.parametrize("b", (1, 3, 5))
def test_s2w_prologue_equals_the_mirror(size, b):
    from gan_des_midi_music_gen_amd import ops
    g = np.random.default_rng(1000 * size + b)
    dim = size - 5
    ms = np.stack([_matrix(kind, size, g) for kind in BATCHES[b]])
    over = np.full(b, NONE, dtype=np.int32)
    if b > 1:
        over[b - 1] = 91                                                  # an instrument_override on the last sample
    shapes = {"d": (b, dim), "dd": (b, dim, dim), "": (b,)}
    fill = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A, torch.float64: -12345.5}
    guarded, out = {}, {}
    for name, dt, kind in ops._S2W_FIELDS:
        n = int(np.prod(shapes[kind]))
        guarded[name] = torch.full((n + 2 * GUARD,), fill[dt], dtype=dt, device="cuda")
        out[name] = guarded[name][GUARD:GUARD + n].view(shapes[kind])
    m_dev = _up(ms, np.float64)
    got = ops.s2w_prologue(m_dev, _up(over, np.int32), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(m_dev.cpu().numpy()), _bits(ms)), "the input is read only"
    for name, dt, _kind in ops._S2W_FIELDS:
        assert bool((guarded[name][:GUARD] == fill[dt]).all()) and bool((guarded[name][-GUARD:] == fill[dt]).all()), name
    got = {k: v.cpu().numpy() for k, v in got.items()}
    refused = 0
    for i, kind in enumerate(BATCHES[b]):
        inst = None if over[i] == NONE else int(over[i])
        try:
            p = R.prologue(ms[i], inst)
        except R.Refused:
            refused += 1
            assert got["status"][i] == 1 and (got["scale"][i] == -1.0).all()
            off = got["adj"][i][~np.eye(dim, dtype=bool)]
            assert (off == 0).all() and (np.abs(got["adj"][i].diagonal()) == 1).all()
            continue
        assert got["status"][i] == 0
        assert np.array_equal(got["src"][i].astype(bool), p["src"])
        assert np.array_equal(got["instruments"][i], p["instruments"]) and np.array_equal(got["note_levels"][i],
                                                                                           p["note_levels"])
        assert np.array_equal(_bits(got["loc"][i]), _bits(p["loc"])) and np.array_equal(_bits(got["scale"][i]),
                                                                                        _bits(p["scale"]))
        assert (got["queue_cap"][i] == 127).all()
        assert np.array_equal(_bits(got["adj"][i]), _bits(p["adj"])), kind
        if kind == "no_source":
            assert not p["src"].any()
        if kind == "all_sources":
            assert p["src"].all()
    # a zero-sum row is refused; so is a one-node network whose parameter columns are zero (its row has nothing left)
    assert refused == sum(k == "zero_row" or (k == "random" and dim == 1) for k in BATCHES[b])
    if b > 1:
        assert (got["instruments"][b - 1] == 91).all()


def test_s2w_prologue_on_the_recorded_matrices(golden):
    from gan_des_midi_music_gen_amd import ops
    for name in (str(n) for n in golden["names"]):
        inst = int(golden[f"{name}/instrument"])
        for j in range(int(golden[f"{name}/count"])):
            pre = f"{name}/{j}/"
            over = None if inst < 0 else _up([inst], np.int32)
            got = ops.s2w_prologue(_up(golden[pre + "matrix"][None], np.float64), over)
            assert np.array_equal(_bits(got["adj"][0].cpu().numpy()), _bits(golden[pre + "sim_matrix"]))
            assert np.array_equal(_bits(got["loc"][0].cpu().numpy()), _bits(golden[pre + "dist"][:, 0]))
            assert np.array_equal(_bits(got["scale"][0].cpu().numpy()), _bits(golden[pre + "dist"][:, 1]))
            assert np.array_equal(got["instruments"][0].cpu().numpy(), golden[pre + "instruments"])
            assert np.array_equal(got["note_levels"][0].cpu().numpy(), golden[pre + "note_levels"])


# ---- gdm_des_log_to_notes_pc -------------------------------------------------------------------------------------------
def _notes_pc(logs, instruments, note_levels):
    from gan_des_midi_music_gen_amd import ops
    ptr = np.concatenate([[0], np.cumsum([len(lg["value"]) for lg in logs])])
    cat = {k: np.concatenate([lg[k] for lg in logs]) for k in FIELDS}
    rec = (_up(cat["value"], np.float64), _up(cat["event_id"], np.int64), _up(cat["node"], np.int32),
           _up(cat["kind"], np.int32), _up(ptr, np.int64))
    out = ops.des_log_to_notes_pc(*rec, _up(instruments, np.int32), _up(note_levels, np.int32))
    plain = ops.des_log_to_notes(*rec, _up(note_levels, np.int32))
    return [t.cpu().numpy() for t in out], [t.cpu().numpy() for t in plain]


def test_log_to_notes_pc_equals_the_recorded_messages(golden):
    for name in (str(n) for n in golden["names"]):
        for j in range(int(golden[f"{name}/count"])):
            pre = f"{name}/{j}/"
            log = {k: golden[pre + k] for k in FIELDS}
            (notes, n_notes, clip_len, status), _plain = _notes_pc([log], golden[pre + "instruments"][None],
                                                                   golden[pre + "note_levels"][None])
            want, want_len, want_status = R.rows_to_notes([tuple(int(x) for x in r) for r in golden[pre + "rows"]])
            assert status[0] == want_status == R.OK and n_notes[0] == len(want) and clip_len[0] == want_len
            assert np.array_equal(notes[0, :len(want)], want) and not notes[0, len(want):].any()


def test_log_to_notes_pc_on_the_crafted_logs(golden_dir):
    """Every branch of process_line (the crafted logs of des_notes.npz), all cases in one launch; the existing entry on
    the same records returns what its own mirror says, as before."""
    with np.load(os.path.join(golden_dir, "des_notes.npz")) as z:
        names = [str(n) for n in z["names"] if f"{n}/value" in z.files]
        logs = [{k: z[f"{n}/{k}"] for k in FIELDS} for n in names]
        inst = np.stack([z[f"{n}/instruments"] for n in names])
        levels = np.stack([z[f"{n}/note_levels"] for n in names])
    assert len(names) == 7
    (notes, n_notes, clip_len, status), (p_notes, p_n, p_len, p_status) = _notes_pc(logs, inst, levels)
    assert n_notes.sum() > 300
    for i, log in enumerate(logs):
        want, want_len, want_status = R.rows_to_notes(R.log_rows(log, inst[i], levels[i]))
        assert status[i] == want_status and n_notes[i] == len(want) and clip_len[i] == want_len, names[i]
        assert np.array_equal(notes[i, :len(want)], want), names[i]
        old, old_len, old_status = DR.log_to_notes(log, levels[i])
        assert p_status[i] == old_status and p_n[i] == len(old) and p_len[i] == old_len
        assert np.array_equal(p_notes[i, :len(old)], old)
        assert np.array_equal(2 * old[:, :2], want[:, :2]) and np.array_equal(old[:, 2:], want[:, 2:4])


def test_log_to_notes_pc_refuses_program_128(golden):
    pre = "size13/0/"
    log = {k: golden[pre + k] for k in FIELDS}
    inst = np.stack([golden[pre + "instruments"], golden[pre + "instruments"]])
    inst[1, :] = 128
    levels = np.stack([golden[pre + "note_levels"]] * 2)
    (notes, n_notes, clip_len, status), _plain = _notes_pc([log, log], inst, levels)
    assert status.tolist() == [R.OK, R.EPROGRAM] and n_notes[0] > 0 and n_notes[1] == 0 and clip_len[1] == 0
    from gan_des_midi_music_gen_amd import sim_log_process_music
    with pytest.raises(ValueError, match="sample 1: program outside"):
        sim_log_process_music.raise_for_status(torch.from_numpy(status))


# ---- gdm_synth_windows_gm ----------------------------------------------------------------------------------------------
ENV = R.gm_tables()[1]


def family_clip():
    """One note per family and attack-straddling length: s_off - s_on in {1, A_f - 1, A_f, A_f + 1}; onsets 3000 apart,
    so the long releases (up to 65536 samples) of different families overlap."""
    rows, on = [], 500
    for f in range(16):
        att = int(ENV[f, 0])
        for length in (1, att - 1, att, att + 1):
            rows.append((on, on + length, 40 + 3 * f, 60 + 4 * f, 8 * f + (f % 8)))
            on += 3000
    return np.asarray(rows, dtype=np.int64)


def crowd_clip():
    """1025 quiet notes of all families that sound throughout samples 2048 .. 4096: a second GDM_SYNTH_TILE."""
    g = np.random.default_rng(7)
    n = 1025
    return np.stack([np.sort(g.integers(0, 2000, n)), np.full(n, 8000), g.integers(40, 90, n), np.full(n, 20),
                     g.integers(0, 128, n)], axis=1).astype(np.int64)


def loud_clip():
    """Five loud unison voices of one family: the sum leaves the 16-bit range on both sides."""
    return np.asarray([(100, 30000, 57, 127, 19)] * 5, dtype=np.int64)


CLIPS = [np.zeros((0, 5), np.int64), family_clip(), crowd_clip(), loud_clip()]
IN_RELEASE = int(CLIPS[1][7, 1]) + int(ENV[1, 1]) // 2               # inside the release of a family-1 note


def _gm(clips, win_clip, win_start, win_len):
    from gan_des_midi_music_gen_amd import ops
    notes = _up(np.concatenate(clips), np.int64)
    ends = _up(np.concatenate([R.end_max(c) for c in clips]), np.int64)
    ptr = _up(np.concatenate([[0], np.cumsum([len(c) for c in clips])]), np.int64)
    w = len(win_clip)
    stride = (win_len + 7) // 8 * 8 + 8
    buf = torch.full((w * stride + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = buf[GUARD:GUARD + w * stride].view(w, stride)
    ops.synth_windows_gm(notes, ends, ptr, _up(win_clip, np.int32), _up(win_start, np.int64), win_len, out=out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0x5A5A).all() and (got[-GUARD:] == 0x5A5A).all()
    got = got[GUARD:-GUARD].reshape(w, stride)
    assert (got[:, win_len:] == 0x5A5A).all(), "columns from win_len on are not written"
    return got[:, :win_len]


def test_synth_gm_windows_equal_the_mirror():
    win_clip, win_start, win = [2, 3, 0, 1, 1, 3], [0, 0, 123, IN_RELEASE, 0, 25000], 6000
    got = _gm(CLIPS, win_clip, win_start, win)
    for w, (c, s) in enumerate(zip(win_clip, win_start)):
        assert np.array_equal(got[w], R.window(CLIPS[c], s, win)), (c, s)
    crowd = R.voice_sum(CLIPS[2], 2048, 2048)
    assert len(CLIPS[2]) == 1025 and (CLIPS[2][:, 0] < 2048).all() and (CLIPS[2][:, 1] > 4096).all() and crowd.any()
    loud = R.voice_sum(CLIPS[3], 0, win)
    assert loud.max() > 32767 and loud.min() < -32768 and got[1].max() == 32767 and got[1].min() == -32768
    assert not got[2].any()                                               # the empty clip
    assert CLIPS[1][7, 1] < IN_RELEASE < CLIPS[1][7, 1] + ENV[1, 1]      # the window opens inside that note's release
    assert R.voice_sum(CLIPS[1][7:8], IN_RELEASE, 100).any()
    assert 30000 < 25000 + win < 30000 + ENV[2, 1] and got[5][-100:].any()  # ... and the last one ends inside one


def test_synth_gm_every_family_at_attack_straddling_lengths():
    clip = CLIPS[1]
    total = int(R.end_max(clip)[-1])
    got = _gm([clip], [0], [0], total)
    want = R.window(clip, 0, total)
    assert np.array_equal(got[0], want)
    assert sorted(set(((clip[:, 4] & 127) >> 3).tolist())) == list(range(16))
    lengths = (clip[:, 1] - clip[:, 0]).reshape(16, 4)
    assert np.array_equal(lengths, np.stack([np.ones(16, np.int64), ENV[:, 0] - 1, ENV[:, 0], ENV[:, 0] + 1], axis=1))
    # two families overlap: where the second note of family 15 starts, a family-14 release (65536 samples) still sounds
    one = R.voice_sum(clip[56:60], int(clip[61, 0]), 100)
    assert one.any() and R.voice_sum(clip[60:64], int(clip[61, 0]), 100).any()


@pytest.mark.parametrize("win_len", (1, 2048, 2049))
def test_synth_gm_window_lengths(win_len):
    got = _gm(CLIPS, [3, 1, 2], [101, 500, 2047], win_len)
    for w, (c, s) in enumerate(zip([3, 1, 2], [101, 500, 2047])):
        assert np.array_equal(got[w], R.window(CLIPS[c], s, win_len))
    assert got[0].any()


def test_synth_gm_clamps_the_envelope_table():
    """env is clamped to 1 .. 2^21 on the device before use."""
    from gan_des_midi_music_gen_amd import ops
    waves, env, inc = ops.synth_gm_tables(torch.device("cuda"))
    bad = env.clone()
    bad[0] = torch.tensor([0, -5], dtype=torch.int32)
    clip = np.asarray([(10, 50, 60, 100, 0), (20, 400, 64, 90, 9)], dtype=np.int64)
    host_env = bad.cpu().numpy()
    out = ops.synth_windows_gm(_up(clip, np.int64), _up(R.end_max(clip, host_env), np.int64), _up([0, 2], np.int64),
                               _up([0], np.int32), _up([0], np.int64), 1000, tables=(waves, bad, inc))
    want = R.window(clip, 0, 1000, (R.gm_tables()[0], host_env, R.gm_tables()[2]))
    assert np.array_equal(out[0, :1000].cpu().numpy(), want) and want.any()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _read_wav(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt " and struct.unpack("<HHI", data[20:28]) == (1, 1, 44100)
    n = struct.unpack("<I", data[40:44])[0]
    assert len(data) == 44 + n
    return np.frombuffer(data[44:], dtype="<i2")


def _messages(path):
    from gan_des_midi_music_gen_amd import datasets
    md = datasets.read_midi(path)
    kinds = {0xC: R.PROGRAM_CHANGE, 0x9: R.NOTE_ON, 0x8: R.NOTE_OFF}
    rows, prev = [], 0
    for tick, st, a, b in zip(md.tick.tolist(), md.status.tolist(), md.a.tolist(), md.b.tolist()):
        if st != 0xFF:
            rows.append((kinds[st >> 4], a, b, tick - prev))
            prev = tick
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


def test_render_whole_cut_blank_and_across_the_chunk_seam(tmp_path, monkeypatch):
    """One 0.82 s clip through ``_render``: the header is ``util.wav_header``, the body the reference render; cut at a
    quarter second; a clip without notes is five seconds of zeros; in 4096-sample chunks the same bytes."""
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W, util
    rows, total, rate = np.asarray([[2, 600, 60, 80, 9]], dtype=np.int64), 36000, 44100
    dev_rows = _up(rows, np.int64)

    def written(name, count, max_seconds=None):
        path = str(tmp_path / "clips" / name)
        S2W._render(dev_rows[:count], count, total if count else 0, path, max_seconds, dev_rows.device)
        return open(path, "rb").read()

    body = R.render(rows, total).astype("<i2").tobytes()
    assert any(body[:2 * 4096]) and any(body[2 * 4096:])
    whole = written("whole.wav", 1)
    assert whole == util.wav_header(total, rate) + body
    assert written("cut.wav", 1, 0.25) == util.wav_header(rate // 4, rate) + body[:2 * (rate // 4)]
    assert written("blank.wav", 0) == util.wav_header(5 * rate, rate) + bytes(10 * rate)
    monkeypatch.setattr(util, "_WAV_CHUNK", 4096)
    assert written("seam.wav", 1) == whole


def test_sim_to_wav_des_equals_the_recording(golden, tmp_path):
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W
    out_dir = str(tmp_path / "out")
    np.random.seed(int(golden["two_size13/seed"]))
    batch = S2W.sim_to_wav([None, None], size=13, simulate="des", out_dir=out_dir, max_seconds=2, return_batch=True)
    assert np.int64(np.random.randint(0, 2 ** 31 - 1)) == golden["two_size13/rng_after"]
    assert batch.wav_paths == [os.path.join(out_dir, "wav", f"output_{i}.wav") for i in range(2)]
    for i in range(2):
        rows = golden[f"two_size13/{i}/rows"]
        assert np.array_equal(_messages(batch.midi_paths[i]), rows)
        notes, clip_len, _status = R.rows_to_notes([tuple(int(x) for x in r) for r in rows])
        n = int(batch.n_notes[i])
        assert n == len(notes) and int(batch.clip_len[i]) == clip_len
        assert np.array_equal(batch.notes[i, :n].cpu().numpy(), notes)
        assert np.array_equal(batch.programs[i].cpu().numpy(), golden[f"two_size13/{i}/instruments"])
        want = R.render(notes, clip_len, max_seconds=2)
        assert len(want) == 2 * 44100 and want.any()
        assert np.array_equal(_read_wav(batch.wav_paths[i]), want)
    assert open(os.path.join(out_dir, "midi", "output.mid"), "rb").read() == open(batch.midi_paths[1], "rb").read()


def test_sim_to_wav_des_batch_equals_independent_host_runs(tmp_path):
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W, simulation_v3
    b, size, dim = 5, 13, 8
    np.random.seed(404)
    base = np.random.randint(0, 2 ** 32, size=b)
    np.random.seed(404)
    batch = S2W.sim_to_wav([None] * b, size=size, simulate="des_batch", out_dir=str(tmp_path / "out"), max_seconds=0.25,
                           return_batch=True)
    alias = S2W.sim_to_wav
    total = 0
    for i in range(b):
        rs = np.random.RandomState(int(base[i]))
        p = R.prologue(R.draw_matrix(size, rs.rand))
        seeds, state = R.reseed_pair(rs)
        host = simulation_v3.run_batch_host(p["adj"][None], p["loc"][None], p["scale"][None],
                                            np.full((1, dim), 127, np.int32), np.asarray(seeds, np.int64),
                                            np.asarray([1000], np.int64), [state], math=1, max_records=5001)
        log = simulation_v3.sample_log(host, 0)
        notes, clip_len, status = R.rows_to_notes(R.log_rows(log, p["instruments"], p["note_levels"]))
        n = int(batch.n_notes[i])
        assert status == R.OK and n == len(notes) and int(batch.clip_len[i]) == clip_len
        assert np.array_equal(batch.notes[i, :n].cpu().numpy(), notes)
        assert np.array_equal(_read_wav(batch.wav_paths[i]), R.render(notes, clip_len, max_seconds=0.25))
        total += n
    assert total > 0
    np.random.seed(404)                      # "des_device" is an alias for now: the same files
    again = alias([None] * b, size=size, simulate="des_device", out_dir=str(tmp_path / "alias"), max_seconds=0.25,
                  return_batch=True)
    assert torch.equal(again.notes, batch.notes) and torch.equal(again.n_notes, batch.n_notes)


def test_sim_to_wav_des_batch_on_the_simulator_kernel(tmp_path):
    """From DES_BATCH_DEVICE_MIN_B samples on "des_batch" simulates with gdm_des_run_batch: the same notes as the host
    mirror with portable math, all samples in one host call."""
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp, simulation_to_wav as S2W, simulation_v3
    b, size, dim = msp.DES_BATCH_DEVICE_MIN_B, 13, 8
    given = np.random.default_rng(5).random((size, size))
    matrices = [given if i == 7 else None for i in range(b)]
    np.random.seed(77)
    base = np.random.randint(0, 2 ** 32, size=b)
    ms, seed, states = S2W.batch_draws(matrices, size, base)
    assert np.array_equal(ms[7], given)
    np.random.seed(77)
    batch = S2W.sim_to_wav(matrices, size=size, simulate="des_batch", out_dir=str(tmp_path / "out"), max_seconds=0.01,
                           return_batch=True)
    pro = [R.prologue(m) for m in ms]
    host = simulation_v3.run_batch_host(np.stack([p["adj"] for p in pro]), np.stack([p["loc"] for p in pro]),
                                        np.stack([p["scale"] for p in pro]), np.full((b, dim), 127, np.int32), seed,
                                        np.full(b, 1000, np.int64), states, math=1, max_records=5001)
    counts = batch.n_notes.cpu().numpy()
    notes = batch.notes.cpu().numpy()
    for i in range(b):
        want, clip_len, status = R.rows_to_notes(R.log_rows(simulation_v3.sample_log(host, i), pro[i]["instruments"],
                                                            pro[i]["note_levels"]))
        assert status == R.OK and counts[i] == len(want) and int(batch.clip_len[i]) == clip_len
        assert np.array_equal(notes[i, :len(want)], want)
    assert (counts > 0).sum() > b // 2 and len(batch.wav_paths) == b


def test_sim_to_wav_size_256_runs_on_the_host_simulator(tmp_path):
    from gan_des_midi_music_gen_amd import ops, simulation_to_wav as S2W
    assert ops.DES_BATCH_MAX_DIM == 128
    np.random.seed(8)
    paths = S2W.sim_to_wav([None], size=256, simulate="des_batch", out_dir=str(tmp_path / "out"), max_events=2000,
                           max_seconds=1)
    assert len(_read_wav(paths[0])) == 44100 and os.path.exists(str(tmp_path / "out" / "midi" / "output_0.mid"))
    with pytest.raises(ValueError, match="valid sizes"):
        S2W.sim_to_wav([None], size=257, out_dir=str(tmp_path / "no"))


def test_sim_to_wav_same_instrument_and_no_source(golden, tmp_path):
    from gan_des_midi_music_gen_amd import simulation_to_wav as S2W
    np.random.seed(int(golden["instrument91/seed"]))
    batch = S2W.sim_to_wav([None], size=13, use_same_instrument=91, out_dir=str(tmp_path / "a"), max_seconds=0.5,
                           return_batch=True)
    rows = _messages(batch.midi_paths[0])
    assert np.array_equal(rows, golden["instrument91/0/rows"])
    n = int(batch.n_notes[0])
    assert n > 0 and bool((batch.notes[0, :n, 4] == 91).all()) and (rows[rows[:, 0] == R.PROGRAM_CHANGE, 1] == 91).all()
    quiet = golden["no_source/0/matrix"]
    for simulate in ("des", "des_batch"):
        batch = S2W.sim_to_wav([quiet], size=quiet.shape[0], simulate=simulate, out_dir=str(tmp_path / simulate),
                               return_batch=True)
        assert int(batch.n_notes[0]) == 0 and int(batch.clip_len[0]) == 0
        assert len(_messages(batch.midi_paths[0])) == 0
        wav = _read_wav(batch.wav_paths[0])
        assert len(wav) == 5 * 44100 and not wav.any()
    bad = quiet.copy()
    bad[0, :] = 0
    with pytest.raises(ValueError, match="matrix 1 has a row"):
        S2W.sim_to_wav([quiet, bad], size=quiet.shape[0], simulate="des_batch", out_dir=str(tmp_path / "bad"))
