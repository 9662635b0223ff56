"""GPU: gdm_synth_windows (csrc/synth.hip) against its numpy mirror (tests/synth_windows_ref.py, written from
include/gdm.h) and what is built on it: ops.synth_windows, util.melspectrogram_db_from_synth_windows,
datasets.MaestroDataset / midi_to_wav / my_collate, SIMNN.train(maestro_dir=...).

Bar: equal bits.  The synth is integer only and its sum does not depend on the order of the voices, so the kernel's PCM
must equal the mirror's sample for sample; the dataset's spectrograms run the kernels of the WAV route on the same
samples, so they must equal that route's float for float (int32 view).  Every clip and window below exists for one
reason, and the test asserts that reason on the mirror before it compares.
"""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import des_notes_ref as DR  # noqa: E402
import synth_windows_ref as SW  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK, TILE, R = 2048, 1024, SW.RELEASE
WIN, GUARD = 5000, 64
LONG_OFF = 400000                 # the pedal-length note of the chord clip ends here


# ---- the clips -----------------------------------------------------------------------------------------------------------
def chord_clip():
    """~40 notes, first onset at 700.  Named rows first (see test_clips_are_what_they_are_for), then seeded filler, some
    of it around sample 350000 where only the pedal-length note still sounds."""
    rows = [
        (700, LONG_OFF, 41, 90),                             # pedal-length: far longer than all others
        (1000, 3000, 60, 100), (1000, 3100, 64, 90), (1000, 3200, 67, 80),         # a chord
        (1200, 2600, 72, 70), (1900, 3500, 72, 75),          # two overlapping notes of one pitch
        (1500, 4300, 55, 85),                                # spans chunks 0, 1 and 2 of a window starting at 0
        (2048, 2500, 76, 95),                                # starts on a chunk's first sample
        (3900, 4000, 50, 110),                               # its release (to 12192) crosses the window's end at 5000
    ]
    g = np.random.default_rng(11)
    for _ in range(18):
        on = int(g.integers(700, 20000))
        rows.append((on, on + int(g.integers(1, 6000)), int(g.integers(30, 100)), int(g.integers(1, 128))))
    for _ in range(13):
        on = int(g.integers(300000, 349000 - R - 600))
        rows.append((on, on + int(g.integers(1, 600)), int(g.integers(30, 100)), int(g.integers(1, 128))))
    notes = np.asarray(rows, dtype=np.int64)
    return notes[np.argsort(notes[:, 0], kind="stable")]


def crowd_clip():
    """1500 quiet notes that all sound throughout samples 2048 .. 4096: more than one tile of candidates."""
    g = np.random.default_rng(7)
    n = 1500
    return np.stack([np.sort(g.integers(0, 2000, n)), np.full(n, 8000), g.integers(40, 90, n), np.full(n, 16)],
                    axis=1).astype(np.int64)


def small_clip():
    return np.asarray([(100, 900, 62, 100), (500, 2500, 65, 90), (2600, 4000, 69, 80), (3000, 6000, 48, 127),
                       (3000, 3001, 100, 5)], dtype=np.int64)


CLIPS = [np.zeros((0, 4), np.int64), chord_clip(), crowd_clip(), small_clip()]
SMALL_LEN = int(CLIPS[3][:, 1].max()) + R
WIN_CLIP = [2, 1, 1, 0, 3, 1]                                  # not sorted by clip
WIN_START = [0, 0, 3000, 123, SMALL_LEN - 2000, 350000]


@pytest.fixture(scope="module")
def mirror():
    return SW.windows(CLIPS, WIN_CLIP, WIN_START, WIN)


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _tables(clips):
    notes = np.concatenate(clips)
    off_max = np.concatenate([SW.off_max(c) for c in clips])
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in clips])])
    return _up(notes, np.int64), _up(off_max, np.int64), _up(ptr, np.int64)


def _guarded(w, stride):
    """(whole buffer, (w, stride) view between two guards of 64 int16 -- 128 bytes, so the view is 16-byte aligned)."""
    buf = torch.full((w * stride + 2 * GUARD,), -7777, dtype=torch.int16, device="cuda")
    return buf, buf[GUARD:GUARD + w * stride].view(w, stride)


def _guards_intact(buf):
    return bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == -7777).all().item())


# ---- the reasons ---------------------------------------------------------------------------------------------------------
def test_clips_are_what_they_are_for(mirror):
    chord, crowd = CLIPS[1], CLIPS[2]
    assert len(CLIPS[0]) == 0 and 35 <= len(chord) <= 45 and WIN % CHUNK != 0
    for c in CLIPS:
        assert (np.diff(c[:, 0]) >= 0).all() and (c[:, 1] >= c[:, 0]).all()
    on, off = chord[:, 0], chord[:, 1]
    assert (np.bincount(on)[1000] == 3)                                              # a chord
    same = [(a, b) for a in range(len(chord)) for b in range(a + 1, len(chord))
            if chord[a, 2] == chord[b, 2] == 72 and on[b] < off[a]]
    assert same                                                                      # one pitch, overlapping
    assert ((on // CHUNK == 0) & ((off + R - 1) // CHUNK >= 2) & (off // CHUNK == 2)).any()      # sounds in three chunks
    assert (on % CHUNK == 0).any()                                                   # starts on a chunk's first sample
    assert ((off < WIN) & (off + R > WIN)).any()                                     # release crosses the window's end
    assert np.sort(off - on)[-1] > 20 * np.sort(off - on)[-2]                        # one note far longer than the rest
    om = SW.off_max(chord)
    late = WIN_START[5]                                                              # only the long note sounds there,
    assert (off[1:] + R <= late).all() and off[0] > late + WIN and (om[1:] > off[1:]).all()      # found through off_max
    assert mirror[5].any()
    # the crowd: every note sounds in all of chunk 1 of window 0 -> two tiles there; clamped AND unclamped samples
    assert len(crowd) > TILE and (crowd[:, 0] <= CHUNK).all() and (crowd[:, 1] >= 2 * CHUNK).all()
    total = SW.voice_sum(crowd, 0, WIN)
    assert (np.abs(total) > 32767).sum() > 0 and ((np.abs(total) <= 32767) & (total != 0)).sum() > 0
    assert (total > 32767).any() and (total < -32768).any() and np.abs(total).max() < 1 << 31
    # the windows
    assert WIN_CLIP[1] == WIN_CLIP[2] and 0 < WIN_START[2] - WIN_START[1] < WIN      # two overlapping windows of a clip
    assert np.array_equal(mirror[1][3000:], mirror[2][:2000]) and mirror[2][:2000].any()
    assert WIN_START[1] < on.min() and not mirror[1][:on.min()].any() and mirror[1][on.min():].any()      # starts early
    assert not mirror[3].any()                                                       # the clip without notes
    assert WIN_START[4] + WIN > SMALL_LEN and mirror[4][:1990].any() and not mirror[4][2000:].any()       # past the end
    assert WIN_CLIP != sorted(WIN_CLIP)


# ---- kernel == mirror ----------------------------------------------------------------------------------------------------
def test_windows_equal_the_mirror(mirror):
    from gan_des_midi_music_gen_amd import ops
    notes, off_max, ptr = _tables(CLIPS)
    buf, out = _guarded(len(WIN_CLIP), WIN)
    got = ops.synth_windows(notes, off_max, ptr, _up(WIN_CLIP, np.int32), _up(WIN_START, np.int64), WIN, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (6, WIN) and got.dtype == torch.int16
    got = got.cpu().numpy()
    for w in range(len(WIN_CLIP)):
        bad = np.flatnonzero(got[w] != mirror[w])
        assert bad.size == 0, f"window {w}: {bad.size} samples differ, first at {bad[:5]}"
    assert _guards_intact(buf)
    # the default buffer: rows padded to a multiple of 8, the padding never read back as audio
    got = ops.synth_windows(notes, off_max, ptr, _up(WIN_CLIP, np.int32), _up(WIN_START, np.int64), WIN - 3)
    assert got.shape == (6, WIN) and np.array_equal(got[:, :WIN - 3].cpu().numpy(), mirror[:, :WIN - 3])


def test_real_geometry_beyond_2_to_31():
    from gan_des_midi_music_gen_amd import ops
    base = (1 << 31) + 10 ** 6
    clip = CLIPS[1].copy()
    clip[:, :2] += base
    win_len, stride = 220500, 220504
    start = base - 500
    want = SW.window(clip, start, win_len)
    assert want.any() and clip[:, 0].min() > 1 << 31 and win_len % CHUNK != 0
    assert not np.array_equal(want[500:], SW.window(clip + [1, 1, 0, 0], start, win_len)[500:])    # times matter
    buf, out = _guarded(1, stride)
    ops.synth_windows(_up(clip, np.int64), _up(SW.off_max(clip), np.int64), _up([0, len(clip)], np.int64),
                      _up([0], np.int32), _up([start], np.int64), win_len, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got[0, :win_len], want)
    assert (got[0, win_len:] == -7777).all() and _guards_intact(buf)                # the tail chunk stores i < win_len


def test_equals_synth_pcm_on_ticks():
    from gan_des_midi_music_gen_amd import ops
    g = np.random.default_rng(5)
    on = np.sort(g.integers(0, 3000, 30))
    ticks = np.stack([on, on + g.integers(1, 800, 30), g.integers(30, 100, 30), g.integers(1, 128, 30)], axis=1)
    ticks = ticks.astype(np.int64)
    samples = ticks.copy()
    samples[:, 0] = (ticks[:, 0] * 735) >> 3
    samples[:, 1] = (ticks[:, 1] * 735) >> 3
    assert (np.diff(samples[:, 0]) >= 0).all()
    count = int(samples[:, 1].max()) + R + 100
    old = ops.synth_pcm(_up(ticks[None], np.int64), _up([30], np.int32), 0, count)
    new = ops.synth_windows(_up(samples, np.int64), _up(SW.off_max(samples), np.int64), _up([0, 30], np.int64),
                            _up([0], np.int32), _up([0], np.int64), count)
    assert old.any() and torch.equal(old, new[0, :count])
    assert np.array_equal(old.cpu().numpy(), DR.pcm(ticks, 0, count))


def test_gm_instance_with_the_plain_tables_is_the_plain_instance(mirror):
    """gdm_synth_windows_gm with the plain wave for all 16 families, env = (A, R) and end_max = off_max + R equals
    gdm_synth_windows bit for bit, whatever the programs: A R = 2^21 in both and every product stays below 2^43.  The
    chord clip and the crowd clip (a second tile), their windows above, the full store (WIN) and the tail store."""
    from gan_des_midi_music_gen_amd import ops
    clips = [CLIPS[1], CLIPS[2]]
    picked = [w for w, c in enumerate(WIN_CLIP) if c in (1, 2)]
    win_clip = _up([WIN_CLIP[w] - 1 for w in picked], np.int32)
    win_start = _up([WIN_START[w] for w in picked], np.int64)
    notes, off_max, ptr = _tables(clips)
    twins = [SW.as_gm(c, 31 + i) for i, c in enumerate(clips)]
    rows, end_max = (_up(np.concatenate([t[k] for t in twins]), np.int64) for k in (0, 1))
    assert len(picked) == 4 and len(set(((rows[:, 4] & 127) >> 3).tolist())) == 16 and WIN % 8 == 0
    assert torch.equal(end_max, off_max + R) and torch.equal(rows[:, :4], notes)
    wave, inc = ops.synth_tables(notes.device)
    env = _up([[ops.SYNTH_ATTACK, ops.SYNTH_RELEASE]] * ops.SYNTH_GM_FAMILIES, np.int32)
    tables = (wave.repeat(ops.SYNTH_GM_FAMILIES, 1).contiguous(), env, inc)
    for win_len in (WIN, WIN - 3):
        plain = ops.synth_windows(notes, off_max, ptr, win_clip, win_start, win_len)[:, :win_len]
        gm = ops.synth_windows_gm(rows, end_max, ptr, win_clip, win_start, win_len, tables=tables)[:, :win_len]
        assert torch.equal(gm, plain), f"win_len {win_len}: {int((gm != plain).sum())} samples differ"
        assert np.array_equal(plain.cpu().numpy(), mirror[picked][:, :win_len])


# ---- host checks ---------------------------------------------------------------------------------------------------------
def test_host_checks_return_before_any_launch():
    from gan_des_midi_music_gen_amd import _lib, ops
    lib = _lib.load()
    notes, off_max, ptr = _tables(CLIPS)
    clip, start = _up(WIN_CLIP, np.int32), _up(WIN_START, np.int64)
    wave, inc = ops.synth_tables(notes.device)
    buf, out = _guarded(6, WIN)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(notes=p(notes), off_max=p(off_max), n_total=notes.shape[0], note_ptr=p(ptr), F=4, win_clip=p(clip),
                win_start=p(start), W=6, win_len=WIN, out_stride=WIN, wave=p(wave), inc=p(inc), out=p(out), stream=None)
    bad = [("notes", None), ("off_max", None), ("note_ptr", None), ("win_clip", None), ("win_start", None),
           ("wave", None), ("inc", None), ("out", None),
           ("out", ctypes.c_void_p(out.data_ptr() + 8)), ("notes", ctypes.c_void_p(notes.data_ptr() + 4)),
           ("F", 0), ("W", 0), ("W", 65536), ("win_len", 0), ("win_len", (1 << 30) + 1),
           ("out_stride", WIN - 8), ("out_stride", WIN + 4), ("n_total", -1)]
    for name, value in bad:
        args = dict(good)
        args[name] = value
        if name == "win_len" and value > WIN:
            args["out_stride"] = (1 << 30) + 8
        assert lib.gdm_synth_windows(*args.values()) == -1, f"{name} = {value} was accepted"
        assert b"gdm_synth_windows" in lib.gdm_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7777).all().item()), "a refused call wrote to the output"
    with pytest.raises(ops.GdmError):
        ops.synth_windows(notes.cpu(), off_max, ptr, clip, start, WIN)
    with pytest.raises(ops.GdmError):
        ops.synth_windows(notes, off_max[:-1], ptr, clip, start, WIN)


def test_device_clamps_make_garbage_valid(mirror):
    """A clip index beyond the clips renders the last clip, a negative one the first; row offsets beyond [0, n_total] are
    taken at its ends.  The tables are views with slack around them, so that the values used here would stay inside
    allocated memory even if taken as they are."""
    from gan_des_midi_music_gen_amd import ops
    notes_np = np.concatenate(CLIPS)
    n = len(notes_np)
    slack = np.zeros((8, 4), np.int64)
    notes = _up(np.concatenate([slack, notes_np, slack]), np.int64)[8:8 + n]
    off_max = _up(np.concatenate([np.zeros(8), np.concatenate([SW.off_max(c) for c in CLIPS]), np.zeros(8)]),
                  np.int64)[8:8 + n]
    ptr_np = np.concatenate([[0], np.cumsum([len(c) for c in CLIPS])])
    ptr_np[0], ptr_np[-1] = -3, n + 3                                   # clamped to 0 and n_total
    ptr = _up(np.concatenate([np.zeros(8), ptr_np, np.full(8, n)]), np.int64)[8:8 + len(ptr_np)]
    win_clip = [4 + 3, -2, 2]                                           # -> clip 3, clip 0, clip 2
    win_start = [WIN_START[4], WIN_START[3], WIN_START[0]]
    got = ops.synth_windows(notes, off_max, ptr, _up(win_clip, np.int32), _up(win_start, np.int64), WIN).cpu().numpy()
    assert np.array_equal(got, mirror[[4, 3, 0]])


# ---- the dataset ---------------------------------------------------------------------------------------------------------
def _performance(seed, seconds, pedal_every=4):
    """A two-track file at the default tempo (960 ticks per second): a tempo track and notes with pedal work."""
    g = np.random.default_rng(seed)
    track, t, end = [], 0, int(seconds * 960)
    k = 0
    while t < end - 800:                                   # gap + dur < 800: the closing delta stays positive
        if k % pedal_every == 0:
            track.append((0, ("cc", 0, 64, 127 if (k // pedal_every) % 2 == 0 else 0)))
        pitch, vel = int(g.integers(40, 90)), int(g.integers(30, 120))
        gap, dur = int(g.integers(20, 300)), int(g.integers(50, 500))
        track += [(gap, ("on", 0, pitch, vel)), (dur, ("off", 0, pitch, 0))]
        t += gap + dur
        k += 1
    track.append((end - t, ("cc", 0, 64, 0)))
    return SW.midi_bytes([[(0, ("tempo", 500000))], track])


@pytest.fixture(scope="module")
def maestro(tmp_path_factory):
    root = tmp_path_factory.mktemp("maestro-v3.0.0")
    names = {"0": "2004/first.midi", "1": "2006/second.midi", "2": "2006/short.midi"}
    os.makedirs(root / "2004")
    os.makedirs(root / "2006")
    for (key, name), seconds in zip(names.items(), (13.0, 18.5, 2.5)):
        (root / name).write_bytes(_performance(20 + int(key), seconds))
    (root / "maestro-v3.0.0.json").write_text(json.dumps({"midi_filename": names, "split": {k: "train" for k in names}}))
    from gan_des_midi_music_gen_amd import datasets
    ds = datasets.MaestroDataset(30, input_folder=str(root))
    return root, names, ds, [ds[i] for i in range(3)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_dataset_items(maestro):
    from gan_des_midi_music_gen_amd import datasets, util
    root, names, ds, items = maestro
    assert len(ds) == 3 and ds.k == 30 and ds.INPUT_FOLDER == str(root) and ds.data == names
    assert ds.meta_data_file == f"{root}/maestro-v3.0.0.json"
    counts = []
    for i, item in enumerate(items):
        _notes, clip_len = datasets.midi_notes(str(root / names[str(i)]))
        windows = util.song_windows(clip_len, 44100, 5, 5, mode="split")
        counts.append(len(windows))
        assert item.shape == (len(windows), 128, 216) and item.dtype == torch.float32 and item.is_cuda
        assert bool(torch.isfinite(item).all().item())
    assert counts[0] >= 3 and counts[1] >= 4 and counts[2] == 1                    # the last: one window under 5 s
    assert datasets.midi_notes(str(root / names["2"]))[1] < 5 * 44100


def test_dataset_equals_the_wav_route(maestro, tmp_path):
    from gan_des_midi_music_gen_amd import datasets, util
    root, names, _ds, items = maestro
    for i, item in enumerate(items):
        wav = str(tmp_path / f"{i}.wav")
        _notes, clip_len = datasets.midi_notes(str(root / names[str(i)]))
        assert datasets.midi_to_wav(str(root / names[str(i)]), wav) == clip_len
        splits = util.split_audio_data(wav)
        assert len(splits) == len(item)
        for w, split in enumerate(splits):
            want = util.get_melspectrogram_db_tensor(split)
            assert torch.equal(_bits(item[w]), _bits(want)), f"file {i}, window {w}"
    # the file itself: the mirror's samples behind the shared header
    notes, clip_len = datasets.midi_notes(str(root / names["2"]))
    raw = open(str(tmp_path / "2.wav"), "rb").read()
    assert raw == DR.wav_bytes(SW.window(notes, 0, clip_len))
    assert datasets.midi_to_wav(str(root / names["0"]), str(tmp_path / "cut.wav"), max_seconds=0.5) == 22050
    assert len(open(str(tmp_path / "cut.wav"), "rb").read()) == 44 + 2 * 22050


def test_dataset_draws_like_random_sample(maestro):
    from gan_des_midi_music_gen_amd import datasets
    root, _names, _ds, items = maestro
    small = datasets.MaestroDataset(2, input_folder=str(root))
    n = len(items[1])
    random.seed(99)
    want = random.sample(list(range(n)), 2)
    state = random.getstate()
    random.seed(99)
    got = small[1]
    assert random.getstate() == state and got.shape == (2, 128, 216)
    assert torch.equal(_bits(got), _bits(items[1][want]))
    assert torch.equal(_bits(small[2]), _bits(items[2]))                           # one window <= k: no draw


def test_spectrograms_collate_and_dataloader(maestro):
    from gan_des_midi_music_gen_amd import datasets
    _root, _names, ds, items = maestro
    everything = torch.cat(items)
    assert torch.equal(_bits(ds.spectrograms([0, 1, 2])), _bits(everything))
    assert torch.equal(_bits(ds.spectrograms()), _bits(everything))
    assert torch.equal(_bits(ds.spectrograms([2, 0])), _bits(torch.cat([items[2], items[0]])))
    assert torch.equal(_bits(datasets.my_collate([items[1], items[2]])), _bits(torch.cat([items[1], items[2]])))
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, collate_fn=datasets.my_collate, num_workers=0)
    batches = list(loader)
    assert len(batches) == 3
    for got, want in zip(batches, items):
        assert torch.equal(_bits(got), _bits(want))


def test_train_on_a_maestro_folder(maestro):
    from gan_des_midi_music_gen_amd import SIMNN
    root = str(maestro[0])
    _gen, _disc, g_losses, d_losses = SIMNN.train(maestro_dir=root, batch_size=4, max_steps=2, save=False, seed=0,
                                                  log=lambda *_: None)
    assert len(g_losses) == len(d_losses) == 2 and np.isfinite(g_losses).all() and np.isfinite(d_losses).all()
    with pytest.raises(ValueError):
        SIMNN.train(maestro_dir=root, audio_file="song.wav")
    with pytest.raises(ValueError):
        SIMNN.train(maestro_dir=root, dataloader=[])
    SIMNN.main(["--maestro-dir", root, "--batch-size", "4", "--max-steps", "1", "--no-save"])
