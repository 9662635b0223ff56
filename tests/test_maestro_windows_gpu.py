"""GPU: model 2's real-data route -- the windowed raster kernel (gdm_piano_roll_windows), ``MaestroWindows`` and its
loaders, ``training_loop(midi_dir=... / pickle_file=...)`` and the command line -- against the pure-Python mirror of
notebook cells 10-11 (tests/maestro_windows_ref.py) and against the per-file kernel.  PARITY UNPINNED as the mirror
says.  Planes hold small integers in fp32 and beats are float32 casts of the same float64 values: every comparison
asks for equal bits."""
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import maestro_windows_ref as R
from gan_des_midi_music_gen_amd import datasets as ds, ops
from oracle import midi_events as ome, piano_roll as opr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MIDI_DIR = os.path.join(HERE, "golden", "midi")
FILES = sorted(glob.glob(os.path.join(MIDI_DIR, "*.mid")))
SYNTH = R.synthetic_files()
SOURCES = FILES + list(SYNTH.values())
DEV = "cuda"
_mirror_cache = {}


def mirror(sample_size, length, sources=None):
    """The mirror's dataset for SOURCES (computed once per case and shared; callers do not modify it)."""
    if sources is not None:
        return R.dataset(sources, sample_size, length)
    key = (sample_size, length)
    if key not in _mirror_cache:
        _mirror_cache[key] = R.dataset(SOURCES, sample_size, length)
    return _mirror_cache[key]


def stacked(items):
    return tuple(torch.from_numpy(np.stack([it[k] for it in items])) for k in range(3))


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)


def upload_events(sources, sample_size):
    """CSR row events of ``sources`` as the raster kernels take them (device int32 tensors)."""
    ptrs, steps, vels, total = [np.zeros(1, np.int32)], [], [], 0
    for src in sources:
        rp, st, ve = ds._row_events(ds.read_midi(src), sample_size, sample_size)
        ptrs.append(rp[1:] + total)
        total += int(rp[-1])
        steps.append(st)
        vels.append(ve)
    return tuple(torch.from_numpy(np.concatenate(a)).to(DEV) for a in (ptrs, steps, vels))


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("sample_size,length,fixture_windows", [(40, 5, 91), (24, 4, 99), (300, 10, 27), (48, 16, 8)])
def test_from_midi_matches_the_mirror(sample_size, length, fixture_windows):
    items, file_index, window_index = mirror(sample_size, length)
    assert int((file_index < len(FILES)).sum()) == fixture_windows
    data = ds.MaestroWindows.from_midi(SOURCES, sample_size, length, device=DEV)
    assert len(data) == len(items) > fixture_windows
    assert np.array_equal(data.file_index, file_index) and np.array_equal(data.window_index, window_index)
    roll, dur, beats = stacked(items)
    assert data.piano_roll.is_cuda and same(data.piano_roll, roll) and same(data.durations, dur)
    assert same(data.beats, beats)
    for n in (0, len(items) - 1):                                     # beats straight from the oracle's beat grid
        src = SOURCES[file_index[n]]
        raw = src if isinstance(src, bytes) else open(src, "rb").read()
        want = opr.get_beats(*ome.read_tracks(raw))
        want = np.pad(want, (0, max(0, 50 - len(want))))[:50].astype(np.float32)
        assert np.array_equal(data.beats[n].cpu().numpy(), want)
    got = data[len(items) - 1]
    assert got[0].data_ptr() == data.piano_roll[-1].data_ptr() and same(got[1], dur[-1]) and same(got[2], beats[-1])


def test_from_midi_reads_a_directory_and_refuses_an_empty_result():
    by_dir = ds.MaestroWindows.from_midi(MIDI_DIR, 48, 16, device=DEV, pattern="*.mid")
    by_list = ds.MaestroWindows.from_midi(FILES, 48, 16, device=DEV)
    assert len(by_dir) == 8 and by_dir.files == FILES and torch.equal(by_dir.piano_roll, by_list.piano_roll)
    assert by_dir.beats.shape == (8, 50) and by_dir.sequence_length == 16 and by_dir.sample_size == 48
    with pytest.raises(ValueError, match=r"30 files.*2 \* sequence_length"):
        ds.MaestroWindows.from_midi(MIDI_DIR, 300, 50, device=DEV)


@pytest.mark.parametrize("length", [5, 50, 128])
def test_kernel_matches_slices_of_the_per_file_kernel(length):
    """Any window list: window 0, overlapping windows, odd first steps, a window ending at the plane's last column."""
    sample_size = 300
    full_roll, full_dur, _ = ds.generate_piano_rolls(SOURCES, sample_size, start=0, end=sample_size, device=DEV)
    assert full_roll.shape == (len(SOURCES), 128, sample_size)
    firsts = [0, 1, length - 1, length, length + 3, sample_size - length, sample_size - length - 1, 7, 7]
    windows = [(f, s0) for f in range(len(SOURCES)) for s0 in firsts[f % 3::3] + [0, sample_size - length]]
    roll, dur = ops.piano_roll_windows(*upload_events(SOURCES, sample_size), i32([w[0] for w in windows]),
                                       i32([w[1] for w in windows]), length)
    assert roll.shape == dur.shape == (len(windows), 128, length)
    want_roll = torch.stack([full_roll[f, :, s0:s0 + length] for f, s0 in windows])
    want_dur = torch.stack([full_dur[f, :, s0:s0 + length] for f, s0 in windows])
    assert torch.equal(roll, want_roll) and torch.equal(dur, want_dur)
    assert int((roll != 0).sum()) > 0 and int((dur != 0).sum()) > 0


def test_durations_cross_windows_with_their_full_length():
    """A note held from step 3 to step 23 reads 20 in every window it crosses; a note struck twice before its note_off
    counts from the later note_on (cell 10 overwrites note_on_time)."""
    sec = 960
    held = [(3 * sec, b"\x90\x3c\x40"), (20 * sec, b"\x80\x3c\x00"),                     # note 60: 3 .. 23
            (0, b"\x90\x3e\x50"), (4 * sec, b"\x90\x3e\x51"), (6 * sec, b"\x80\x3e\x00"),   # note 62: 23, 27 .. 33
            (20 * sec, b"\x90\x40\x01")]                                                  # keeps the loop going to 53
    src = R.smf([held])
    length = 5
    events = upload_events([src], 60)
    firsts = list(range(0, 40, length)) + [2, 21]
    roll, dur = ops.piano_roll_windows(*events, i32([0] * len(firsts)), i32(firsts), length)
    roll, dur = roll.cpu().numpy(), dur.cpu().numpy()
    want_roll, want_dur = np.zeros((128, 60), np.float32), np.zeros((128, 60), np.float32)
    want_roll[60, 3], want_roll[62, 23], want_roll[62, 27], want_roll[64, 53] = 0x40, 0x50, 0x51, 1
    want_dur[60, 3:23] = 20
    want_dur[62, 27:33] = 6                                            # 33 - 27, not 33 - 23; steps 23..26 stay zero
    for n, s0 in enumerate(firsts):
        assert np.array_equal(roll[n], want_roll[:, s0:s0 + length]), s0
        assert np.array_equal(dur[n], want_dur[:, s0:s0 + length]), s0
    crossed = [n for n, s0 in enumerate(firsts) if s0 < 23 and s0 + length > 3]
    assert len(crossed) >= 6 and all(set(dur[n][60].tolist()) <= {0.0, 20.0} and 20.0 in dur[n][60] for n in crossed)
    # the mirror builds the same planes from the same bytes
    m_roll, m_dur, _b, _t = R.generate_piano_roll(src, 60)
    assert np.array_equal(m_roll, want_roll) and np.array_equal(m_dur, want_dur)


def test_a_file_gives_the_same_planes_alone_and_in_the_list():
    sample_size, length = 40, 5
    full = ds.MaestroWindows.from_midi(SOURCES, sample_size, length, device=DEV)
    empty = [i for i in range(len(SOURCES)) if i not in set(full.file_index.tolist())]
    assert len(empty) >= 7                                            # files without a window sit between the others
    assert any(0 < i < max(full.file_index) for i in empty)
    for i, src in enumerate(SOURCES):
        rows = np.flatnonzero(full.file_index == i)
        if not len(rows):
            with pytest.raises(ValueError):
                ds.MaestroWindows.from_midi([src], sample_size, length, device=DEV)
            continue
        alone = ds.MaestroWindows.from_midi([src], sample_size, length, device=DEV)
        sl = slice(rows[0], rows[-1] + 1)
        assert len(alone) == len(rows) and np.array_equal(alone.window_index, full.window_index[sl])
        assert torch.equal(alone.piano_roll, full.piano_roll[sl]) and torch.equal(alone.durations, full.durations[sl])
        assert torch.equal(alone.beats, full.beats[sl])


def test_kernel_writes_its_windows_and_nothing_else():
    """Outputs that are slices of larger sentinel-filled buffers: nothing outside the N windows changes, and nothing
    inside them keeps the sentinel (the kernel clears what no message writes)."""
    sample_size, length, sentinel = 40, 5, -777.0
    events = upload_events(SOURCES, sample_size)
    windows = [(f, s0) for f in range(len(SOURCES)) for s0 in (0, 5, 33)]
    n, pad = len(windows), 3
    bufs = [torch.full((n + 2 * pad, 128, length), sentinel, device=DEV) for _ in range(2)]
    roll, dur = ops.piano_roll_windows(*events, i32([w[0] for w in windows]), i32([w[1] for w in windows]), length,
                                       roll=bufs[0][pad:pad + n], dur=bufs[1][pad:pad + n])
    assert roll.data_ptr() == bufs[0][pad].data_ptr() and dur.data_ptr() == bufs[1][pad].data_ptr()
    for buf in bufs:
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all())
        assert not bool((buf[pad:pad + n] == sentinel).any())
    fresh_roll, fresh_dur = ops.piano_roll_windows(*events, i32([w[0] for w in windows]), i32([w[1] for w in windows]),
                                                   length)
    assert torch.equal(roll, fresh_roll) and torch.equal(dur, fresh_dur) and int((fresh_roll != 0).sum()) > 0


def test_wrapper_refuses_bad_arguments_before_the_launch():
    row_ptr, ev_step, ev_vel = upload_events(SOURCES[:2], 40)
    ok = dict(win_file=i32([0, 1]), win_s0=i32([0, 5]), length=5)
    ops.piano_roll_windows(row_ptr, ev_step, ev_vel, **ok)                        # the good call goes through

    def refused(**kw):
        args = dict(row_ptr=row_ptr, ev_step=ev_step, ev_vel=ev_vel, **ok)
        args.update(kw)
        with pytest.raises(ops.GdmError):
            ops.piano_roll_windows(**args)

    refused(win_file=i32([]), win_s0=i32([]))                                     # N = 0
    refused(length=ops.PIANO_ROLL_WINDOW_MAX + 1)                                 # more LDS than a workgroup has
    refused(length=0)
    refused(row_ptr=row_ptr.cpu())                                                # a CPU tensor
    refused(win_s0=ok["win_s0"].cpu())
    bent = row_ptr.clone()
    bent[5] = bent[-1] + 1                                                        # not monotone
    refused(row_ptr=bent)
    refused(row_ptr=row_ptr + 1)                                                  # does not end at len(ev_step)
    refused(win_file=i32([0, 2]))                                                 # file index out of range
    refused(win_file=i32([-1, 0]))
    refused(win_s0=i32([0, -1]))
    refused(win_s0=i32([0, 2 ** 31 - 3]))                                         # s0 + L overflows
    refused(row_ptr=row_ptr[:-1])                                                 # not 128 * files + 1 offsets
    refused(win_file=ok["win_file"].long())
    refused(roll=torch.empty((2, 128, 6), device=DEV))                            # preallocated output of another shape
    # the C entry refuses the same length on its own, on the host
    from gan_des_midi_music_gen_amd import _lib
    lib = _lib.load()
    one = torch.zeros(4, dtype=torch.int32, device=DEV).data_ptr()
    assert lib.gdm_piano_roll_windows(one, one, one, one, one, 1, ops.PIANO_ROLL_WINDOW_MAX + 1, one, one, None) == -1
    assert b"LDS" in lib.gdm_last_error()
    assert lib.gdm_piano_roll_windows(one, one, one, one, one, 0, 5, one, one, None) == -1


def test_batches_are_views_and_equal_the_dataloader_collation():
    items, _fi, _wi = mirror(24, 4)
    data = ds.MaestroWindows.from_midi(SOURCES, 24, 4, device=DEV)
    n, b = len(data), 4
    assert n % b != 0                                                 # there is a tail to drop
    got = list(data.batches(b))
    assert len(got) == n // b == len(data.batches(b))
    for k, (roll, dur, beats) in enumerate(got):
        assert roll.data_ptr() == data.piano_roll.data_ptr() + k * b * 128 * 4 * 4
        assert dur.data_ptr() == data.durations.data_ptr() + k * b * 128 * 4 * 4
        assert beats.data_ptr() == data.beats.data_ptr() + k * b * 50 * 4
        assert roll.shape == (b, 128, 4) and beats.shape == (b, 50)
    want = list(torch.utils.data.DataLoader(data, batch_size=b, drop_last=True))   # the reference's loader, on views
    assert len(want) == len(got)
    assert all(torch.equal(g, w) for gb, wb in zip(got, want) for g, w in zip(gb, wb))
    m_roll, m_dur, m_beats = stacked(items)
    assert same(torch.cat([g[0] for g in got]), m_roll[:n // b * b])
    assert same(torch.cat([g[1] for g in got]), m_dur[:n // b * b])
    assert same(torch.cat([g[2] for g in got]), m_beats[:n // b * b])
    assert len(list(data.batches(b, drop_last=False))) == n // b + 1
    # shuffled: an epoch is a permutation of the items it uses, the same for the three tensors, seeded by the generator
    tag = torch.arange(n, dtype=torch.float32, device=DEV)
    marked = ds.MaestroWindows(data.piano_roll, tag[:, None, None].expand(n, 128, 4).contiguous(),
                               tag[:, None].expand(n, 50).contiguous(), data.file_index, data.window_index, 24)
    epoch = list(marked.batches(b, drop_last=False, shuffle=True, generator=torch.Generator().manual_seed(5)))
    order = torch.cat([bt[1][:, 0, 0] for bt in epoch]).long()
    assert sorted(order.tolist()) == list(range(n)) and order.tolist() != list(range(n))
    assert torch.equal(torch.cat([bt[2][:, 0] for bt in epoch]).long(), order)
    assert torch.equal(torch.cat([bt[0] for bt in epoch]), data.piano_roll[order])
    dropped = list(marked.batches(b, shuffle=True, generator=torch.Generator().manual_seed(5)))
    assert torch.equal(torch.cat([bt[1][:, 0, 0] for bt in dropped]).long(), order[:n // b * b])


def test_round_trips(tmp_path):
    data = ds.MaestroWindows.from_midi(SOURCES, 40, 5, device=DEV)
    # to_pickle -> MaestroDatasetPickle: the reference's format, a list of CPU float32 tensor triples
    data.to_pickle(tmp_path / "preprocessed_data_5.pkl")
    with open(tmp_path / "preprocessed_data_5.pkl", "rb") as f:
        raw = pickle.load(f)
    assert isinstance(raw, list) and len(raw) == len(data) and isinstance(raw[0], tuple) and len(raw[0]) == 3
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in raw[0])
    assert raw[0][0].shape == (128, 5) and raw[0][2].shape == (50,)
    for device in ("cpu", DEV):
        back = ds.MaestroDatasetPickle("preprocessed_data_5.pkl", 5, 50, device, data_dir=str(tmp_path))
        assert back.piano_roll.device.type == torch.device(device).type and len(back) == len(data)
        for name in ("piano_roll", "durations", "beats"):
            assert torch.equal(getattr(back, name).cpu(), getattr(data, name).cpu())
    # save -> load: plain tensors
    data.save(tmp_path / "windows.pt")
    assert isinstance(torch.load(tmp_path / "windows.pt", weights_only=True), dict)
    back = ds.MaestroWindows.load(tmp_path / "windows.pt", device=DEV)
    for name in ("piano_roll", "durations", "beats"):
        assert getattr(back, name).is_cuda and torch.equal(getattr(back, name), getattr(data, name))
    assert np.array_equal(back.file_index, data.file_index) and np.array_equal(back.window_index, data.window_index)
    assert (back.sample_size, back.sequence_length, back.beats_length) == (40, 5, 50)
    # write_torch_files -> MaestroDatasetTorch: notebook cell 9's per-file tuples
    few = FILES[:7]
    paths = ds.write_torch_files(few, tmp_path / "tensors", sequence_length=100, beats_length=50, device=DEV)
    assert [os.path.basename(p) for p in paths] == [f"data_{i}.pt" for i in range(7)]
    per_file = ds.MaestroDatasetTorch(str(tmp_path / "tensors"), device=DEV)
    roll, dur, beats = ds.generate_piano_rolls(few, 100, 50, device=DEV)
    assert len(per_file) == 7
    for i in range(7):
        item = per_file[i]
        assert item[0].is_cuda and item[0].shape == (128, 50)
        assert torch.equal(item[0], roll[i]) and torch.equal(item[1], dur[i]) and torch.equal(item[2], beats[i])


def test_training_loop_on_midi_files_end_to_end(tmp_path):
    """48 / 16 gives 8 windows over the fixtures: 2 steps of 4 per epoch.  The same data three ways -- midi_dir, batches
    made by hand from the mirror's windows, the reference's pickle -- gives the same loss lists, bit for bit."""
    from gan_des_midi_music_gen_amd import network_tests as NT
    kw = dict(sequence_length=16, num_epochs=2, seed=7, log=lambda *_a: None)
    d_midi, g_midi = NT.training_loop(4, midi_dir=MIDI_DIR, sample_size=48, **kw)
    assert len(d_midi) == len(g_midi) == 2 and np.all(np.isfinite(d_midi + g_midi))
    items, _fi, _wi = mirror(48, 16, sources=FILES)
    assert len(items) == 8
    roll, dur, beats = stacked(items)
    by_hand = [(roll[k:k + 4], dur[k:k + 4], beats[k:k + 4]) for k in (0, 4)]
    d_hand, g_hand = NT.training_loop(4, train_loader=by_hand, **kw)
    assert d_hand == d_midi and g_hand == g_midi
    R.write_pickle(items, tmp_path / "preprocessed_data_16.pkl")
    d_pkl, g_pkl = NT.training_loop(4, pickle_file=str(tmp_path / "preprocessed_data_16.pkl"), **kw)
    assert d_pkl == d_midi and g_pkl == g_midi
    with pytest.raises(ValueError, match="fewer than one batch"):
        NT.training_loop(16, midi_dir=MIDI_DIR, sample_size=48, **kw)


def test_command_line_trains_on_a_midi_folder():
    r = subprocess.run([sys.executable, "-m", "gan_des_midi_music_gen_amd.network_tests", "--midi-dir", MIDI_DIR,
                        "--sample-size", "48", "--sequence-length", "16", "--batch-size", "4", "--epochs", "1",
                        "--max-steps", "1"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch 1/1, Batch 0" in r.stdout
