"""CPU: the host side of model 2's real-data route -- ``datasets.window_plan`` (which windows notebook cell 11 keeps of
a file, from cell 10's ``total_time``), ``MaestroDatasetPickle`` on the CPU, and ``training_loop``'s argument check --
against the pure-Python mirror of the notebook (tests/maestro_windows_ref.py).  PARITY UNPINNED as the mirror says; all
comparisons are on integers or on float32 casts of the same float64 values, so they ask for equality."""
import glob
import os

import numpy as np
import pytest
import torch

import maestro_windows_ref as R
from gan_des_midi_music_gen_amd import datasets as ds

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "golden", "midi", "*.mid")))
SYNTH = R.synthetic_files()
GRID = ((300, 50), (300, 10), (40, 5), (24, 4), (48, 16), (7, 3))
# windows the 30 fixture files yield, computed once from oracle.midi_events: no case passes on an empty set
FIXTURE_WINDOWS = {(40, 5): 91, (24, 4): 99, (300, 10): 27, (48, 16): 8, (300, 50): 0}


def _sources():
    return [(os.path.basename(f), f) for f in FILES] + list(SYNTH.items())


def _mismatches(faults=()):
    """Cases (name, sample_size, L) on which the plan and the mirror (with ``faults`` planted) differ."""
    out = []
    for (sample_size, length) in GRID:
        for name, src in _sources():
            total, kept, _items = R.file_windows(src, sample_size, length, faults=faults)
            p_total, p_kept, _ev = ds.window_plan(src, sample_size, length)
            if total != p_total or kept != p_kept.tolist():
                out.append((name, sample_size, length, (total, kept), (p_total, p_kept.tolist())))
    return out


def test_fixture_set_is_complete():
    assert len(FILES) == 30


def test_plan_matches_the_mirror():
    assert _mismatches() == []


@pytest.mark.parametrize("case", sorted(FIXTURE_WINDOWS))
def test_window_counts_over_the_fixtures_are_pinned(case):
    sample_size, length = case
    mirror = [R.file_windows(f, sample_size, length) for f in FILES]
    plan = [ds.window_plan(f, sample_size, length) for f in FILES]
    assert sum(len(k) for _t, k, _i in mirror) == FIXTURE_WINDOWS[case]
    assert sum(len(k) for _t, k, _e in plan) == FIXTURE_WINDOWS[case]
    for (total, kept, _i) in mirror:                                  # the closed form the plan documents
        assert len(kept) == max(0, min(total // length, sample_size // length) - 1)
        assert kept == list(range(1, 1 + len(kept)))
    if case == (40, 5):
        assert sum(1 for _t, k, _i in mirror if not k) == 7
        assert all(roll.any() for _t, _k, items in mirror for roll, _d, _b in items)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_checker_rejects_planted_faults(fault):
    assert _mismatches(faults=(fault,)), f"a mirror with the fault {fault!r} agrees with the plan on every case"


def test_synthetic_files_exercise_what_they_claim():
    total = {name: R.file_windows(src, 300, 10)[0] for name, src in SYNTH.items()}
    assert total["eot_gap_5000"] > total["eot_gap_0"]                 # the final end_of_track's delta counts
    assert ds.window_plan(SYNTH["eot_gap_5000"], 300, 10)[0] == total["eot_gap_5000"]
    assert total["jump_beyond_sample_size"] > 300                     # the message that triggers `break` is included
    assert total["format0_one_note_long_gap"] == 53                   # 3 s of notes + 50 s of gap
    assert ds.read_midi(SYNTH["format0_one_note_long_gap"]).format == 0
    assert ds.read_midi(SYNTH["empty_track"]).track.tolist().count(0) == 0          # track 0 holds no message
    # running times 0.5, 6.5, 7.5, 12.5, 24.5: the steps are 0, 6, 8, 12, 24 (half to even), so a break at 7 sees 8
    assert R.file_windows(SYNTH["half_steps"], 300, 10)[0] == 24
    assert R.file_windows(SYNTH["half_steps"], 7, 3)[0] == 8 == ds.window_plan(SYNTH["half_steps"], 7, 3)[0]


def test_plan_refuses_non_positive_sizes():
    for (sample_size, length) in ((300, 0), (300, -5), (0, 50), (-1, 50)):
        with pytest.raises(ValueError):
            ds.window_plan(FILES[0], sample_size, length)
        with pytest.raises(ValueError):
            ds.MaestroWindows.from_midi(FILES[:1], sample_size, length, device="cpu")


def test_from_midi_without_any_window_raises_before_the_device():
    with pytest.raises(ValueError, match=r"30 files.*2 \* sequence_length"):
        ds.MaestroWindows.from_midi(FILES, 300, 50, device="cpu")


@pytest.fixture(scope="module")
def mirror_set():
    return R.dataset(FILES + list(SYNTH.values()), 24, 4)


def test_pickle_dataset_on_the_cpu(tmp_path, mirror_set):
    items, _fi, _wi = mirror_set
    assert len(items) > 99 and len(items) % 4
    R.write_pickle(items, tmp_path / "preprocessed_data_4.pkl")
    data = ds.MaestroDatasetPickle("preprocessed_data_4.pkl", sequence_length=4, device="cpu", data_dir=str(tmp_path))
    assert len(data) == len(items) and data.piano_roll.device.type == "cpu"
    for i in (0, 1, len(items) // 2, len(items) - 1, -1):
        got = data[i]
        assert [t.dtype for t in got] == [torch.float32] * 3
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, items[i]))
    assert data[3][0].data_ptr() == data.piano_roll[3].data_ptr()                 # items are views
    with pytest.raises(IndexError):
        data[len(items)]

    class Upstream(torch.utils.data.Dataset):                         # the reference's item access (datasets.py:73-87)
        def __len__(self):
            return len(items)

        def __getitem__(self, idx):
            return tuple(torch.from_numpy(a) for a in items[idx])

    want = list(torch.utils.data.DataLoader(Upstream(), batch_size=4, drop_last=True))
    got = list(data.batches(4))
    assert len(got) == len(want) == len(items) // 4 == len(data.batches(4))
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))
    assert got[1][0].data_ptr() == data.piano_roll[4].data_ptr()                  # unshuffled batches are views
    assert len(list(data.batches(4, drop_last=False))) == -(-len(items) // 4)
    again = list(data.batches(4))                                                 # re-iterable: one epoch per iter()
    assert torch.equal(again[0][0], got[0][0])
    gen = torch.Generator().manual_seed(3)
    shuffled = torch.cat([b[0] for b in data.batches(4, drop_last=False, shuffle=True, generator=gen)])
    assert shuffled.shape == data.piano_roll.shape and not torch.equal(shuffled, data.piano_roll)
    assert torch.equal(shuffled.flatten(1).sum(0), data.piano_roll.flatten(1).sum(0))


def test_training_loop_refuses_two_data_sources(tmp_path):
    from gan_des_midi_music_gen_amd.network_tests import training_loop
    for kw in ({"train_loader": [], "midi_dir": str(tmp_path)}, {"midi_dir": str(tmp_path), "pickle_file": "x.pkl"},
               {"train_loader": [], "pickle_file": "x.pkl"},
               {"train_loader": [], "midi_dir": str(tmp_path), "pickle_file": "x.pkl"}):
        with pytest.raises(ValueError, match="at most one"):
            training_loop(4, num_epochs=1, device="cpu", **kw)
