"""GPU: model 1's built-in DES bridge -- log -> notes (csrc/des_notes.hip), the integer synth as STFT frames and as PCM
(csrc/synth.hip) -- and the Python surface on top: sim_log_process_music, matrix_to_wav(simulate="des"),
SIMNN.train(fake_provider="des"), SIMNN.generate_song(bridge="des").

Every stage is integer arithmetic defined by this package, so every comparison with the mirror (tests/des_notes_ref.py)
demands equal bits; the note stage is also held to the rows recorded from the reference (tests/golden/des_notes.npz).
The mel chain behind the stages is the existing one and keeps test_mel.py's tolerances.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import des_notes_ref as N  # noqa: E402
from test_des_notes_ref import GOLD, NAMES, case_log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DIM = 15
_cache = {}


def events(rec):
    from gan_des_midi_music_gen_amd.simulation_v3 import EVENT_DTYPE
    out = np.zeros(len(rec["value"]), dtype=EVENT_DTYPE)
    for k in ("value", "event_id", "node", "kind"):
        out[k] = rec[k]
    return out


def levels(name):
    """The case's note levels, padded to 15 nodes so that cases of both sizes share a launch."""
    lv = [int(x) for x in GOLD[f"{name}/note_levels"]]
    return lv + [0] * (DIM - len(lv))


def stage_a_cases():
    """(name, log, note levels, mirror result): the fixture's logs plus an empty one.  Computed once."""
    if "a" not in _cache:
        cases = [(n, events(case_log(n)), levels(n)) for n in NAMES]
        cases.append(("empty", events({k: np.zeros(0) for k in ("value", "event_id", "node", "kind")}), [60] * DIM))
        _cache["a"] = [(n, lg, lv, N.log_to_notes({k: lg[k] for k in lg.dtype.names}, lv)) for n, lg, lv in cases]
    return _cache["a"]


@pytest.mark.parametrize("batch", [1, 3])
def test_stage_a_equals_mirror_and_recorded_rows(batch):
    from gan_des_midi_music_gen_amd.sim_log_process_music import log_to_notes
    cases = stage_a_cases()
    assert {"empty", "lines_5003"} <= {c[0] for c in cases} and len({len(c[1]) for c in cases}) > 5     # ragged
    for a in range(0, len(cases), batch):
        part = cases[a:a + batch]
        notes, n_notes, clip_len = log_to_notes([c[1] for c in part], [[0] * DIM] * len(part), [c[2] for c in part])
        assert notes.is_cuda and notes.dtype == torch.int64 and notes.shape == (len(part), 5000, 4)
        assert n_notes.dtype == torch.int32 and clip_len.dtype == torch.int64
        notes, n_notes, clip_len = notes.cpu().numpy(), n_notes.cpu().numpy(), clip_len.cpu().numpy()
        for i, (name, _log, _lv, (want, want_len, status)) in enumerate(part):
            assert status == N.OK
            assert n_notes[i] == len(want) and clip_len[i] == want_len, name
            assert np.array_equal(notes[i, :n_notes[i]], want), name
            assert not notes[i, n_notes[i]:].any(), name
            if name != "empty":                                 # the kernel against the reference's own rows
                rows = [tuple(int(x) for x in r) for r in GOLD[f"{name}/rows"]]
                assert np.array_equal(notes[i, :n_notes[i]], N.rows_to_notes(rows)[0]), name
    assert sum(len(c[3][0]) for c in cases) > 2000


def test_stage_a_error_statuses():
    from gan_des_midi_music_gen_amd import ops
    from gan_des_midi_music_gen_amd.sim_log_process_music import log_to_notes
    log = events(case_log("repeated_departures"))               # notes on node 2; a silent departure on node 3
    with pytest.raises(ValueError):
        log_to_notes([log], [[0, 0]], [[60, 64]])               # node 2 has no note level (KeyError upstream)
    with pytest.raises(ValueError):
        log_to_notes([log], [[0] * 4], [[60, 64, 128, 0]])      # mido refuses note 128
    with pytest.raises(ValueError):
        log_to_notes([log, log], [[0] * 4] * 2, [[60, 64, 67, 0], [60, 64, -1, 0]])
    notes, n_notes, _ = log_to_notes([log], [[0] * 3], [[60, 64, 67]])          # node 3 never sounds: nothing raised
    assert int(n_notes[0]) == 3
    # an overlong clip is blank, not an error: the second delta time alone passes 2^40 samples
    long_log = events({"value": np.asarray([1.0, 2e10]), "event_id": np.asarray([3, 3]), "node": np.asarray([0, 0]),
                       "kind": np.asarray([0, 1])})
    assert N.log_to_notes({k: long_log[k] for k in long_log.dtype.names}, [60])[2] == N.ELONG
    fine = events(case_log("values"))
    notes, n_notes, clip_len = log_to_notes([fine, long_log, fine], [[0] * 4] * 3, [[60, 62, 64, 65]] * 3)
    assert n_notes.tolist() == [3, 0, 3] and clip_len[1].item() == 0 and clip_len[0].item() == clip_len[2].item() > 0
    with pytest.raises(ops.GdmError):
        log_to_notes([fine], [[0] * 300], [[60] * 300])         # dim beyond the kernel's limit
    with pytest.raises(ops.GdmError):
        log_to_notes([np.zeros(3, dtype=[("value", "f8")])], [[0]], [[60]])


def test_process_adjsim_log_reads_the_text_log_and_writes_output_mid(tmp_path, monkeypatch):
    """Reference entry point: ./logs/simulation.log in, ./adj_sim_outputs/midi/output.mid out, its path returned; the file
    holds the four header messages and the recorded note_on / note_off rows with their delta times."""
    from gan_des_midi_music_gen_amd import datasets
    from gan_des_midi_music_gen_amd.sim_log_process_music import process_adjsim_log
    from gan_des_midi_music_gen_amd.sim_log_to_midi import track_bytes
    name = "values"                              # holds unmatched lines: an exponent, a sign, 'processing'
    rec = case_log(name)
    monkeypatch.chdir(tmp_path)
    os.makedirs("logs")
    with open("logs/simulation.log", "w") as f:
        for i in range(len(rec["value"])):
            f.write(f"INFO:root:{float(rec['value'][i])!r} - {int(rec['event_id'][i])} - {int(rec['node'][i])} - "
                    f"{('arrival', 'departure', 'processing')[rec['kind'][i]]}\n")
    args = dict(instruments=[int(x) for x in GOLD[f"{name}/instruments"]],
                note_levels=[int(x) for x in GOLD[f"{name}/note_levels"]])
    path = process_adjsim_log(**args)
    assert path == "./adj_sim_outputs/midi/output.mid"
    rows = [tuple(int(x) for x in r) for r in GOLD[f"{name}/rows"]]
    want = track_bytes(N.track_of(rows))
    assert open(path, "rb").read() == want
    other = process_adjsim_log(log=events(rec), midi_path=str(tmp_path / "other.mid"), **args)
    assert open(other, "rb").read() == want
    md = datasets.read_midi(path)
    on = md.kind == datasets._K_ON
    assert on.sum() == len(rows) // 2 == 3 and md.b[on].tolist() == [r[2] for r in rows[::2]]


# ---- the synth ---------------------------------------------------------------------------------------------------------
CLIPS = {
    "one_note": [(10, 40, 69, 100)],                                            # 11 867 samples: hop 55, frames overlap
    "stack_64": [(5, 5, 48 + k % 25, 60 + k) for k in range(64)],               # zero length, one tick, one release
    "chords": [(0, 20, 60, 127), (0, 40, 64, 120), (10, 40, 67, 110), (20, 40, 72, 126)],
    "sparse": [(100, 220, 45, 80), (3000, 3100, 81, 110), (5000, 5100, 33, 64)],    # 476 754 samples: hop 2217
    "far": [(10, 50, 60, 100), (24000000, 24000100, 72, 90)],                   # second note beyond sample 2^31
    "blank": [],
}
SHORT = ("one_note", "stack_64", "chords")


def clip(name):
    """-> (notes (n, 4) int64, clip_len, mirror frames), computed once."""
    if name not in _cache:
        notes = np.asarray(CLIPS[name], dtype=np.int64).reshape(-1, 4)
        length = N.tick_to_sample(notes[-1, 1]) + N.RELEASE if len(notes) else 0
        _cache[name] = (notes, length, N.frames(notes, length))
    return _cache[name]


def on_device(names, cap):
    notes = np.zeros((len(names), cap, 4), dtype=np.int64)
    for i, n in enumerate(names):
        notes[i, :len(clip(n)[0])] = clip(n)[0]
    up = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(DEV)        # noqa: E731
    return up(notes, np.int64), up([len(clip(n)[0]) for n in names], np.int32), up([clip(n)[1] for n in names], np.int64)


def guarded(n, dtype):
    """A buffer of n elements with 64 guard elements on both sides -> (whole buffer, the inner view, guard value)."""
    canary = -12345
    buf = torch.full((n + 128,), canary, dtype=dtype, device=DEV)
    return buf, buf[64:64 + n], canary


def guards_intact(buf, canary):
    return bool((buf[:64] == canary).all()) and bool((buf[-64:] == canary).all())


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.int32),
                          np.ascontiguousarray(want, dtype=np.float32).view(np.int32))


def test_clips_are_what_they_are_named_for():
    assert clip("one_note")[1] // 215 < 2048 < clip("sparse")[1] // 215
    assert N.tick_to_sample(clip("far")[0][1, 0]) > 1 << 31 and clip("blank")[1] == 0
    s_on = {N.tick_to_sample(t) for t in clip("stack_64")[0][:, 0]}
    assert len(s_on) == 1 and len(clip("stack_64")[0]) == 64
    for name in CLIPS:
        assert clip(name)[2].any() == (name != "blank")
    idx = N.frame_positions(clip("one_note")[1])
    raw = np.arange(216)[:, None] * (clip("one_note")[1] // 215) + np.arange(2048)[None, :] - 1024
    assert (raw < 0).any() and (raw >= clip("one_note")[1]).any() and idx.max() == clip("one_note")[1] - 1


@pytest.mark.parametrize("names,cap", [(("one_note",), 1), (("stack_64",), 64), (("sparse",), 5000), (("far",), 7),
                                       (("chords", "blank", "one_note"), 16)])
def test_stage_b_equals_mirror(names, cap):
    from gan_des_midi_music_gen_amd import ops
    notes, n_notes, clip_len = on_device(names, cap)
    buf, out, canary = guarded(len(names) * 216 * 2048, torch.float32)
    got = ops.synth_frames(notes, n_notes, clip_len, out=out.view(len(names) * 216, 2048))
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy().reshape(len(names), 216, 2048)
    assert guards_intact(buf, canary)
    for i, name in enumerate(names):
        assert same_bits(got[i], clip(name)[2]), name
    fresh = ops.synth_frames(notes, n_notes, clip_len)                          # the allocating form, same bits
    assert same_bits(fresh.cpu().numpy().reshape(got.shape), got)


def test_n_notes_is_clamped_to_the_list_and_tables_are_arguments():
    from gan_des_midi_music_gen_amd import ops
    notes, n_notes, clip_len = on_device(("chords",), 4)
    want = ops.synth_frames(notes, n_notes, clip_len)
    over = torch.tensor([1 << 20], dtype=torch.int32, device=DEV)               # more notes than the list holds
    assert torch.equal(ops.synth_frames(notes, over, clip_len), want)
    under = torch.tensor([-3], dtype=torch.int32, device=DEV)
    assert not ops.synth_frames(notes, under, clip_len).any()
    wave, inc = ops.synth_tables(DEV)
    w, i = N.tables()
    assert np.array_equal(wave.cpu().numpy(), w) and np.array_equal(inc.cpu().numpy().view(np.uint32), i)
    square = torch.where(wave >= 0, 12000, -12000).to(torch.int16)              # another wave table: another mirror
    got = ops.synth_frames(notes, n_notes, clip_len, tables=(square, inc)).cpu().numpy()
    sq = np.where(w >= 0, 12000, -12000).astype(np.int16)
    assert same_bits(got, N.frames(clip("chords")[0], clip("chords")[1], sq, i))
    with pytest.raises(ops.GdmError):
        ops.synth_frames(torch.zeros((1, 5001, 4), dtype=torch.int64, device=DEV), n_notes, clip_len)
    with pytest.raises(ops.GdmError):
        ops.synth_frames(notes.cpu(), n_notes.cpu(), clip_len.cpu())


@pytest.mark.parametrize("name", SHORT)
def test_stage_c_equals_mirror_and_stage_b_through_the_pcm_front_end(name):
    """PCM rendered by gdm_synth_pcm, framed by the existing gdm_pcm_stft_frames, equals gdm_synth_frames: the two
    kernels evaluate the same per-sample function, and the frame kernel's reflection is the front end's."""
    from gan_des_midi_music_gen_amd import ops
    notes, n_notes, clip_len = on_device((name,), 64)
    length = clip(name)[1]
    buf, out, canary = guarded(length, torch.int16)
    pcm = ops.synth_pcm(notes, n_notes, 0, length, out=out)
    assert guards_intact(buf, canary) and np.array_equal(pcm.cpu().numpy(), N.pcm(clip(name)[0], 0, length))
    hop = length // 215
    frames, n_frames = ops.pcm_stft_frames(pcm.clone().view(torch.uint8), ops.PCM_S16, 1, 0, length, 0, 0, 1, -1, length,
                                           hop, 2048)
    assert n_frames >= 216
    direct = ops.synth_frames(notes, n_notes, clip_len)
    assert torch.equal(frames[:216].view(torch.int32), direct.view(torch.int32)) and bool(direct.any())
    # a range that starts inside the clip, ends beyond it and is no multiple of the 8 samples a thread stores
    buf, out, canary = guarded(3001, torch.int16)
    part = ops.synth_pcm(notes, n_notes, length - 2000, 3001, out=out).cpu().numpy()
    assert guards_intact(buf, canary) and np.array_equal(part, N.pcm(clip(name)[0], length - 2000, 3001))
    assert part[:1990].any() and not part[2000:].any()


def test_synth_pcm_beyond_sample_2_31():
    from gan_des_midi_music_gen_amd import ops
    notes, n_notes, _ = on_device(("far",), 2)
    first = N.tick_to_sample(24000000) - 100
    got = ops.synth_pcm(notes, n_notes, first, 4096).cpu().numpy()
    assert first > 1 << 31 and got.any() and np.array_equal(got, N.pcm(clip("far")[0], first, 4096))


# ---- end to end --------------------------------------------------------------------------------------------------------
def _wav_fixture():
    d = np.load(os.path.join(HERE, "golden", "des_prologue_rng.npz"))
    return torch.from_numpy(d["wav/matrices"][:3]).to(DEV), int(d["wav/np_seed"])


def test_matrix_to_wav_des_equals_the_hand_run_chain():
    """Built-in back end == the injected-callable route (whose interleaving tests/test_des_prologue_gpu.py pins to the
    reference's recording) with run_spec, the mirror's notes and the mirror's frames behind it, then the same mel chain:
    same bits, same final position of numpy's global stream."""
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp, simulation_v3, util
    m, seed = _wav_fixture()
    hand = []

    def simulate(spec, index):
        log, _ = simulation_v3.run_spec(spec)
        notes, length, status = N.log_to_notes({k: log[k] for k in log.dtype.names}, spec.note_levels)
        assert status == N.OK
        hand.append(N.frames(notes, length))
        return torch.zeros(128, 216)

    np.random.seed(seed)
    msp.matrix_to_wav(m, size=20, start=0, end=216, simulate=simulate)
    state_want = np.random.get_state()
    frames = torch.from_numpy(np.concatenate(hand)).to(DEV)
    want = util._db_from_frames(frames, 3, 216, 44100, 2048, 128, 20, 8300, 80)
    np.random.seed(seed)
    got = msp.matrix_to_wav(m, size=20, start=0, end=216, device=DEV, simulate="des")
    state_got = np.random.get_state()
    assert state_got[2] == state_want[2] and np.array_equal(state_got[1], state_want[1])
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (3, 128, 216)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert sum(bool(h.any()) for h in hand) >= 2 and float(got.max()) > -60.0          # audible clips, not blanks
    np.random.seed(seed)
    cut = msp.matrix_to_wav(m, size=20, start=20, end=194, device="cpu", simulate="des")   # the reference's slice
    assert not cut.is_cuda and torch.equal(cut, got[:, :, 20:194].cpu())
    with pytest.raises(msp.ops.GdmError):
        msp.matrix_to_wav(m, size=20, simulate="fluidsynth")
    with pytest.raises(msp.ops.GdmError):
        msp.matrix_to_wav(m, size=20)                                                      # the default is unchanged


def test_blank_clip_is_minus_100_db_and_a_loud_clip_agrees_with_the_oracle():
    from gan_des_midi_music_gen_amd import ops, util
    from oracle import mel as omel
    names = ("chords", "blank", "one_note")
    notes, n_notes, clip_len = on_device(names, 16)
    db = util._db_from_frames(ops.synth_frames(notes, n_notes, clip_len), 3, 216, 44100, 2048, 128, 20, 8300, 80)
    db = db.cpu().numpy()
    assert np.abs(db[1] + 100.0).max() < 1e-4                                   # the reference's "blank wav"
    for i in (0, 2):
        length = clip(names[i])[1]
        assert length <= 216 * (length // 215)                                  # the featuriser's crop keeps all of it
        wav = N.pcm(clip(names[i])[0], 0, length).astype(np.float32) * np.float32(2.0 ** -15)
        want = omel.get_melspectrogram_db_tensor(wav)
        assert want.shape == (128, 216) and want.max() > -40.0
        loud = want > want.max() - 60
        assert np.abs(db[i] - want)[loud].max() < 0.02, names[i]


# ---- training and generate_song ----------------------------------------------------------------------------------------
def test_train_with_the_built_in_bridge(monkeypatch):
    from gan_des_midi_music_gen_amd import SIMNN, matrix_sim_process as msp, synthetic
    from gan_des_midi_music_gen_amd.train import SimnnTrainer
    fakes, original = [], msp.matrix_to_wav

    def recording(*a, **k):
        assert k["simulate"] == "des" and (k["start"], k["end"]) == (0, 216)
        out = original(*a, **k)                  # a prologue quirk (two thresholded sources, an empty row) would raise
        fakes.append(out.clone())
        return out

    monkeypatch.setattr(msp, "matrix_to_wav", recording)
    np.random.seed(4)
    _g, _d, g_loss, d_loss = SIMNN.train(fake_provider="des", batch_size=3, max_steps=2, seed=11, save=False,
                                         log=lambda *_a: None, device=DEV)
    assert len(fakes) == 2 and all(f.shape == (3, 128, 216) and f.is_cuda for f in fakes)
    assert len(g_loss) == len(d_loss) == 2 and np.isfinite(g_loss).all() and np.isfinite(d_loss).all()
    assert all(float(f.max()) > -99.0 for f in fakes)                           # real clips, not blanks
    # the same two iterations with the recorded fakes handed over as tensors
    torch.manual_seed(11)
    gen, disc = SIMNN.Generator().to(DEV), SIMNN.Discriminator(input_hw=(128, 216)).to(DEV)
    gen, disc = gen.apply(SIMNN.weights_init), disc.apply(SIMNN.weights_init)
    trainer = SimnnTrainer(gen, disc, lr=0.00002, betas=(0.5, 0.999))
    for step in range(2):
        real = synthetic.spectrogram_batch(3, (128, 216), seed=1234 + step).to(DEV)
        noise = SIMNN.get_noise(3, 100, device=DEV)
        dl, gl = trainer.step(real, noise, fakes[step])
        assert dl.item() == d_loss[step] and gl.item() == g_loss[step], step
    with pytest.raises(ValueError):
        SIMNN.train(fake_provider="des", input_hw=(128, 256), max_steps=1, save=False, device=DEV)
    with pytest.raises(ValueError):
        SIMNN.train(fake_provider="fluidsynth", max_steps=1, save=False, device=DEV)


def test_generate_song_writes_midi_and_wav(tmp_path):
    from gan_des_midi_music_gen_amd import SIMNN, datasets, util
    torch.manual_seed(21)
    path = str(tmp_path / "gen_5_0.pt")
    torch.save(SIMNN.Generator().apply(SIMNN.weights_init).state_dict(), path)
    mid, wav = str(tmp_path / "out" / "song.mid"), str(tmp_path / "out" / "song.wav")
    np.random.seed(8)
    spec = SIMNN.generate_song(path, device=DEV, bridge="des", midi_path=mid, wav_path=wav, max_seconds=3)
    assert spec.shape == (128, 216) and spec.is_cuda and bool(torch.isfinite(spec).all()) and float(spec.max()) > -99.0
    md = datasets.read_midi(mid)
    on, off = md.kind == datasets._K_ON, md.kind == datasets._K_OFF
    assert md.ticks_per_beat == 480 and on.sum() == off.sum() > 10 and (md.kind == datasets._K_TEMPO).sum() == 1
    notes = np.stack([md.tick[on], md.tick[off], md.a[on], md.b[on]], axis=1).astype(np.int64)
    assert np.array_equal(md.a[on], md.a[off]) and (notes[:, 0] <= notes[:, 1]).all()
    data = util.load_wav(wav)
    assert (data.fmt, data.channels, data.sample_rate) == (util.ops.PCM_S16, 1, 44100)
    want_len = min(3 * 44100, N.tick_to_sample(notes[-1, 1]) + N.RELEASE)
    assert data.n_frames == want_len
    assert open(wav, "rb").read() == N.wav_bytes(N.pcm(notes, 0, want_len))
    # the returned spectrogram is the whole clip's: the mirror's frames through the same mel chain
    length = N.tick_to_sample(notes[-1, 1]) + N.RELEASE
    frames = torch.from_numpy(N.frames(notes, length)).to(DEV)
    want = util._db_from_frames(frames, 1, 216, 44100, 2048, 128, 20, 8300, 80)[0]
    assert torch.equal(spec.view(torch.int32), want.view(torch.int32))
    adj = SIMNN.generate_song(path, device=DEV)                                 # the default is unchanged
    assert adj.shape == (20, 20)
