"""CPU: the DES log -> MIDI -> piano-roll restatement (tests/des_midi_ref.py) against tracks recorded from the
reference's own MidiGenerator (tests/golden/des_midi.npz, recorder: tests/golden/make_des_midi_golden.py), and the
Standard MIDI File writer against both of the project's readers and the reference's own generation.mid."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import des_midi_ref as R  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "des_midi.npz"))
CORE = np.load(os.path.join(HERE, "golden", "des_core.npz"))
NAMES = [str(n) for n in GOLD["names"]]


def case_log(name):
    """The records the recorder wrote to the reference's log file for this case (see its ``transformed``)."""
    log, n, tr = str(GOLD[f"{name}/log"]), int(GOLD[f"{name}/n_lines"]), int(GOLD[f"{name}/transform"])
    rec = {k: CORE[f"{log}/{k}"] for k in ("value", "event_id", "node", "kind")}
    if tr in (1, 2):
        keep = rec["kind"] == 0
        rec = {k: v[keep] for k, v in rec.items()}
        rec["node"] = (rec["event_id"] % 2).astype(np.int32)
    if tr == 2:                                   # one node: `fill` arrivals, then departure / arrival in turn
        rec["node"] = np.zeros_like(rec["node"])
        rec["kind"] = rec["kind"].copy()
        rec["kind"][int(GOLD[f"{name}/fill"])::2] = 1
    if n >= 0:
        rec = {k: v[:n] for k, v in rec.items()}
    return rec


def rows(track):
    return np.asarray(track, dtype=np.int32).reshape(-1, 4)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_recorded_tracks(name):
    rec = case_log(name)
    before = R.build_track(rec, GOLD[f"{name}/tail"], GOLD[f"{name}/instruments"], GOLD[f"{name}/note_levels"])
    assert np.array_equal(rows(before), GOLD[f"{name}/before"])
    saved = bool(GOLD[f"{name}/generate"]) or R.lines_read(len(rec["value"])) % 100 == 0
    assert saved == bool(GOLD[f"{name}/saved"])
    if saved:
        assert np.array_equal(rows(R.save_track(before)), GOLD[f"{name}/after"])


def test_golden_cases_reach_the_branches():
    """The fixture is only worth something if the cases hit what they are named for."""
    p = {n: R.parameters(GOLD[f"{n}/tail"]) for n in NAMES}
    low = p["midi0_low_base_var0_tempo0"]
    assert low["base"] == 80 and low["var"] == 30 and low["tempo"] == 500000
    assert int(GOLD["midi0_low_base_var0_tempo0/tail"][3] * np.float32(90)) < 50
    assert p["midi1_tempo_capped"]["tempo"] == 16777215
    assert len(case_log("midi0_3000_lines_simulation")["value"]) == 3000 and bool(GOLD["midi0_3000_lines_simulation/saved"])
    assert not bool(GOLD["midi0_1234_lines_not_saved/saved"]) and not bool(GOLD["midi1_all_lines_not_saved/saved"])
    assert len(np.unique(GOLD["midi0_one_instrument/instruments"])) == 1
    assert len(np.unique(GOLD["midi0_rand0/instruments"])) > 1
    for n in ("midi0_queues_fill", "midi1_queues_fill"):        # two nodes, arrivals only: counts pass 127
        ons = GOLD[f"{n}/before"]
        assert (ons[:, 0] == R.NOTE_ON).sum() > 2 * 127
    # queue-count folding: the count only shows as the service time in a departure's note_off time, so the cases that
    # pin it carry departures after the fill, and the recorded note_off times differ from what either branch, switched
    # off in the restatement, would give
    for log in ("midi0", "midi1"):
        for n, branch, other in ((f"{log}_queue_fold_127", 0, "fold_254"), (f"{log}_queue_fold_254", 1, "fold_127")):
            args = (case_log(n), GOLD[f"{n}/tail"], GOLD[f"{n}/instruments"], GOLD[f"{n}/note_levels"])
            gold, seen = GOLD[f"{n}/before"], {}
            assert np.array_equal(rows(R.build_track(*args, seen=seen)), gold)
            assert seen["fold_127"] > 0 and (branch == 0) == (other not in seen), seen
            off = gold[:, 0] == R.NOTE_OFF
            assert off.sum() > 10
            unfolded = rows(R.build_track(*args, fold=(branch != 0, branch != 1)))
            assert unfolded.shape != gold.shape or (unfolded[off][:, 3] != gold[off][:, 3]).any(), n
            assert not np.array_equal(unfolded, gold)
    assert any((GOLD[f"{n}/before"][:, 3] > 200).any() for n in NAMES), "save_midi's removal loop is exercised"
    assert any(len(GOLD[f"{n}/before"]) == 501 for n in NAMES), "an arrival may append two messages at 499"


def test_regex_predicate_on_every_golden_record():
    """line_matches decides numerically what the reference decides with re.match on the line's text."""
    from gan_des_midi_music_gen_amd.sim_log_to_midi import LOG_REGEX
    rx = re.compile(LOG_REGEX)
    names = ("arrival", "departure", "processing")
    total = unmatched_ad = 0
    for log in ("midi0", "midi1", "wav0", "wav1", "hand"):
        v, e, nd, kd = (CORE[f"{log}/{k}"] for k in ("value", "event_id", "node", "kind"))
        for i in range(len(v)):
            text = f"INFO:root:{float(v[i])!r} - {int(e[i])} - {int(nd[i])} - {names[kd[i]]}\n"
            want = rx.match(text) is not None
            assert R.line_matches(v[i], int(e[i]), int(nd[i]), int(kd[i])) == want, text
            total += 1
            unmatched_ad += (not want) and kd[i] != 2
    assert total > 80000 and unmatched_ad > 0
    # hand-made values around the edges of repr's plain-digit range
    for val in (0.0, -0.0, 1e-4, 9.999999999999999e-05, 1e16, 9999999999999998.0, float("inf"), float("nan"), -1.5, 5e-324):
        text = f"INFO:root:{val!r} - 3 - 4 - arrival\n"
        assert R.line_matches(val, 3, 4, 0) == (rx.match(text) is not None), text


def test_planes_restatement_equals_oracle_on_written_file(tmp_path):
    """track -> planes of the restatement == oracle.piano_roll.generate_piano_roll on the file write_midi writes (the
    oracle is the project's existing, stated-unpinned statement of mido's iteration)."""
    from gan_des_midi_music_gen_amd.sim_log_to_midi import write_midi
    from oracle import piano_roll as opr
    for name in NAMES:
        if not bool(GOLD[f"{name}/saved"]):
            continue
        path = write_midi(GOLD[f"{name}/after"], str(tmp_path / f"{name}.mid"))
        for (start, end) in ((0, 50), (100, 150), (0, 30)):
            want = opr.generate_piano_roll(path, start=start, end=end)
            got = R.track_to_planes([tuple(m) for m in GOLD[f"{name}/after"].tolist()], start, end)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, start, end)
            assert want[0].shape == (128, end - start)
    assert any(R.track_to_planes([tuple(m) for m in GOLD[f"{n}/after"].tolist()], 0, 50)[0].any() for n in NAMES)


def test_writer_round_trips_through_both_readers(tmp_path):
    from gan_des_midi_music_gen_amd import datasets
    from gan_des_midi_music_gen_amd.sim_log_to_midi import write_midi
    from oracle import midi_events as me
    names = {R.SET_TEMPO: "set_tempo", R.TIME_SIGNATURE: "time_signature", R.NOTE_ON: "note_on", R.NOTE_OFF: "note_off",
             R.END_OF_TRACK: "end_of_track"}
    kinds = {R.SET_TEMPO: datasets._K_TEMPO, R.TIME_SIGNATURE: datasets._K_TSIG, R.NOTE_ON: datasets._K_ON,
             R.NOTE_OFF: datasets._K_OFF, R.END_OF_TRACK: datasets._K_EOT}
    for name in NAMES:
        track = GOLD[f"{name}/after"] if bool(GOLD[f"{name}/saved"]) else GOLD[f"{name}/before"]
        path = write_midi(track, str(tmp_path / f"{name}.mid"))
        expect = [tuple(m) for m in track.tolist()]
        if expect[-1][0] != R.END_OF_TRACK:
            expect.append((R.END_OF_TRACK, 0, 0, 0))            # the writer closes the track, as mido's save does
        fmt, tpb, tracks = me.load(path)
        assert (fmt, tpb, len(tracks)) == (1, 480, 1) and len(tracks[0]) == len(expect)
        for (d, kind, a, b), (k, ea, eb, t) in zip(tracks[0], expect):
            assert d == t
            if k in names:
                assert (kind, a, b) == (names[k], ea, eb)
            else:                                               # key_signature: 'other' to this reader
                assert kind == "other" and (k == R.KEY_SIGNATURE or a == ea)
        md = datasets.read_midi(path)
        assert (md.format, md.ticks_per_beat) == (1, 480) and len(md.tick) == len(expect)
        assert np.array_equal(md.tick, np.cumsum([m[3] for m in expect]))
        for i, (k, ea, eb, _t) in enumerate(expect):
            if k in kinds:
                assert (md.kind[i], md.a[i], md.b[i]) == (kinds[k], ea, eb)
            else:
                assert md.kind[i] == datasets._K_OTHER
                if k == R.PROGRAM_CHANGE:
                    assert md.a[i] == ea


def test_header_bytes_equal_the_references_own_file():
    """tests/golden/midi/generation.mid was written by the reference through mido.  What is recoverable from it: the
    tempo (set_tempo body) and the key (sharps / minor bytes 06 00 = 'F#', index 5).  Compared: the MThd chunk, and
    the track bytes from the first delta up to (not including) the first note message -- set_tempo, time_signature,
    key_signature, program_change 0 -- i.e. file bytes [0:14] and [22:46]; the MTrk length differs with the notes."""
    from gan_des_midi_music_gen_amd.sim_log_to_midi import track_bytes
    ref = open(os.path.join(HERE, "golden", "midi", "generation.mid"), "rb").read()
    assert ref[22:26] == b"\x00\xff\x51\x03" and ref[37:43] == b"\x00\xff\x59\x02\x06\x00"
    tempo = int.from_bytes(ref[26:29], "big")
    ours = track_bytes(R.header({"tempo": tempo, "key": R.KEYS.index("F#")}))
    assert ours[:14] == ref[:14] and ours[14:18] == b"MTrk"
    assert ours[22:46] == ref[22:46]
    assert ref[47] == 0x90, "the reference's file goes on with a delta and a note_on there"


def test_argument_checks_without_a_device():
    import torch
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, sim_log_to_midi as S
    log = np.zeros(3, dtype=S.EVENT_DTYPE)
    with pytest.raises(ops.GdmError):
        S.log_to_rolls([log], np.zeros((1, 10), np.float32), [[0] * 4], [[60] * 4], device="cpu")
    with pytest.raises(ops.GdmError):
        S.log_to_rolls([], np.zeros((0, 10), np.float32), [], [])
    with pytest.raises(ops.GdmError):
        z = torch.zeros(4)
        ops.des_log_to_roll(z.double(), z.long(), z.int(), z.int(), torch.zeros(2, dtype=torch.int64),
                            torch.zeros(1, 10), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32),
                            torch.zeros(1, dtype=torch.int32), 0, 50)
    with pytest.raises(ops.GdmError):
        msp.matrix_to_midi(torch.zeros(1, 1, 8, 8), torch.zeros(1, 20), adj_size=(8, 8), simulate="nope")
    with pytest.raises(ops.GdmError):                             # simulate=None keeps raising
        msp.matrix_to_midi(torch.zeros(1, 1, 8, 8), torch.zeros(1, 20), adj_size=(8, 8))
    assert ops.des_roll_width(0, 50) == 50 and ops.des_roll_width(100, 150) == 50 and ops.des_roll_width(30, 80) == 20
