"""Batched generation against the one-sample entry points it batches.

  sample      MultiModalGAN.sample (one gdm_mmgan_gen_eval launch) against the eval-mode module forwards of both
              generators in bf16 (8 block launches + 2 cats up to 256 rows, GEMM + batch-norm launches above), at the
              checkpoint geometry, B = 1 / 16 / 256 / 4096: device time between HIP events around one call, the
              kernel alone, and wall time per call ending in a synchronise
  midis       generate_midis(256) end to end against 256 calls of generate_midi with one sample, and the former taken
              apart: generators, scan, host draws + routing, simulator, log -> roll + read-back, file writing
  songs       generate_songs(30) against 30 calls of generate_song(bridge="des_batch"), --max-seconds of audio each

Routes are alternated --rounds times in one process after a warm-up; medians are printed, one JSON line per item.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_des_midi_music_gen_amd import SIMNN, ops  # noqa: E402
from gan_des_midi_music_gen_amd import matrix_sim_process as msp  # noqa: E402
from gan_des_midi_music_gen_amd import network_tests as NT  # noqa: E402
from gan_des_midi_music_gen_amd import sim_log_to_midi  # noqa: E402

DEV = torch.device("cuda")


def wall(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def model2(midi_path=None):
    torch.manual_seed(3)
    mm = NT.MultiModalGAN(z_dim=50, adj_size=(64, 64), roll_size=(2, 128, 50), input_dim=50, output_dim=20, instrument=0,
                          start=100, end=150, device=DEV, fake_provider="des_batch", midi_path=midi_path).to(DEV)
    g = torch.Generator().manual_seed(4)
    for gen in (mm.generator1, mm.generator2):
        gen.compute_dtype = "bf16"
        for blk in gen.gen:
            blk[1].running_mean.copy_(torch.randn(blk[1].num_features, generator=g) * 0.1)
            blk[1].running_var.copy_(torch.rand(blk[1].num_features, generator=g) + 0.5)
    return mm.eval()


def bench_sample(rounds, emit):
    mm = model2()
    for B in (1, 16, 256, 4096):
        g = torch.Generator().manual_seed(B)
        n1, n2, gi = (torch.randn(B, 50, generator=g).to(DEV) for _ in range(3))
        beats = torch.cumsum(torch.rand(B, 50, generator=g) * 0.5 + 0.3, dim=1).to(DEV)

        def new():
            return mm.sample(noise1=n1, noise2=n2, input_tensor=beats, gen1_input=gi)

        def old():
            with torch.no_grad():
                return mm.generator1(n1, gi), mm.generator2(n2, beats)

        reps = 200 if B <= 256 else 50
        for fn in (new, old):
            wall(fn, 20)
        res = {"new_wall": [], "old_wall": [], "new_dev": [], "old_dev": [], "new_kernel": []}
        for _ in range(rounds):
            res["old_wall"].append(wall(old, reps))
            res["new_wall"].append(wall(new, reps))
            res["old_dev"].append(device_ms(old, reps))
            res["new_dev"].append(device_ms(new, reps))
            ops.time_entry_point("gdm_mmgan_gen_eval")
            for _ in range(reps):
                new()
            torch.cuda.synchronize()
            res["new_kernel"].append(ops.timed_durations_ms()[0])
            ops.time_entry_point(None)
        emit(dict(item="sample", B=B, **{k + "_us": round(statistics.median(v) * 1e3, 2) for k, v in res.items()}))


def midis_split(mm, n1, n2, beats, out_dir):
    """generate_midis(bridge="des_batch") stage by stage, a synchronise after each: ms per stage."""
    t = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        t[name] = (time.perf_counter() - t0) * 1e3
        return time.perf_counter()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o1, o2 = mm.sample(noise1=n1, noise2=n2, input_tensor=beats)
    t0 = lap("generators", t0)
    h = msp.MIDI.scan(o1, 64, o2)
    t0 = lap("scan", t0)
    pro = msp.MIDI.batched(h, 0)
    t0 = lap("host_draws_and_routing", t0)
    log = pro.simulate_on(DEV, max_records=sim_log_to_midi.MAX_LINES + 1)
    t0 = lap("simulator", t0)
    good = (log.stop_reason != ops.DES_STOP_ERROR) & (log.stop_reason != ops.DES_STOP_BUDGET)
    tails = torch.from_numpy(np.ascontiguousarray(h["g2"][:, 10:])).to(DEV)
    _planes, track, track_len, _status = ops.des_log_to_roll(
        log.value, log.event_id, log.node, log.kind, log.rec_ptr, tails, torch.from_numpy(pro.instruments).to(DEV),
        torch.from_numpy(pro.note_levels).to(DEV), good.to(torch.int32), 100, 150)
    track, track_len = track.cpu().numpy(), track_len.cpu().numpy()
    t0 = lap("log_to_roll_and_readback", t0)
    for i in range(len(track)):
        sim_log_to_midi.write_midi(track[i, :track_len[i]], os.path.join(out_dir, f"split_{i:04d}.mid"))
    lap("file_writing", t0)
    return t


def bench_midis(rounds, emit, n=256):
    with tempfile.TemporaryDirectory() as tmp:
        mm = model2(midi_path=os.path.join(tmp, "generation.mid"))
        g = torch.Generator().manual_seed(7)
        n1, n2 = (torch.randn(n, 50, generator=g).to(DEV) for _ in range(2))
        beats = torch.cumsum(torch.rand(n, 50, generator=g) * 0.5 + 0.3, dim=1).to(DEV)

        def new():
            np.random.seed(1)
            return mm.generate_midis(noise1=n1, noise2=n2, input_tensor=beats, out_dir=os.path.join(tmp, "new"))

        def old():
            np.random.seed(1)
            for i in range(n):
                mm.generate_midi(n1[i:i + 1], n2[i:i + 1], beats[i:i + 1])

        new()
        mm.generate_midi(n1[:1], n2[:1], beats[:1])
        res = {"new": [], "old": []}
        splits = []
        for _ in range(rounds):
            res["old"].append(wall(old, 1))
            res["new"].append(wall(new, 1))
            np.random.seed(1)
            splits.append(midis_split(mm, n1, n2, beats, tmp))
        ok = int(new().ok.sum())
        emit(dict(item="generate_midis", n=n, ok=ok, new_ms=round(statistics.median(res["new"]), 2),
                  old_ms=round(statistics.median(res["old"]), 2),
                  split_ms={k: round(statistics.median(s[k] for s in splits), 2) for k in splits[0]}))


def bench_songs(rounds, emit, max_seconds, n=30):
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(21)
        ck = os.path.join(tmp, "gen_5_0.pt")
        torch.save(SIMNN.Generator().apply(SIMNN.weights_init).state_dict(), ck)

        def new():
            np.random.seed(2)
            return SIMNN.generate_songs(ck, n, out_dir=os.path.join(tmp, "new"), max_seconds=max_seconds, device=DEV)

        def old():
            np.random.seed(2)
            for i in range(n):
                SIMNN.generate_song(ck, device=DEV, bridge="des_batch", compute_dtype="bf16", max_seconds=max_seconds,
                                    midi_path=os.path.join(tmp, "old", f"{i}.mid"),
                                    wav_path=os.path.join(tmp, "old", f"{i}.wav"))

        new()
        old()
        res = {"new": [], "old": []}
        for _ in range(rounds):
            res["old"].append(wall(old, 1))
            res["new"].append(wall(new, 1))
        emit(dict(item="generate_songs", n=n, max_seconds=max_seconds, new_ms=round(statistics.median(res["new"]), 2),
                  old_ms=round(statistics.median(res["old"]), 2)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--items", default="sample,midis,songs")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-seconds", type=float, default=10.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    items = a.items.split(",")
    if "sample" in items:
        bench_sample(a.rounds, emit)
    if "midis" in items:
        bench_midis(a.rounds, emit)
    if "songs" in items:
        bench_songs(a.rounds, emit, a.max_seconds)


if __name__ == "__main__":
    main()
