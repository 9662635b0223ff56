"""Device time of the four synth entry points (csrc/synth.hip) at the geometries DESIGN.md section 7 reports.  On an MI355X:

    python tools/bench_synth.py                         one measurement of the library GDM_LIB_TAG names (default: shipped)
    python tools/bench_synth.py --compare TAG --rounds 5 --out FILE.jsonl
        alternates fresh child processes on libgdm_hip_TAG.so (a build of another commit's csrc/, see tools/README.md)
        and on the shipped library, `rounds` times each, and appends one line per entry point: median, min and max of
        both, and whether the shipped median lies inside the other's min .. max.

  gdm_synth_frames      B = 30 clips of the bridge (f7: the five matrices of des_prologue_rng.npz six times, "des")
  gdm_synth_pcm         the first five seconds of the first of those clips
  gdm_synth_windows     30 five-second windows of a generated ten-minute performance of 20 000 notes (f9)
  gdm_synth_windows_gm  one chunk of sim_to_wav's render: a size-32 matrix under a fixed seed, five seconds (f12)

Each figure is the mean of `calls` launches between two HIP events per launch (``ops.time_entry_point``), after a warm-up.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gdm_synth_frames", "gdm_synth_pcm", "gdm_synth_windows", "gdm_synth_windows_gm")


def measure(calls, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_to_wav as s2w, simulation_v3
    from gan_des_midi_music_gen_amd.sim_log_process_music import MAX_LINES
    dev = torch.device("cuda")
    up = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)   # noqa: E731
    five = 5 * ops.SYNTH_RATE

    # the bridge's clips (tools/bench_des_bridge.py)
    d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
    matrices = torch.from_numpy(np.tile(d["wav/matrices"], (6, 1, 1))[:30]).to(dev)
    np.random.seed(int(d["wav/np_seed"]))
    logs, levels = [], []
    for spec in msp.WAV.specs(msp.WAV.scan(matrices, 20)):
        logs.append(simulation_v3.run_spec(spec)[0][:MAX_LINES])
        levels.append([int(x) for x in spec.note_levels])
    rec = np.concatenate(logs)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in logs])])
    notes, n_notes, clip_len, _status = ops.des_log_to_notes(up(rec["value"]), up(rec["event_id"]), up(rec["node"]),
                                                             up(rec["kind"]), up(ptr, np.int64), up(levels, np.int32))
    frames = torch.empty((30 * ops.SYNTH_FRAMES, ops.SYNTH_NFFT), dtype=torch.float32, device=dev)
    pcm = torch.empty(five, dtype=torch.int16, device=dev)

    # the performance (tools/bench_maestro_dataset.py's note statistics, rows in samples: 960 ticks per second)
    g = np.random.default_rng(0)
    on = np.sort(g.integers(0, 600 * 960 - 2000, 20000))
    rows = np.stack([on * 735 // 16, (on + g.integers(40, 1500, 20000)) * 735 // 16, g.integers(21, 109, 20000),
                     g.integers(20, 120, 20000)], axis=1).astype(np.int64)
    starts = sorted(random.Random(0).sample(range(0, int(rows[:, 1].max()), five), 30))
    perf = (up(rows), up(np.maximum.accumulate(rows[:, 1])), up([0, len(rows)], np.int64), up([0] * 30, np.int32),
            up(starts, np.int64))
    windows = torch.empty((30, five + 4), dtype=torch.int16, device=dev)

    # the demo's clip (simulation_to_wav._render)
    with np.load(os.path.join(ROOT, "tests/golden/sim_to_wav.npz")) as z:
        np.random.seed(int(z["size32/seed"]))
    with tempfile.TemporaryDirectory() as tmp:
        batch = s2w.sim_to_wav([None], size=32, simulate="des", out_dir=tmp, max_seconds=5, return_batch=True)
    count = int(batch.n_notes[0])
    assert count > 0
    mul, div = ops.tick_rule()
    gm = batch.notes[0, :count].clone()
    gm[:, :2] = torch.div(gm[:, :2] * mul, div, rounding_mode="floor")
    release = ops.synth_gm_tables(dev)[1][:, 1].to(torch.int64)
    end_max = torch.cummax(gm[:, 1] + release[(gm[:, 4] & 127) >> 3], dim=0).values.contiguous()
    demo = (gm, end_max, up([0, count], np.int64), up([0], np.int32), up([0], np.int64))
    chunk = torch.empty((1, five + 4), dtype=torch.int16, device=dev)

    runs = {"gdm_synth_frames": lambda: ops.synth_frames(notes, n_notes, clip_len, out=frames),
            "gdm_synth_pcm": lambda: ops.synth_pcm(notes[:1], n_notes[:1], 0, five, out=pcm),
            "gdm_synth_windows": lambda: ops.synth_windows(*perf, five, out=windows),
            "gdm_synth_windows_gm": lambda: ops.synth_windows_gm(*demo, five, out=chunk)}
    res = {"lib": os.environ.get("GDM_LIB_TAG", ""), "calls": calls,
           "notes": {"bridge_mean": float(n_notes.float().mean()), "performance": len(rows), "demo": count}}
    for name in ENTRIES:
        for _ in range(warmup):
            runs[name]()
        torch.cuda.synchronize()
        ops.time_entry_point(name)
        for _ in range(calls):
            runs[name]()
        torch.cuda.synchronize()
        ms, n = ops.timed_durations_ms()
        ops.time_entry_point(None)
        assert n == calls
        res[name + "_us"] = round(ms * 1e3, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", default=None, help="GDM_LIB_TAG of the other library")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare is None:
        print(json.dumps(measure(args.calls, args.warmup)))
        return
    runs = {"other": [], "this": []}
    for _ in range(args.rounds):
        for name, tag in (("other", args.compare), ("this", "")):
            env = dict(os.environ, GDM_LIB_TAG=tag)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=300, env=env)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"measurement of library {tag!r} failed (exit {r.returncode}): nothing more is started")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = []
    for entry in ENTRIES:
        o, t = ([r[entry + "_us"] for r in runs[k]] for k in ("other", "this"))
        lines.append({"entry": entry, "rounds": args.rounds, "calls": args.calls, "other_lib": args.compare,
                      "notes": runs["this"][0]["notes"], "other_us": o, "this_us": t,
                      "other_median_min_max": [statistics.median(o), min(o), max(o)],
                      "this_median_min_max": [statistics.median(t), min(t), max(t)],
                      "this_median_inside_other_range": min(o) <= statistics.median(t) <= max(o)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
