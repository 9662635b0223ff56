"""Timing of model 2's MIDI-folder input.  On an MI355X:

    python tools/bench_maestro_windows.py [OUT.json] [--files F] [--copies C]

F generated two-track files (default 40, ~12 000 messages, 48 KB and ~390 s each, seeded) are parsed once
(``read_midi``, timed on its own: host work both routes share); the parsed list is used C times over (default 32:
1 280 files, 5 windows each at sample_size 300 / L 50 -- MAESTRO's size) so that the device part works on what a user
would run.

1. Building the dataset from the parsed files, two routes alternated, one warm-up and three timed repetitions each,
   medians and ranges; both end in a device synchronise:
     windows   datasets.MaestroWindows.from_midi(parsed): window_plan per file, one upload, ONE gdm_piano_roll_windows
               launch, beats gathered per window
     per_file  the way without it: generate_piano_rolls(parsed, 300, start=0, end=300) (one gdm_piano_roll_raster launch
               on full-width planes), then torch slicing of windows 1..k per file and one torch.stack per tensor.  It is
               HANDED every file's kept windows, planned outside the timed region; ``plan_only`` times that host plan
               (window_plan over the files, which ``windows`` contains) beside the two
   and the device part of each alone, from arrays that are already uploaded (20 repetitions): the one launch against
   the per-file launch + slicing + stack.
2. Per training step at B = 16 and B = 256, alternated, five epochs each: ``batches(B)`` (views) against
   ``DataLoader(dataset, B, drop_last=True)`` over the same device items (one torch.stack per tensor per step), per-step
   medians over the epochs; beside them the measured time of ``MmganTrainer.step`` at that B on such a batch.
Figures are printed as JSON (and written to OUT.json); nothing is asserted except that the two routes return the same
bits."""
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import datasets, network_tests as NT, ops, synthetic
from gan_des_midi_music_gen_amd.train import MmganTrainer

argv = sys.argv[1:]
n_files = int(argv[argv.index("--files") + 1]) if "--files" in argv else 40
copies = int(argv[argv.index("--copies") + 1]) if "--copies" in argv else 32
out_path = argv[0] if argv and not argv[0].startswith("--") else None
SAMPLE, L, BEATS = 300, 50, 50


def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def make_file(seed, notes=6000):
    """A MAESTRO-like performance: tempo track + one note track, ~15 notes a second for ~400 s, 480 ticks per beat."""
    g = np.random.default_rng(seed)
    pending = []                                                # (absolute tick, raw bytes)
    now = 0
    for _ in range(notes):
        now += int(g.integers(5, 120))
        note, vel, held = int(g.integers(21, 109)), int(g.integers(1, 128)), int(g.integers(30, 2000))
        pending.append((now, bytes([0x90, note, vel])))
        pending.append((now + held, bytes([0x80, note, 64])))
    pending.sort(key=lambda m: m[0])
    last, body = 0, b""
    for tick, raw in pending:
        body += vlq(tick - last) + raw
        last = tick
    body += vlq(1) + b"\xff\x2f\x00"
    meta = vlq(0) + b"\xff\x51\x03" + (500000).to_bytes(3, "big") + vlq(0) + b"\xff\x58\x04\x04\x02\x18\x08" + \
        vlq(1) + b"\xff\x2f\x00"
    chunks = b"".join(b"MTrk" + len(t).to_bytes(4, "big") + t for t in (meta, body))
    return b"MThd" + (6).to_bytes(4, "big") + (1).to_bytes(2, "big") + (2).to_bytes(2, "big") + (480).to_bytes(2, "big") + chunks


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


raw = [make_file(s) for s in range(n_files)]
t0 = time.perf_counter()
parsed = [datasets.read_midi(b) for b in raw]
parse_ms = (time.perf_counter() - t0) * 1e3
files = parsed * copies
plans = [datasets.window_plan(md, SAMPLE, L) for md in parsed] * copies
kept = [p[1] for p in plans]


def windows():
    return datasets.MaestroWindows.from_midi(files, SAMPLE, L, BEATS)


def per_file():
    roll, dur, beats = datasets.generate_piano_rolls(files, SAMPLE, BEATS, 0, SAMPLE)
    rs, ds_, bs = [], [], []
    for f, ks in enumerate(kept):
        for i in ks:
            rs.append(roll[f, :, i * L:(i + 1) * L])
            ds_.append(dur[f, :, i * L:(i + 1) * L])
            bs.append(beats[f])
    return torch.stack(rs), torch.stack(ds_), torch.stack(bs)


(a, _), (b, _) = timed(windows), timed(per_file)                # warm-up of both routes
assert torch.equal(a.piano_roll, b[0]) and torch.equal(a.durations, b[1]) and torch.equal(a.beats, b[2])
def plan_only():                                                # host share of `windows` that `per_file` is handed
    return [datasets.window_plan(md, SAMPLE, L) for md in files]


build = {"windows": [], "per_file": [], "plan_only": []}
for rep in range(3):                                            # alternate the routes
    for name, fn in (("windows", windows), ("per_file", per_file), ("plan_only", plan_only)):
        build[name].append(timed(fn)[1])

# the device part alone, from uploaded arrays
ptrs, steps, vels, total = [np.zeros(1, np.int32)], [], [], 0
for _t, _k, (rp, st, ve) in plans:
    ptrs.append(rp[1:] + total); total += int(rp[-1]); steps.append(st); vels.append(ve)
up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
row_ptr, ev_step, ev_vel = up(np.concatenate(ptrs)), up(np.concatenate(steps)), up(np.concatenate(vels))
win_file = up(np.concatenate([np.full(len(k), f, np.int32) for f, k in enumerate(kept)]))
win_s0 = up((np.concatenate(kept) * L).astype(np.int32))
starts = [(f, int(i) * L) for f, ks in enumerate(kept) for i in ks]


def dev_windows():
    return ops.piano_roll_windows(row_ptr, ev_step, ev_vel, win_file, win_s0, L)


def dev_per_file():
    roll, dur = ops.piano_roll_raster(row_ptr, ev_step, ev_vel, len(files), SAMPLE)
    return (torch.stack([roll[f, :, s:s + L] for f, s in starts]), torch.stack([dur[f, :, s:s + L] for f, s in starts]))


timed(dev_windows), timed(dev_per_file)
device = {"windows": [], "per_file": []}
for rep in range(20):
    for name, fn in (("windows", dev_windows), ("per_file", dev_per_file)):
        device[name].append(timed(fn)[1])
ops.time_entry_point("gdm_piano_roll_windows")
for rep in range(20):
    dev_windows()
torch.cuda.synchronize()
kernel_ms, _n = ops.timed_durations_ms()
ops.time_entry_point(None)

# per training step
data = a
loader_res = {}
for bsz in (16, 256):
    torch.manual_seed(0)
    mm = NT.MultiModalGAN(z_dim=50, adj_size=(64, 64), roll_size=(2, 128, L), input_dim=BEATS, output_dim=20,
                          instrument=0, start=100, end=100 + L, device="cuda")
    mm.train()
    tr = MmganTrainer(mm)
    d = synthetic.mmgan_inputs(bsz, L, seed=1, device="cuda")
    views = data.batches(bsz)
    loader = torch.utils.data.DataLoader(data, batch_size=bsz, drop_last=True)
    n_steps = len(views)

    def epoch(it):
        keep = None
        for batch in it:
            keep = batch
        return keep

    def train_steps(k=20):
        it = iter(views)
        for _ in range(k):
            roll, dur, beats = next(it)
            tr.step(roll, dur, beats, d["noise1"], d["noise2"], d["fake_a"], d["fake_b"])

    timed(lambda: epoch(views)), timed(lambda: epoch(loader)), timed(lambda: train_steps(3))
    per = {"views": [], "dataloader": []}
    for rep in range(5):
        for name, it in (("views", views), ("dataloader", loader)):
            per[name].append(timed(lambda: epoch(it))[1] / n_steps)
    step_ms = [timed(train_steps)[1] / 20 for _ in range(3)]
    loader_res[f"B{bsz}"] = {"steps_per_epoch": n_steps, "views_ms_per_step": spread(per["views"]),
                             "dataloader_ms_per_step": spread(per["dataloader"]),
                             "trainer_step_ms": spread(step_ms)}

res = {"files": {"generated": n_files, "copies": copies, "bytes_each": len(raw[0]), "messages_each": len(parsed[0].tick),
                 "windows": len(data), "sample_size": SAMPLE, "sequence_length": L,
                 "dataset_bytes": sum(t.numel() * 4 for t in (data.piano_roll, data.durations, data.beats))},
       "parse_ms_total": parse_ms, "parse_ms_per_file": parse_ms / n_files,
       "build_from_parsed_ms": {k: spread(v) for k, v in build.items()},
       "device_part_ms": {k: spread(v) for k, v in device.items()},
       "gdm_piano_roll_windows_event_ms": kernel_ms,
       "per_step": loader_res}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
