"""Timing of the DES log -> MIDI -> piano-roll bridge.  On an MI355X:

    python tools/bench_des_midi.py [OUT.json]

For B = 16 and B = 256 samples cut from the golden model-2 logs, routes alternated, 7 repetitions, median of the last 6:
one gdm_des_log_to_roll launch (HIP events), log_to_rolls end to end, writing B files from the finished tracks, and the
per-sample host route on those files (read_midi + _row_events + one piano_roll_raster launch each); the Python
restatement's log -> track time extrapolated from 16 samples; and run_spec's share of matrix_to_midi(simulate="des")
at B = 16.  Figures are printed as JSON (and written to OUT.json), nothing is asserted."""
import json, os, sys, time, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import des_midi_ref as R
from gan_des_midi_music_gen_amd import datasets, ops, sim_log_to_midi as S, simulation_v3, matrix_sim_process as msp
from gan_des_midi_music_gen_amd.simulation_v3 import EVENT_DTYPE
core = np.load(os.path.join(ROOT, "tests/golden/des_core.npz"))
def ev(k):
    out = np.zeros(len(core[f"{k}/value"]), dtype=EVENT_DTYPE)
    for f in ("value", "event_id", "node", "kind"): out[f] = core[f"{k}/{f}"]
    return out
base = [ev("midi0"), ev("midi1")]
rng = np.random.default_rng(1)
dev = torch.device("cuda")
res = {}
tmp = tempfile.mkdtemp()
for B in (16, 256):
    logs = [base[i % 2][int(rng.integers(0, 3000)):][:6000] for i in range(B)]
    tails = rng.random((B, 10)).astype(np.float32)
    inst = rng.integers(0, 127, (B, 61)); notes = rng.integers(0, 128, (B, 61))
    save = [True] * B
    # device tensors prepared once for the launch-only timing
    heads = [l[:5000] for l in logs]
    ptr = np.zeros(B + 1, np.int64); np.cumsum([len(h) for h in heads], out=ptr[1:])
    rec = np.concatenate(heads)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (up(rec["value"]), up(rec["event_id"]), up(rec["node"]), up(rec["kind"]), up(ptr), up(tails),
            up(inst.astype(np.int32)), up(notes.astype(np.int32)), up(np.ones(B, np.int32)), 0, 50, 100)
    rolls, tracks = S.log_to_rolls(logs, tails, inst, notes, start=0, end=50, save=save)
    paths = [S.write_midi(t, os.path.join(tmp, f"{B}_{i}.mid")) for i, t in enumerate(tracks)]
    host_planes = datasets.generate_piano_rolls(paths, 100, 50, 0, 50)
    assert torch.equal(host_planes[0], rolls[:, 0]) and torch.equal(host_planes[1], rolls[:, 1])
    launch, e2e, host_raster, host_write = [], [], [], []
    for rep in range(7):                      # alternate the routes
        ops.time_entry_point("gdm_des_log_to_roll")      # events around the C call alone, not the wrapper's checks
        torch.cuda.synchronize(); ops.des_log_to_roll(*args); torch.cuda.synchronize()
        launch.append(ops.timed_durations_ms()[0]); ops.time_entry_point(None)
        t0 = time.perf_counter(); S.log_to_rolls(logs, tails, inst, notes, start=0, end=50, save=save); torch.cuda.synchronize()
        e2e.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for i, t in enumerate(tracks): S.write_midi(t, paths[i])
        host_write.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for pth in paths:                      # the per-sample host route that exists at the parent commit
            md = datasets.read_midi(pth); rp, st, ve = datasets._row_events(md, 100, 50)
            ops.piano_roll_raster(up(np.concatenate([[0], rp[1:]]).astype(np.int32)), up(st), up(ve), 1, 50)
        torch.cuda.synchronize()
        host_raster.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for i in range(min(B, 16)): R.consume({k: logs[i][k] for k in EVENT_DTYPE.names}, tails[i], inst[i], notes[i], generate=True, start=0, end=50)
    py_track = (time.perf_counter() - t0) * 1e3 / min(B, 16) * B
    med = lambda x: float(np.median(x[1:]))
    res[f"B{B}"] = {"launch_ms_device": med(launch), "launch_all": launch, "log_to_rolls_wall_ms": med(e2e),
                    "host_file_write_ms": med(host_write), "host_read_rowevents_raster_per_sample_ms": med(host_raster),
                    "python_restatement_log_to_track_ms_extrapolated": py_track}
# share of run_spec in matrix_to_midi(simulate="des")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
g1 = torch.from_numpy(np.tile(d["midi/g1"], (4, 1, 1))).unsqueeze(1).to(dev); g2 = torch.from_numpy(np.tile(d["midi/g2"], (4, 1))).to(dev)
spent = [0.0]; orig = simulation_v3.run_spec
def timed(*a, **k):
    t0 = time.perf_counter(); r = orig(*a, **k); spent[0] += time.perf_counter() - t0; return r
simulation_v3.run_spec = timed
shares = []
for rep in range(4):
    np.random.seed(3); spent[0] = 0.0
    t0 = time.perf_counter(); msp.matrix_to_midi(g1, g2, adj_size=(64, 64), start=100, end=150, simulate="des", return_tensor=True)
    torch.cuda.synchronize(); tot = time.perf_counter() - t0
    shares.append({"total_ms": tot * 1e3, "run_spec_ms": spent[0] * 1e3, "share": spent[0] / tot})
res["matrix_to_midi_B16"] = shares
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
