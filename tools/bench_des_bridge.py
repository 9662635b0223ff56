"""Stage times of model 1's DES bridge at the reference's batch, B = 30.  On an MI355X:

    python tools/bench_des_bridge.py [OUT.json]

matrix_to_wav(simulate="des") taken apart: the host part (per sample: draws, one-sample routing launch, run_spec; wall
clock), the upload of the B logs (wall clock, ends in a synchronise), and the three device stages -- log -> notes,
notes -> STFT frames, frames -> mel dB -- each between HIP events on the stream.  One warm-up pass, then the median of
three.  The matrices are the five of tests/golden/des_prologue_rng.npz repeated six times under a fixed numpy seed, so
the DES logs are the size real generator output gives (tens of thousands of events, about 900 notes per clip).
Figures are printed as JSON (and written to OUT.json); nothing is asserted and there is no parent to compare with."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_v3, util  # noqa: E402
from gan_des_midi_music_gen_amd.sim_log_process_music import MAX_LINES  # noqa: E402

B = 30
dev = torch.device("cuda")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
matrices = torch.from_numpy(np.tile(d["wav/matrices"], (6, 1, 1))[:B]).to(dev)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def one_pass():
    t = {}
    np.random.seed(int(d["wav/np_seed"]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logs, levels = [], []
    for spec in msp.WAV.specs(msp.WAV.scan(matrices, 20)):
        logs.append(simulation_v3.run_spec(spec)[0])
        levels.append([int(x) for x in spec.note_levels])
    t["host_des_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    heads = [lg[:MAX_LINES] for lg in logs]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(x) for x in heads], out=ptr[1:])
    rec = np.concatenate(heads)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    args = (up(rec["value"]), up(rec["event_id"]), up(rec["node"]), up(rec["kind"]), up(ptr),
            up(np.asarray(levels, dtype=np.int32)))
    torch.cuda.synchronize()
    t["upload_ms"] = (time.perf_counter() - t0) * 1e3
    (notes, n_notes, clip_len, _status), t["stage_a_notes_ms"] = device_ms(lambda: ops.des_log_to_notes(*args))
    frames, t["stage_b_frames_ms"] = device_ms(lambda: ops.synth_frames(notes, n_notes, clip_len))
    _mel, t["mel_chain_ms"] = device_ms(lambda: util._db_from_frames(frames, B, 216, 44100, 2048, 128, 20, 8300, 80))
    t["events_per_log"] = float(np.mean([len(lg) for lg in logs]))
    t["notes_per_clip"] = float(n_notes.float().mean())
    t["seconds_per_clip"] = float(clip_len.float().mean()) / 44100.0
    return t


one_pass()                                     # warm-up: code objects, the cached DFT / mel matrices, the allocator
passes = [one_pass() for _ in range(3)]
res = {"B": B, "median_of_3": {k: float(np.median([p[k] for p in passes])) for k in passes[0]}, "passes": passes}
t0 = time.perf_counter()
np.random.seed(int(d["wav/np_seed"]))
msp.matrix_to_wav(matrices, size=20, start=0, end=216, device=dev, simulate="des")
torch.cuda.synchronize()
res["matrix_to_wav_wall_ms"] = (time.perf_counter() - t0) * 1e3
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
