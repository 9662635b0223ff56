"""The batched device simulator behind both DES bridges.  On an MI355X:

    python tools/bench_des_batch.py [OUT.json]

Model 1 at B = 30 on the inputs of tools/bench_des_bridge.py (f7), model 2 at B = 16 and B = 256 on those of
tools/bench_des_midi.py (f5: the four golden generator outputs, tiled).  Per size, with the method of f7 -- one warm-up
pass, then the median of three; wall clock ending in a synchronise for what involves the host, HIP events on the stream
for launches:

    des_ms              matrix_to_wav / matrix_to_midi(simulate="des"), end to end      } alternated
    des_batch_device_ms the same call with simulate="des_batch", end to end, kernel route  } pass by pass
    des_batch_host_ms   ... and with the host-mirror route (DES_BATCH_DEVICE_MIN_B picks)  }
    launch_ms           gdm_des_run_batch alone (one wave per sample + pack), inputs on the device
    pack_ms             gdm_des_pack alone on that launch's output
    host_mirror_ms      gdm_des_run_batch_host (portable math), sequential, same specs, same 5001-record cap
    host_draws_ms       the host draws of the batched prologue (B x: sources, dim residue columns, reseed, snapshot)
    prologue_ms         the whole batched prologue (scan launch + read-back, draws, routing launch, parameter build)

Figures are printed as JSON (and written to OUT.json); nothing is asserted."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402

dev = torch.device("cuda")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
CAP = 5001
default_min_b = msp.DES_BATCH_DEVICE_MIN_B


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def measure(seed, end_to_end, prologue, scan, draws):
    def one_pass():
        t = {}
        for mode, min_b in (("des", None), ("des_batch", 1), ("des_batch", 1 << 30)):
            np.random.seed(seed)
            name = mode if min_b is None else ("des_batch_device" if min_b == 1 else "des_batch_host")
            msp.DES_BATCH_DEVICE_MIN_B = default_min_b if min_b is None else min_b
            _, t[f"{name}_ms"] = wall_ms(lambda: end_to_end(mode))
        msp.DES_BATCH_DEVICE_MIN_B = default_min_b
        np.random.seed(seed)
        pro, t["prologue_ms"] = wall_ms(prologue)
        b = pro.h["b"]
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)   # noqa: E731
        key, pos, has, gauss = sv.pack_states(pro.states, b)
        fixed = (pro.routing, up(pro.loc, torch.float64), up(pro.scale, torch.float64), up(pro.queue_cap, torch.int32),
                 up(pro.seed, torch.int64), up(pro.customers, torch.int64))
        state = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32), up(gauss, torch.float64))
        out, t["launch_ms"] = device_ms(lambda: ops.des_run_batch(*fixed, *state, max_queue_cap=254, max_records=CAP))
        value, event_id, node, kind, rec_ptr, n_records, stop = out
        _, t["pack_ms"] = device_ms(lambda: ops.des_pack(n_records, rec_ptr, value, event_id, node, kind, CAP))
        routing = pro.routing.cpu().numpy()
        t0 = time.perf_counter()
        host = sv.run_batch_host(routing, pro.loc, pro.scale, pro.queue_cap, pro.seed, pro.customers, pro.states, math=1,
                                 max_records=CAP, max_queue_cap=254)
        t["host_mirror_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(rec_ptr.cpu().numpy(), host.rec_ptr) and np.array_equal(stop.cpu().numpy(), host.stop_reason)
        np.random.seed(seed)
        h = scan()
        t0 = time.perf_counter()
        for i in range(b):
            draws(h, i)
            np.random.get_state()
        t["host_draws_ms"] = (time.perf_counter() - t0) * 1e3
        t["records_per_sample"] = float(host.n_records.mean())
        t["stop_reasons"] = sorted({int(x) for x in host.stop_reason})
        return t

    one_pass()                                     # warm-up: code objects, cached matrices, the allocator
    passes = [one_pass() for _ in range(3)]
    return {"median_of_3": {k: float(np.median([p[k] for p in passes])) for k in passes[0] if k != "stop_reasons"},
            "passes": passes}


res = {}
B = 30
matrices = torch.from_numpy(np.tile(d["wav/matrices"], (6, 1, 1))[:B]).to(dev)
res["model1_B30"] = measure(
    int(d["wav/np_seed"]),
    lambda mode: msp.matrix_to_wav(matrices, size=20, start=0, end=216, device=dev, simulate=mode),
    lambda: msp.batched_prologue_wav(matrices, 20, None), lambda: msp.WAV.scan(matrices, 20), msp.WAV.draws)
for B in (16, 256):
    reps = B // 4
    g1 = torch.from_numpy(np.tile(d["midi/g1"], (reps, 1, 1))).unsqueeze(1).to(dev)
    g2 = torch.from_numpy(np.tile(d["midi/g2"], (reps, 1))).to(dev)
    res[f"model2_B{B}"] = measure(
        3, lambda mode: msp.matrix_to_midi(g1, g2, adj_size=(64, 64), start=100, end=150, simulate=mode,
                                           return_tensor=True),
        lambda: msp.batched_prologue_midi(g1, g2, (64, 64), None), lambda: msp.MIDI.scan(g1, 64, g2), msp.MIDI.draws)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
