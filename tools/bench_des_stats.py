"""The log-free statistics kernel against the logging kernel on the same inputs.  On an MI355X:

    python tools/bench_des_stats.py [OUT.json]

Inputs with the bridges' own geometry, those of tools/bench_des_batch.py's model 2 leg: the four golden generator
outputs tiled to B = 256 and B = 48, through the batched prologue (routing matrices from ops.des_routing at adj_size
64 x 64 -- 61 nodes --, the bridges' parameters, capacities of 254 and customer counts).  Per B, after one warm-up pass,
seven passes that alternate the four launches, each from fresh copies of the same generator states, timed with HIP
events on the stream:

    log_ms           gdm_des_run_batch, max_records = 5001: what the bridges run (kernel + pack); a sample stops at
                     its 5001st record
    stats_ms         gdm_des_stats_batch: no record cap, so every sample runs to its number_of_customers
    log_uncapped_ms  gdm_des_run_batch with a cap above the longest run: the same events as stats_ms
    stats_capped_ms  gdm_des_stats_batch stopped by max_events after about as many events as log_ms processes
                     (5001 x the statistics run's events per record): the same length of chain as log_ms

with the processed events per sample of the statistics run and the records per sample of each.  Figures are printed as
JSON (and written to OUT.json); the statistics are compared with the host mirror once, nothing else is asserted."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402

dev = torch.device("cuda")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
CAP, PASSES = 5001, 7


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def measure(b):
    reps = b // 4
    g1 = torch.from_numpy(np.tile(d["midi/g1"], (reps, 1, 1))).unsqueeze(1).to(dev)
    g2 = torch.from_numpy(np.tile(d["midi/g2"], (reps, 1))).to(dev)
    np.random.seed(3)
    pro = msp.batched_prologue_midi(g1, g2, (64, 64), None)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)   # noqa: E731
    key, pos, has, gauss = sv.pack_states(pro.states, b)
    fixed = (pro.routing, up(pro.loc, torch.float64), up(pro.scale, torch.float64), up(pro.queue_cap, torch.int32),
             up(pro.seed, torch.int64), up(pro.customers, torch.int64))
    state0 = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32), up(gauss, torch.float64))
    fresh = lambda: tuple(t.clone() for t in state0)                              # noqa: E731

    stats = ops.des_run_stats(*fixed, *fresh(), max_queue_cap=254)                # warm-up, and the work there is
    n_rec = stats["n_records"].cpu().numpy()
    uncapped = int(n_rec.max()) + 1
    host = sv.run_stats_host(pro.routing.cpu().numpy(), pro.loc, pro.scale, pro.queue_cap, pro.seed, pro.customers,
                             pro.states, math=1, max_queue_cap=254)
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert stats[f].cpu().numpy().tobytes() == getattr(host, f).tobytes(), f
    like_log = max(1, int(round(CAP * float(stats["events"].sum()) / float(n_rec.sum()))))
    runs = {"log_ms": lambda st: ops.des_run_batch(*fixed, *st, max_queue_cap=254, max_records=CAP),
            "stats_ms": lambda st: ops.des_run_stats(*fixed, *st, max_queue_cap=254),
            "log_uncapped_ms": lambda st: ops.des_run_batch(*fixed, *st, max_queue_cap=254, max_records=uncapped),
            "stats_capped_ms": lambda st: ops.des_run_stats(*fixed, *st, max_queue_cap=254, max_events=like_log)}
    for fn in runs.values():
        fn(fresh())
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(PASSES):
        for k, fn in runs.items():
            state = fresh()                                # the states are updated in place: copied outside the window
            torch.cuda.synchronize()
            _, ms = device_ms(lambda: fn(state))
            times[k].append(ms)
    log = ops.des_run_batch(*fixed, *fresh(), max_queue_cap=254, max_records=CAP)
    out = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    out["events_stats_capped"] = like_log
    out["dim"] = int(pro.routing.shape[1])
    out["events_per_sample_stats"] = float(stats["events"].double().mean())
    out["records_per_sample_stats"] = float(n_rec.mean())
    out["records_max_stats"] = int(n_rec.max())
    out["records_per_sample_log"] = float(log[5].double().mean())
    out["stop_reasons_stats"] = sorted({int(x) for x in stats["stop_reason"].cpu()})
    out["stop_reasons_log"] = sorted({int(x) for x in log[6].cpu()})
    return out


res = {f"B{b}": measure(b) for b in (256, 48)}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
