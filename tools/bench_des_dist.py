"""The statistics kernel with a kind per node beside the one it was factored out of.  On an
MI355X:

    python tools/bench_des_dist.py [OUT.json] [--parent-lib PATH]

Inputs as in tools/bench_des_stats.py (model 2's bridge geometry: 61 nodes, capacities 254, the bridges' customer counts;
B = 256 and B = 48).  Per B, after one warm-up pass, seven passes that alternate the launches, each from fresh copies of
the same generator states, timed with HIP events on the stream:

    stats_parent_ms   gdm_des_stats_batch of the library at PATH (a build of the parent commit), when given
    stats_ms          gdm_des_stats_batch of this tree
    dist_normal_ms    gdm_des_stats_batch_dist with every kind 0: the same events as stats_ms, bytes compared
    dist_expon_ms     gdm_des_stats_batch_dist with every kind 1 and scale = the node's mean (loc), another chain

with the processed events per sample of each chain.  Figures are printed as JSON (and written to OUT.json); the all-normal
run is compared with stats_ms's bytes and the exponential one with the host mirror once, nothing else is asserted."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import _lib, matrix_sim_process as msp, ops, simulation_v3 as sv  # noqa: E402

dev = torch.device("cuda")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
PASSES = 7
args = sys.argv[1:]
parent = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    _lib.load()                                            # torch's HIP runtime first, as for the shipped library
    parent = ctypes.CDLL(os.path.abspath(args[i + 1]))
    parent.gdm_des_stats_batch.restype, parent.gdm_des_stats_batch.argtypes = _lib.SIGNATURES["gdm_des_stats_batch"]
    del args[i:i + 2]


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def parent_stats(fixed, state, out, ws):
    """gdm_des_stats_batch of the parent's library on preallocated outputs (the call ops.des_run_stats makes)."""
    adj, loc, scale, qcap, seed, cust = fixed
    p = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    rc = parent.gdm_des_stats_batch(p(adj), adj.shape[0], adj.shape[1], p(loc), p(scale), p(qcap), p(seed), p(cust), 254,
                                    200000, *(p(t) for t in state),
                                    *(p(out[n]) for n, _dt in ops.DES_STATS_NODE_FIELDS + ops.DES_STATS_SAMPLE_FIELDS),
                                    None, p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, parent.gdm_last_error()
    return out


def measure(b):
    reps = b // 4
    g1 = torch.from_numpy(np.tile(d["midi/g1"], (reps, 1, 1))).unsqueeze(1).to(dev)
    g2 = torch.from_numpy(np.tile(d["midi/g2"], (reps, 1))).to(dev)
    np.random.seed(3)
    pro = msp.batched_prologue_midi(g1, g2, (64, 64), None)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)   # noqa: E731
    key, pos, has, gauss = sv.pack_states(pro.states, b)
    head = (pro.routing, up(pro.loc, torch.float64), up(pro.scale, torch.float64))
    tail = (up(pro.queue_cap, torch.int32), up(pro.seed, torch.int64), up(pro.customers, torch.int64))
    dim = int(pro.routing.shape[1])
    zeros = torch.zeros((b, dim), dtype=torch.int32, device=dev)
    ones = torch.ones((b, dim), dtype=torch.int32, device=dev)
    expon = (pro.routing, head[1], head[1])                                       # scale = the mean; loc is not read
    state0 = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32), up(gauss, torch.float64))
    fresh = lambda: tuple(t.clone() for t in state0)                              # noqa: E731

    stats = ops.des_run_stats(*head, *tail, *fresh(), max_queue_cap=254)
    normal = ops.des_run_stats_dist(*head, zeros, *tail, *fresh(), max_queue_cap=254)
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert normal[f].cpu().numpy().tobytes() == stats[f].cpu().numpy().tobytes(), f
    ex = ops.des_run_stats_dist(*expon, ones, *tail, *fresh(), max_queue_cap=254)
    host = sv.run_stats_host(pro.routing.cpu().numpy(), pro.loc, pro.loc, pro.queue_cap, pro.seed, pro.customers,
                             pro.states, math=1, max_queue_cap=254, kind=np.ones((b, dim), dtype=np.int32))
    for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
        assert ex[f].cpu().numpy().tobytes() == getattr(host, f).tobytes(), f
    runs = {"stats_ms": lambda st: ops.des_run_stats(*head, *tail, *st, max_queue_cap=254),
            "dist_normal_ms": lambda st: ops.des_run_stats_dist(*head, zeros, *tail, *st, max_queue_cap=254),
            "dist_expon_ms": lambda st: ops.des_run_stats_dist(*expon, ones, *tail, *st, max_queue_cap=254)}
    if parent is not None:
        out = {n: torch.empty_like(stats[n]) for n, _dt in ops.DES_STATS_NODE_FIELDS + ops.DES_STATS_SAMPLE_FIELDS}
        ws = torch.empty(ops.des_stats_workspace_bytes(b, dim, 254), dtype=torch.uint8, device=dev)
        runs = {"stats_parent_ms": lambda st: parent_stats(head + tail, st, out, ws), **runs}
        parent_stats(head + tail, fresh(), out, ws)
        torch.cuda.synchronize()
        for f in sv.STATS_NODE_FIELDS + sv.STATS_SAMPLE_FIELDS:
            assert out[f].cpu().numpy().tobytes() == stats[f].cpu().numpy().tobytes(), f
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
    res = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    res["dim"] = dim
    res["events_per_sample_normal"] = float(stats["events"].double().mean())
    res["events_max_normal"] = int(stats["events"].max())
    res["events_per_sample_expon"] = float(ex["events"].double().mean())
    res["events_max_expon"] = int(ex["events"].max())
    res["stop_reasons_normal"] = sorted({int(x) for x in stats["stop_reason"].cpu()})
    res["stop_reasons_expon"] = sorted({int(x) for x in ex["stop_reason"].cpu()})
    for k, ev in (("stats_ms", "events_max_normal"), ("dist_normal_ms", "events_max_normal"),
                  ("dist_expon_ms", "events_max_expon")):
        res[k]["us_per_event_of_the_longest_chain"] = 1e3 * res[k]["median"] / res[ev]
        res[k]["us_per_mean_event"] = 1e3 * res[k]["median"] / res[ev.replace("events_max", "events_per_sample")]
    return res


res = {f"B{b}": measure(b) for b in (256, 48)}
if args:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
