"""The kernels with 'queue' and 'branch' nodes beside the ones they share their bodies with.
On an MI355X:

    python tools/bench_des_net.py [OUT.json] [--parent-lib PATH]

Inputs as in tools/bench_des_dist.py (model 2's bridge geometry: 61 nodes, capacities 254, the bridges' customer counts;
B = 256 and B = 48).  Per B, after one warm-up pass, seven passes that alternate the launches, each from fresh copies of
the same generator states, timed with HIP events on the stream.  Every entry is called through ctypes on preallocated
outputs, the parent's library and this tree's alike:

    parent/<entry>, parent_again/<entry>   the six device entries -- gdm_des_stats_batch, gdm_des_stats_batch_dist and
                      gdm_des_stats_batch_net (kinds 0), gdm_des_run_batch, gdm_des_run_batch_dist and
                      gdm_des_run_batch_net (kinds 0) -- of the library at PATH (a build of the parent commit), when
                      given, measured twice in the same passes: the difference of the two medians is the spread a
                      difference to this tree is read against
    tree/<entry>      the same entries of this tree
    tree/gdm_des_stats_batch_dist_expon, tree/gdm_des_stats_batch_net_expon, ..._run_batch_...   the _net kernels on
                      all-exponential kinds (scale = the node's mean) beside the _dist kernels on the same inputs,
                      bytes compared
    mmck/...          one M/M/c sweep batch through gdm_des_stats_batch_net: c = 4, lam = 6, mu = 1, capacity 2,
                      B samples x 4000 customers (about 12 700 events per sample), with the histogram

Figures are printed as JSON (and written to OUT.json); besides the byte comparisons nothing is asserted."""
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
MAX_RECORDS = 5001
EXISTING = ("gdm_des_stats_batch", "gdm_des_stats_batch_dist", "gdm_des_stats_batch_net",
            "gdm_des_run_batch", "gdm_des_run_batch_dist", "gdm_des_run_batch_net")
STAT_FIELDS = tuple(n for n, _dt in ops.DES_STATS_NODE_FIELDS + ops.DES_STATS_SAMPLE_FIELDS)
LOG_FIELDS = ("value", "event_id", "node", "kind", "rec_ptr", "n_records", "stop_reason")
args = sys.argv[1:]
tree = _lib.load()                                         # torch's HIP runtime first, as for the shipped library
parent = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    parent = ctypes.CDLL(os.path.abspath(args[i + 1]))
    for name in EXISTING:
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    del args[i:i + 2]


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


class Inputs:
    """Device inputs of one batch and preallocated outputs for both families of entries."""

    def __init__(self, adj, loc, scale, qcap, seed, cust, states, max_queue_cap, max_events, histogram=False):
        up = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).to(dt)  # noqa: E731
        self.b, self.dim = int(adj.shape[0]), int(adj.shape[1])
        self.head = (up(adj, torch.float64).contiguous(), up(loc, torch.float64), up(scale, torch.float64))
        self.tail = (up(qcap, torch.int32), up(seed, torch.int64), up(cust, torch.int64))
        key, pos, has, gauss = sv.pack_states(states, self.b)
        self.state0 = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32),
                       up(gauss, torch.float64))
        self.cap, self.max_events = int(max_queue_cap), int(max_events)
        b, dim = self.b, self.dim
        self.stats = {n: torch.empty((b, dim), dtype=dt, device=dev) for n, dt in ops.DES_STATS_NODE_FIELDS}
        self.stats.update({n: torch.empty(b, dtype=dt, device=dev) for n, dt in ops.DES_STATS_SAMPLE_FIELDS})
        self.hist = torch.empty((b, dim, self.cap + 1), dtype=torch.float64, device=dev) if histogram else None
        n = b * MAX_RECORDS
        self.log = {"value": torch.empty(n, dtype=torch.float64, device=dev),
                    "event_id": torch.empty(n, dtype=torch.int64, device=dev),
                    "node": torch.empty(n, dtype=torch.int32, device=dev),
                    "kind": torch.empty(n, dtype=torch.int32, device=dev),
                    "rec_ptr": torch.empty(b + 1, dtype=torch.int64, device=dev),
                    "n_records": torch.empty(b, dtype=torch.int64, device=dev),
                    "stop_reason": torch.empty(b, dtype=torch.int32, device=dev)}
        self.ws = torch.empty(ops.des_stats_workspace_bytes(b, dim, self.cap), dtype=torch.uint8, device=dev)

    def fresh(self):
        return tuple(t.clone() for t in self.state0)

    def call(self, lib, name, state, kind=None, head=None):
        """One entry of ``lib`` on the preallocated outputs (the call ops.des_run_stats / des_run_batch make)."""
        adj, loc, scale = head or self.head
        first = (p(adj), self.b, self.dim, p(loc), p(scale), *(() if kind is None else (p(kind),)),
                 *(p(t) for t in self.tail), self.cap, self.max_events)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if "_stats_" in name:
            rc = getattr(lib, name)(*first, *(p(t) for t in state), *(p(self.stats[n]) for n in STAT_FIELDS),
                                    p(self.hist), p(self.ws), self.ws.numel(), stream)
        else:
            lg = self.log
            rc = getattr(lib, name)(*first, MAX_RECORDS, *(p(t) for t in state), p(lg["value"]), p(lg["event_id"]),
                                    p(lg["node"]), p(lg["kind"]), self.b * MAX_RECORDS, p(lg["rec_ptr"]),
                                    p(lg["n_records"]), p(lg["stop_reason"]), p(self.ws), self.ws.numel(), stream)
        assert rc == 0, lib.gdm_last_error()

    def result(self, name):
        """The bytes an entry of that family last wrote (records: the packed part)."""
        torch.cuda.synchronize()
        if "_stats_" in name:
            return [self.stats[n].cpu().numpy().tobytes() for n in STAT_FIELDS]
        n = int(self.log["rec_ptr"][-1])
        return [self.log[f][:n].cpu().numpy().tobytes() if f in LOG_FIELDS[:4] else self.log[f].cpu().numpy().tobytes()
                for f in LOG_FIELDS]


def timed(runs, fresh):
    for fn in runs.values():
        fn(fresh())
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(PASSES):
        for k, fn in runs.items():
            state = fresh()                                # the states are updated in place: copied outside the window
            torch.cuda.synchronize()
            times[k].append(device_ms(lambda: fn(state)))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def measure(b):
    reps = b // 4
    g1 = torch.from_numpy(np.tile(d["midi/g1"], (reps, 1, 1))).unsqueeze(1).to(dev)
    g2 = torch.from_numpy(np.tile(d["midi/g2"], (reps, 1))).to(dev)
    np.random.seed(3)
    pro = msp.batched_prologue_midi(g1, g2, (64, 64), None)
    x = Inputs(pro.routing, pro.loc, pro.scale, pro.queue_cap, pro.seed, pro.customers, pro.states, 254, 200000)
    zeros = torch.zeros((b, x.dim), dtype=torch.int32, device=dev)
    ones = torch.ones((b, x.dim), dtype=torch.int32, device=dev)
    expon = (x.head[0], x.head[1], x.head[1])                                     # scale = the mean; loc is not read
    kinds = {name: zeros if name.endswith(("_dist", "_net")) else None for name in EXISTING}

    # what is timed against what computes the same bytes
    want = {}
    for name in EXISTING:
        x.call(tree, name, x.fresh(), kinds[name])
        want[name] = x.result(name)
        if parent is not None:
            x.call(parent, name, x.fresh(), kinds[name])
            assert x.result(name) == want[name], name
    events = {"normal": x.stats["events"].double().mean().item(), "normal_max": int(x.stats["events"].max())}
    for fam in ("stats", "run"):
        x.call(tree, f"gdm_des_{fam}_batch_dist", x.fresh(), ones, expon)
        dist = x.result(f"gdm_des_{fam}_batch_dist")
        if fam == "stats":
            events.update(expon=x.stats["events"].double().mean().item(), expon_max=int(x.stats["events"].max()))
        x.call(tree, f"gdm_des_{fam}_batch_net", x.fresh(), ones, expon)
        assert x.result(f"gdm_des_{fam}_batch_net") == dist, fam

    runs = {}
    for name in EXISTING:
        if parent is not None:
            runs[f"parent/{name}"] = lambda st, name=name: x.call(parent, name, st, kinds[name])
        runs[f"tree/{name}"] = lambda st, name=name: x.call(tree, name, st, kinds[name])
        if parent is not None:
            runs[f"parent_again/{name}"] = lambda st, name=name: x.call(parent, name, st, kinds[name])
    for fam in ("stats", "run"):
        for pol in ("dist", "net"):
            runs[f"tree/gdm_des_{fam}_batch_{pol}_expon"] = \
                lambda st, n=f"gdm_des_{fam}_batch_{pol}": x.call(tree, n, st, ones, expon)
    res = timed(runs, x.fresh)
    res["dim"], res["events_per_sample"] = x.dim, events
    if parent is not None:
        for name in EXISTING:
            a, t, again = (res[f"{k}/{name}"]["median"] for k in ("parent", "tree", "parent_again"))
            res[f"summary/{name}"] = {"tree_over_parent": t / (0.5 * (a + again)),
                                      "parent_spread": abs(a - again) / (0.5 * (a + again))}
    return res


def measure_mmck(b):
    c, lam, mu, cap, customers = 4, 6.0, 1.0, 2, 4000
    specs = [sv.mmck_spec(c, lam, mu, cap, customers, seed) for seed in range(b)]
    adj, kind, loc, scale, qcap, seed, cust = sv.net_arrays(specs)
    x = Inputs(adj, loc, scale, qcap, seed, cust, sv.replication_states(range(b)), cap, 16 * customers + 64, True)
    k = torch.from_numpy(kind).to(dev)
    x.call(tree, "gdm_des_stats_batch_net", x.fresh(), k)
    torch.cuda.synchronize()
    host = sv.run_stats_host(adj, loc, scale, qcap, seed, cust, sv.replication_states(range(b)), math=1,
                             max_queue_cap=cap, max_events=16 * customers + 64, histogram=True, kind=kind, net=True)
    for f in STAT_FIELDS:
        assert x.stats[f].cpu().numpy().tobytes() == getattr(host, f).tobytes(), f
    assert x.hist.cpu().numpy().tobytes() == host.queue_time.tobytes()
    res = timed({"mmck/gdm_des_stats_batch_net": lambda st: x.call(tree, "gdm_des_stats_batch_net", st, k)}, x.fresh)
    res["events_per_sample"] = float(host.events.mean())
    res["events_max"] = int(host.events.max())
    res["mmck/gdm_des_stats_batch_net"]["us_per_event_of_the_longest_chain"] = \
        1e3 * res["mmck/gdm_des_stats_batch_net"]["median"] / res["events_max"]
    return res


res = {f"B{b}": {**measure(b), **{f"mmck_{k}" if not k.startswith("mmck") else k: v
                                  for k, v in measure_mmck(b).items()}} for b in (256, 48)}
if args:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
