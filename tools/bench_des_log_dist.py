"""The logging kernel with a kind per node beside the one it was factored out of, and the two queue-track launches on its
logs.  On an MI355X:

    python tools/bench_des_log_dist.py [OUT.json]

Inputs as in tools/bench_des_dist.py (model 2's bridge geometry: 61 nodes, capacities 254, the bridges' customer counts;
B = 256 and B = 48; the bridges' cap of 5001 records).  Per B, after one warm-up pass, seven passes that alternate the
launches, each from fresh copies of the same generator states, timed with HIP events on the stream:

    batch_ms          gdm_des_run_batch (kernel + pack step)
    dist_normal_ms    gdm_des_run_batch_dist with every kind 0: the same events as batch_ms, bytes compared
    dist_expon_ms     gdm_des_run_batch_dist with every kind 1 and scale = the node's mean (loc), another chain
    tracks_count_ms   gdm_des_log_tracks_count on the exponential logs, every server a column
    tracks_fill_ms    gdm_des_log_tracks on the same logs (the 8-byte read-back between the two is outside both)

Figures are printed as JSON (and written to OUT.json); the all-normal run is compared with batch_ms's bytes, the
exponential one and its tracks with the host mirrors once, nothing else is asserted."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops, simlog_to_vid as sl, simulation_v3 as sv  # noqa: E402

dev = torch.device("cuda")
d = np.load(os.path.join(ROOT, "tests/golden/des_prologue_rng.npz"))
PASSES = 7
MAX_RECORDS = 5001
MAX_LINES = 5000
args = sys.argv[1:]


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
    head = (pro.routing, up(pro.loc, torch.float64), up(pro.scale, torch.float64))
    tail = (up(pro.queue_cap, torch.int32), up(pro.seed, torch.int64), up(pro.customers, torch.int64))
    dim = int(pro.routing.shape[1])
    zeros = torch.zeros((b, dim), dtype=torch.int32, device=dev)
    ones = torch.ones((b, dim), dtype=torch.int32, device=dev)
    expon = (pro.routing, head[1], head[1])                                       # scale = the mean; loc is not read
    state0 = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32), up(gauss, torch.float64))
    fresh = lambda: tuple(t.clone() for t in state0)                              # noqa: E731
    kw = dict(max_queue_cap=254, max_records=MAX_RECORDS)

    old = ops.des_run_batch(*head, *tail, *fresh(), **kw)
    normal = ops.des_run_batch_dist(*head, zeros, *tail, *fresh(), **kw)
    n = int(old[4][-1])
    for i in range(7):
        got, want = normal[i].cpu().numpy(), old[i].cpu().numpy()
        assert (got[:n] if i < 4 else got).tobytes() == (want[:n] if i < 4 else want).tobytes(), i
    ex = ops.des_run_batch_dist(*expon, ones, *tail, *fresh(), **kw)
    host = sv.run_batch_host(pro.routing.cpu().numpy(), pro.loc, pro.loc, pro.queue_cap, pro.seed, pro.customers,
                             pro.states, math=1, max_queue_cap=254, max_records=MAX_RECORDS,
                             kind=np.ones((b, dim), dtype=np.int32))
    n_ex = int(host.rec_ptr[-1])
    for i, f in enumerate(("value", "event_id", "node", "kind")):
        assert ex[i][:n_ex].cpu().numpy().tobytes() == getattr(host, f).tobytes(), f
    assert ex[4].cpu().numpy().tobytes() == host.rec_ptr.tobytes()

    # the tracks of the exponential logs: every server of a sample a column, in node order
    is_server = (torch.diagonal(pro.routing, dim1=1, dim2=2) <= 0).cpu().numpy()
    s = int(is_server.sum(axis=1).max())
    col = np.full((b, dim), -1, dtype=np.int32)
    for i in range(b):
        # a sample with fewer servers than the widest gets its remaining columns from its sources (they never log)
        order = np.concatenate([np.nonzero(is_server[i])[0], np.nonzero(~is_server[i])[0]])[:s]
        col[i, order] = np.arange(s)
    col_d = up(col, torch.int32)
    node, kind, rec_ptr = ex[2], ex[3], ex[4]
    tracks, row_ptr, n_rows, status = ops.des_log_tracks(node, kind, rec_ptr, col_d, s, max_lines=MAX_LINES)
    servers = np.argsort(np.where(col < 0, 1 << 20, col), axis=1, kind="stable")[:, :s]
    want_tracks, want_ptr = sl.log_tracks(host, servers, max_lines=MAX_LINES, dim=dim)
    assert not status.any() and row_ptr.cpu().numpy().tobytes() == want_ptr.tobytes()
    assert tracks.cpu().numpy().tobytes() == want_tracks.tobytes()
    total = int(row_ptr[-1])

    def count():
        ops._call("gdm_des_log_tracks_count", ops._p(node), ops._p(kind), ops._p(rec_ptr), node.numel(), b, dim,
                  ops._p(col_d), MAX_LINES, ops._p(n_rows), ops._p(row_ptr), ops._p(status), ops._stream())

    def fill():
        ops._call("gdm_des_log_tracks", ops._p(node), ops._p(kind), ops._p(rec_ptr), node.numel(), b, dim, ops._p(col_d), s,
                  MAX_LINES, ops._p(row_ptr), total, ops._p(tracks), ops._stream())

    runs = {"batch_ms": lambda st: ops.des_run_batch(*head, *tail, *st, **kw),
            "dist_normal_ms": lambda st: ops.des_run_batch_dist(*head, zeros, *tail, *st, **kw),
            "dist_expon_ms": lambda st: ops.des_run_batch_dist(*expon, ones, *tail, *st, **kw),
            "tracks_count_ms": lambda st: count(), "tracks_fill_ms": lambda st: fill()}
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
    res.update(dim=dim, track_columns=s, track_rows=total, records_normal=n, records_expon=n_ex,
               stop_reasons_normal=sorted({int(x) for x in old[6].cpu()}),
               stop_reasons_expon=sorted({int(x) for x in ex[6].cpu()}))
    return res


res = {f"B{b}": measure(b) for b in (256, 48)}
if args:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
