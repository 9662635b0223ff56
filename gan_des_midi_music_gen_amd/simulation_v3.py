"""Drop-in surface of the reference's discrete-event simulator for the way its two bridges use it
(SIMULATOR/simulation_v3.py -- byte-identical copies in GAN_DES/ and MMGAN_MIDI_DES/; constructed at
MMGAN_MIDI_DES/matrix_sim_process.py:150-151 and GAN_DES/matrix_sim_process.py:106-108):

    sim = Sim(sim_matrix, distributions, queue_list, seeds=seeds, log_path="logs/", generate_log=True, animation=False,
              record_history=False, logging_mode='Music', max_sim_time=...)
    sim.run(number_of_customers=n)

behind which sits the deterministic C++ core ``gdm_des_run`` (csrc/des_core.hip, host code).
Same constructor / ``run`` signature, same 'Music' log lines in ``logs/simulation.log`` when ``generate_log`` is set,
same consumption of numpy's GLOBAL legacy random stream (routing draws: simulation_v3.py:57,62) and of the per-node
``RandomState`` streams -- under the same seeds the event sequence is the reference's, record for record
(tests/golden/des_core.npz was recorded from the reference's own ``Sim``).

Differences, on purpose:
  * the run ends after ``max_events`` processed events (default 200 000) instead of after ``max_sim_time`` seconds of
    WALL CLOCK (simulation_v3.py:496-499: the reference's results depend on how fast the machine is; ``max_sim_time`` is
    accepted and ignored);
  * only what the bridges construct is supported: 'normal' distributions, ``logging_mode='Music'``, probability routing
    (no 'queue' / 'branch' nodes, no animation, no metric history) -- anything else raises NotImplementedError (the
    log-free statistics run and ``run_batch_dist`` below also take 'exponential' and 'uniform' nodes, and 'queue' and
    'branch' nodes);
  * the log records are also kept as arrays (``sim.music_log``), so a caller need not go through the log file;
  * where the reference's run ends in an exception, ``Sim.run`` raises ValueError with the core's message, and a sample
    of ``run_batch`` / ``run_batch_host`` ends with stop reason 3 ("error") and an empty log, its neighbours untouched
    (tests/golden/des_corpus.npz records the reference's exception, tests/test_des_corpus.py pins this table):

        case                                            reference                                   here
        a customer is routed to a source node           KeyError (``self.servers[id]``, Sim.run)    ValueError / stop 3
        a source has no child with a positive flow      KeyError (``self.servers[None]``, Sim.run)  ValueError / stop 3

    In both cases the reference fails when it takes the event off the list, before the arrival is logged; the records
    written up to that point stay in its log file, while ``Sim.run`` here returns nothing.

  * the queueing statistics of the reference's ``Server`` / ``Source`` objects and ``Sim.calculate_metrics`` (752-824) are
    not attributes of ``Sim`` (``record_history`` stays refused) but the result of a log-free batched run: ``run_stats``
    / ``run_stats_host`` / ``run_stats_device`` return the accumulators as arrays with a leading B (``BatchStats``),
    ``metrics`` the derived quantities under the reference's names, NaN where the reference has no dict entry (and
    where it raises ZeroDivisionError because ``Clock == 0``), ``replicate`` their mean / std / sem over seeded runs of
    one net.  Counts and the sums the reference accumulates once per event (service, queue and inter-arrival times,
    ``Clock``) are the reference's bits with ``math=0``; the time spent at each queue length is integrated when a
    queue changes instead of on every event for every server (472-484), the same sum rounded differently (a few
    1e-16 relative; tests/test_des_stats.py).  ``clock`` is the reference's ``Clock`` and ``end_time`` its
    ``previous_time``: the event that triggers the ``number_of_customers`` stop is counted in the time integration
    but ``Clock`` is not advanced to it.  A sample that ends in an error returns zeros and keeps its generator state.
  * the statistics run and ``run_batch_dist`` -- not ``Sim``, ``run_batch``, ``spec_arrays`` or the bridges -- take
    nodes of DIST_KINDS: ``['normal', loc, s]``,
    ``['exponential', s]`` and ``['uniform', loc, s]`` as the reference's ``Server`` / ``Source`` construct them
    (181-192, 263-274).  The last two are ONE uniform double on the node's stream, in scipy's order of operations:
    ``(-log(1.0 - u)) * s + 0.0`` and ``u * s + loc``; ``s == 0`` returns loc (0.0) without a draw.  ``dist_arrays``
    parses specs, ``run_stats_host`` / ``run_stats_device`` take ``kind=``, ``run_stats`` / ``replicate`` route to the
    entries with kinds (``gdm_des_stats_batch_dist[_host]``) only when some node is not normal.  Where the reference
    would never return -- a server whose every draw is <= 0 without consuming draws: an exponential with scale 0, a
    uniform with scale 0 and loc <= 0 -- the sample stops with reason 3; a uniform whose support is <= 0 ends on the
    draw budget.  ``mm1k_sweep`` puts the simulated M/M/1/K beside ``queueing_theory.mm1k`` (tests/golden/des_dist.npz
    records the reference's own runs of the same nets; ``tools/des_validate.py`` prints the table).
  * the LOG of such nets comes from ``run_batch_dist`` (specs) or ``run_batch_host`` / ``run_batch_device`` with
    ``kind=`` (``gdm_des_run_batch_dist[_host]``; csrc/des_batch.hip: des_batch_dist_kernel): the same draws, refusals
    and stop reasons as the statistics run, the records of ``run_batch``.  With ``math=0`` the log is the reference's,
    record for record and bit for bit (tests/golden/des_log_dist.npz).  Unlike ``run_batch`` a sample that stops with
    reason 3 keeps the generator state it came with, as in the statistics run.  ``write_music_log`` writes any such
    log as the reference's ``logs/simulation.log``; ``simlog_to_vid`` turns it into queue tracks and an animation.

  * the reference's two node kinds WITHOUT a distribution (``Server.__init__``, 193-197) are taken by ``run_stats``,
    ``replicate``, ``run_batch_dist`` and ``mmck_sweep`` -- NODE_KINDS = DIST_KINDS + ('queue', 'branch'); ``Sim``,
    ``run_batch``, ``spec_arrays``, ``dist_arrays`` and the bridges keep refusing them: ``['queue']``, a waiting room in
    front of several servers (its departure takes the first idle child that is a server, and waits -- is scheduled
    again at the earliest next departure among its children, 656-697 -- while there is none), and ``['branch']``, a
    zero-time router.  Both are servers with their own FIFO and ``queue_list`` capacity, draw nothing, and write a
    ``processing`` record of value 0.  A queue node's delayed departure counts as a waiting customer in the admission
    test and in the time at queue length (557, 477), so a queue node with ``queue_list`` 0 still holds one customer
    and an M/M/c station built with ``mmck_spec`` is M/M/c/N with N = c + max(queue_cap, 1).  ``net_arrays`` parses
    such specs; ``run_stats_host`` / ``run_stats_device`` / ``run_batch_host`` / ``run_batch_device`` take
    ``net=True`` with ``kind=`` (``gdm_des_stats_batch_net[_host]``, ``gdm_des_run_batch_net[_host]``; never chosen
    from the values in ``kind``: the entries without it refuse kind 3 as ever), the spec-level functions go there only
    when some node is 'queue' or 'branch'.  With ``math=0`` log and statistics are the reference's
    (tests/golden/des_net.npz); ``mmck_sweep`` puts simulated M/M/c/N beside ``queueing_theory.mmck``.  Two more rows
    of the table above, both stop 3 with the generator state kept:

        a source is a 'queue' or 'branch' node         ValueError ("Distribution not supported")   stop 3
        a queue node must wait and every child is a     the departure is scheduled at +inf: the     stop 3
        source (none ever schedules a departure)        run is not defined by its inputs alone

  * the statistics at S customer counts of ONE run: ``number_of_customers`` enters the reference only in its stop test
    (486), so its run of n1 customers is a prefix of its run of n2 > n1, and ``run_stats_snapshots`` /
    ``run_stats_snapshots_host`` (``gdm_des_stats_batch_snap_host``, des::SnapStats in csrc/des_sim.h) leave at every
    checkpoint what ``run_stats_host`` returns for that many customers, bit for bit (tests/golden/des_snap.npz holds the
    reference's own shorter runs).  ``snapshot`` and ``window`` cut BatchStats out of them, ``convergence`` is
    ``replicate`` at every checkpoint from one batch, ``batch_means`` a confidence interval from one long run, and
    ``warmup=`` on ``replicate`` / ``mm1k_sweep`` / ``mmck_sweep`` leaves the empty-system start out.  These run on the
    host mirror; there is no kernel for them, and a device is refused by name.

  * the log customer by customer: an ``event_id`` is a customer and keeps its id from node to node, so a 'Music' log
    holds what happened to every one of them, which no per-node accumulator says.  ``log_visits``
    (``gdm_des_log_visits_host``, the walk of csrc/des_visits.h) turns the logs of a BatchLog into two tables, one row
    per VISIT (a customer's stay at one node: its arrival, service-start and departure records and their clocks) and
    one row per CUSTOMER (its visits, when it entered and left, whether it left or was turned away) -> LogVisits;
    ``visit_stats`` sums them per node (``started`` IS the statistics run's ``served``, ``service_sum`` its
    ``time_in_service`` and ``wait_sum`` its ``time_in_queue``, bit for bit on nets without queue nodes),
    ``waiting_times`` / ``sojourn_times`` / ``wait_tail`` are the distributions, and ``mm1k_wait_sweep`` puts the
    waiting-time law of simulated M/M/1/K beside ``queueing_theory.mm1k_wait_tail``.  The walk runs on the host; a
    BatchLog of device tensors is read back once, and there is no kernel for it.

  * shortest-queue routing is not built: ``FlowBranchOperator.shortest_queue`` (49-52) is set from the probabilities
    AFTER they were normalised, so it can be true only for a node without children, which the table above covers;
    ``use_next_available_server`` (731-736) is read on that path only.  ``Sim.run`` accepts and ignores the argument.

``run_batch`` / ``run_batch_host`` simulate B specs of one size at once, every sample FROM ITS OWN snapshot of numpy's
global stream (``gdm_des_run_batch`` on a HIP device: one wave per sample, csrc/des_batch.hip; ``gdm_des_run_batch_host``
on the host).  Both run the event logic of csrc/des_sim.h, the same source ``gdm_des_run`` is compiled from.  With
portable math (``math=1``, the only one on the device) the host entry is the device's oracle, bit for bit; against the
reference the event structure is the same and values differ in their last bits (libm's ``log`` is not portable).
"""
import collections
import ctypes
import os

import numpy as np

from . import _lib

ARRIVAL, DEPARTURE, PROCESSING = 0, 1, 2
KIND_NAMES = ("arrival", "departure", "processing")
EVENT_DTYPE = np.dtype([("value", np.float64), ("event_id", np.int64), ("node", np.int32), ("kind", np.int32)])
STOP_REASONS = ("event list empty", "number_of_customers reached", "max_events reached", "error", "max_records reached",
                "draw budget exhausted")         # GDM_DES_STOP_*; the last two: the batch entries only


class Sim:
    arrival = 1
    departure = 2

    def __init__(self, adj_matrix, distributions, queue_list, seeds=None, num_runs=None, generate_log=False,
                 log_path='logs/', log_name=None, animation=False, record_history=False, logging_mode='All',
                 max_sim_time=1000, verbose=False, max_events=200000):
        if logging_mode != 'Music':
            raise NotImplementedError("only logging_mode='Music' (what matrix_to_midi / matrix_to_wav use) is built")
        if animation or record_history:
            raise NotImplementedError("animation / metric history of the reference's Sim are out of scope")
        if seeds is not None:
            self.seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
        elif num_runs is not None:
            raise TypeError("can only concatenate list (not \"int\") to list")      # simulation_v3.py:353, as upstream
        else:
            raise ValueError("Either seeds or num_runs must be provided.")
        self.num_runs = len(self.seeds)
        self.adj_matrix = np.ascontiguousarray(np.asarray(adj_matrix, dtype=np.float64))
        dim = self.adj_matrix.shape[0]
        assert self.adj_matrix.shape == (dim, dim) and len(distributions) == dim and len(queue_list) == dim
        for d in distributions:
            if d[0] != "normal":
                raise NotImplementedError(f"distribution {d[0]!r}: the deterministic core implements 'normal' only")
        # np.float32 parameters (matrix_sim_process.py:72-74) widen exactly, like `vals * scale + loc` in scipy
        self.loc = np.ascontiguousarray([float(d[1]) for d in distributions], dtype=np.float64)
        self.scale = np.ascontiguousarray([float(d[2]) for d in distributions], dtype=np.float64)
        if (self.scale < 0).any():
            raise ValueError("Domain error in arguments. The `scale` parameter must be positive for all distributions")
        self.queue_list = np.ascontiguousarray(queue_list, dtype=np.int32)
        self.distributions = distributions
        self.generate_log = generate_log
        self.logging_mode = logging_mode
        self.max_sim_time = max_sim_time
        self.max_events = int(max_events)
        self.verbose = verbose
        self.log_file = (log_path + ("simulation.log" if log_name is None else log_name)) if generate_log else None
        if self.log_file is not None:
            os.makedirs(os.path.dirname(self.log_file) or ".", exist_ok=True)
            open(self.log_file, "w").close()          # simulation_v3.py:337-341: the old log is emptied on construction
        self.music_log = np.zeros(0, dtype=EVENT_DTYPE)
        self.stop_reason = None

    def _run_once(self, seed, number_of_customers):
        lib = _lib.load()
        dim = self.adj_matrix.shape[0]
        name, key, pos, has_gauss, gauss = np.random.get_state()
        assert name == "MT19937"
        cap = 4 * self.max_events + 4 * dim + 64 if self.max_events > 0 else 1 << 16
        while True:
            k = np.ascontiguousarray(key, dtype=np.uint32).copy()
            c_pos, c_has, c_gauss = ctypes.c_int(int(pos)), ctypes.c_int(int(has_gauss)), ctypes.c_double(float(gauss))
            out = np.empty(cap, dtype=EVENT_DTYPE)        # only out[:n_out] is returned
            n_out, reason = ctypes.c_int64(0), ctypes.c_int(0)
            rc = lib.gdm_des_run(self.adj_matrix.ctypes.data, dim, self.loc.ctypes.data, self.scale.ctypes.data,
                                 self.queue_list.ctypes.data, int(seed), int(number_of_customers), self.max_events,
                                 k.ctypes.data, ctypes.byref(c_pos), ctypes.byref(c_has), ctypes.byref(c_gauss),
                                 out.ctypes.data, cap, ctypes.byref(n_out), ctypes.byref(reason))
            if rc == -3 and n_out.value > cap:        # GDM_EWORKSPACE: retry from the ORIGINAL generator state
                cap = int(n_out.value) + 64
                continue
            if rc != 0:
                msg = lib.gdm_last_error().decode(errors="replace")
                raise ValueError(msg)                 # the reference raises ValueError / KeyError in these cases
            np.random.set_state((name, k, c_pos.value, c_has.value, c_gauss.value))
            return out[:n_out.value], reason.value

    def run(self, number_of_customers=50, use_next_available_server=False):
        logs = []
        for seed in self.seeds:
            log, reason = self._run_once(seed, number_of_customers)
            logs.append(log)
            self.stop_reason = STOP_REASONS[reason]
        self.music_log = np.concatenate(logs) if logs else np.zeros(0, dtype=EVENT_DTYPE)
        if self.log_file is not None:
            write_music_log(self.music_log, self.log_file)
        return self.music_log


def write_music_log(records, path, kind=None):
    """EVENT_DTYPE records (``Sim.music_log``, ``sample_log`` of a BatchLog) -> the 'Music' log file the reference's
    ``logging.info`` writes (``logs/simulation.log``): ``INFO:root:<repr of the value> - <id> - <node> - <kind>``.
    ``kind``: the net's (dim) row of NODE_KINDS indices; the ``processing`` record of a 'queue' or 'branch' node is then
    written as the reference writes it, the int ``0`` (ScheduleDeparture's ``service_time = 0``), not ``0.0``."""
    timeless = None if kind is None else np.asarray(kind).reshape(-1) >= NODE_KINDS.index("queue")
    with open(path, "w") as f:
        for v, eid, node, k in records:
            text = "0" if timeless is not None and k == PROCESSING and timeless[int(node)] else repr(float(v))
            f.write(f"INFO:root:{text} - {int(eid)} - {int(node)} - {KIND_NAMES[k]}\n")


def run_spec(spec, max_events=200000, generate_log=False, log_path="logs/"):
    """The DES call of the bridges for one ``matrix_sim_process.DesSpec``: returns (music_log, stop_reason)."""
    sim = Sim(spec.sim_matrix, spec.distributions, spec.queue_list, seeds=spec.seeds, log_path=log_path,
              generate_log=generate_log, animation=False, record_history=False, logging_mode='Music',
              max_sim_time=spec.max_sim_time, max_events=max_events)
    sim.run(number_of_customers=spec.num_customers)
    return sim.music_log, sim.stop_reason


# ---- batched simulation: every sample from its own generator state -----------------------------------------------------
BatchLog = collections.namedtuple("BatchLog", "value event_id node kind rec_ptr n_records stop_reason mt_key mt_pos "
                                              "has_gauss gauss")
BatchLog.__doc__ = """Records of B simulations in the CSR layout of ``ops.des_log_to_roll`` / ``ops.des_log_to_notes``
(sample b: [rec_ptr[b], rec_ptr[b+1])), n_records (B), stop_reason (B, index into STOP_REASONS) and the generator
states after the runs (mt_key (B,624) uint32 -- int32 bit patterns on a device --, mt_pos, has_gauss, gauss (B))."""


def pack_states(states, b):
    """B ``np.random.get_state()`` tuples (or one for all; None: the current global state) -> (key (B,624) uint32, pos
    (B) int32, has_gauss (B) int32, gauss (B) float64)."""
    if states is None:
        states = np.random.get_state()
    if isinstance(states, tuple) and len(states) == 5 and isinstance(states[0], str):
        states = [states] * b
    if len(states) != b:
        raise ValueError(f"run_batch: {len(states)} generator states for {b} samples")
    for st in states:
        if st[0] != "MT19937":
            raise ValueError("run_batch: generator states must be numpy legacy MT19937 states (np.random.get_state())")
    key = np.ascontiguousarray([np.asarray(st[1], dtype=np.uint32) for st in states], dtype=np.uint32).reshape(b, 624)
    pos = np.ascontiguousarray([int(st[2]) for st in states], dtype=np.int32)
    has = np.ascontiguousarray([int(st[3]) for st in states], dtype=np.int32)
    gauss = np.ascontiguousarray([float(st[4]) for st in states], dtype=np.float64)
    return key, pos, has, gauss


def state_of(log, b):
    """Sample b's generator state after the run, as ``np.random.set_state`` takes it."""
    key = np.asarray(log.mt_key[b].cpu() if hasattr(log.mt_key, "cpu") else log.mt_key[b])
    return ("MT19937", key.view(np.uint32).copy(), int(log.mt_pos[b]), int(log.has_gauss[b]), float(log.gauss[b]))


def sample_log(log, b):
    """Sample b's records of a host BatchLog as an EVENT_DTYPE array (what ``Sim.music_log`` holds)."""
    lo, hi = int(log.rec_ptr[b]), int(log.rec_ptr[b + 1])
    out = np.empty(hi - lo, dtype=EVENT_DTYPE)
    for name in ("value", "event_id", "node", "kind"):
        out[name] = np.asarray(getattr(log, name)[lo:hi])
    return out


_HostInputs = collections.namedtuple("_HostInputs", "b dim adj state max_queue_cap policy head arrays")


def _host_inputs(who, adj, loc, scale, queue_cap, seed, customers, states, max_queue_cap, math, max_events, kind, net):
    """What both host runners do with their inputs: the arrays as the C entries read them, the generator states
    ``state`` = (key, pos, has_gauss, gauss) as writable arrays, ``max_queue_cap`` (None: the largest capacity), the
    entry's ``policy`` suffix ("", "_dist", "_net"), and ``head``, the entry's arguments up to ``max_events``, which
    point into ``arrays``."""
    if net and kind is None:
        raise ValueError(f"{who}: net=True needs kind")
    adj = np.ascontiguousarray(adj, dtype=np.float64)
    b, dim = adj.shape[0], adj.shape[1]
    assert adj.shape == (b, dim, dim), adj.shape
    loc = np.ascontiguousarray(loc, dtype=np.float64).reshape(b, dim)
    scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(b, dim)
    queue_cap = np.ascontiguousarray(queue_cap, dtype=np.int32).reshape(b, dim)
    seed = np.ascontiguousarray(seed, dtype=np.int64).reshape(b)
    customers = np.ascontiguousarray(customers, dtype=np.int64).reshape(b)
    state = tuple(np.array(a) for a in pack_states(states, b))
    if max_queue_cap is None:
        max_queue_cap = max(1, int(queue_cap.max()))
    kinds = () if kind is None else (np.ascontiguousarray(kind, dtype=np.int32).reshape(b, dim),)
    arrays = (adj, loc, scale, *kinds, queue_cap, seed, customers)
    head = (adj.ctypes.data, b, dim, *(a.ctypes.data for a in arrays[1:]), int(max_queue_cap), int(math),
            int(max_events))
    policy = "" if kind is None else "_net" if net else "_dist"
    return _HostInputs(b, dim, adj, state, int(max_queue_cap), policy, head, arrays)


def run_batch_host(adj, loc, scale, queue_cap, seed, customers, states=None, *, math=1, max_events=200000,
                   max_records=5001, max_queue_cap=None, kind=None, net=False):
    """``gdm_des_run_batch_host`` on numpy arrays: adj (B,dim,dim), loc, scale, queue_cap (B,dim), seed, customers (B).
    math 0 = libm (the reference's bits), 1 = portable (the device's bits).  max_records 0 = no cap.  -> BatchLog of
    numpy arrays; the record arrays are cut to rec_ptr[B].  ``kind`` (B,dim), the index into DIST_KINDS per node:
    ``gdm_des_run_batch_dist_host``; None: every node is normal.  ``net=True`` (with ``kind``, the index into NODE_KINDS):
    ``gdm_des_run_batch_net_host``, which also takes 'queue' and 'branch' nodes."""
    x = _host_inputs("run_batch_host", adj, loc, scale, queue_cap, seed, customers, states, max_queue_cap, math,
                     max_events, kind, net)
    b, dim, (key, pos, has, gauss) = x.b, x.dim, x.state
    max_events, max_records = int(max_events), int(max_records)
    name = f"gdm_des_run_batch{x.policy}_host"
    entry = getattr(_lib.load(), name)
    per = 4 * max_events + 4 * dim + 64                    # at most four records per processed event
    cap = b * (min(per, max_records) if max_records > 0 else per)
    while True:
        value, eid = np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.int64)
        node, rkind = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        rec_ptr, n_rec, stop = np.zeros(b + 1, dtype=np.int64), np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int32)
        k, p, h, g = key.copy(), pos.copy(), has.copy(), gauss.copy()
        rc = entry(*x.head, max_records, k.ctypes.data, p.ctypes.data, h.ctypes.data, g.ctypes.data, value.ctypes.data,
                   eid.ctypes.data, node.ctypes.data, rkind.ctypes.data, cap, rec_ptr.ctypes.data, n_rec.ctypes.data,
                   stop.ctypes.data)
        if rc == -3 and int(rec_ptr[-1]) > cap:            # GDM_EWORKSPACE: again from the ORIGINAL generator states
            cap = int(rec_ptr[-1])
            continue
        _lib.check(rc, name)
        n = int(rec_ptr[-1])
        return BatchLog(value[:n], eid[:n], node[:n], rkind[:n], rec_ptr, n_rec, stop, k, p, h, g)


def _one_seed(sp, name):
    if np.asarray(sp.seeds).size != 1:
        raise ValueError(f"{name}: one seed (one run) per spec")


def _normal_row(sp):
    """``dist_row`` of a spec for the entries without kinds: every node 'normal'."""
    if any(d[0] != "normal" for d in sp.distributions):
        raise NotImplementedError("run_batch: the deterministic core implements 'normal' distributions only")
    _one_seed(sp, "run_batch")
    return dist_row(sp.distributions)


def spec_arrays(specs):
    """[DesSpec] of one size -> (adj, loc, scale, queue_cap, seed, customers) numpy arrays with a leading B."""
    adj, _kind, *rest = _spec_arrays(specs, "run_batch", _normal_row)
    return (adj, *rest)


DIST_KINDS = ("normal", "exponential", "uniform")     # GDM_DES_DIST_*: the index is the kind


NODE_KINDS = DIST_KINDS + ("queue", "branch")         # the entries with node kinds (_net) take these as well


def dist_row(distributions, who="dist_arrays", kinds=DIST_KINDS):
    """One spec's ``distributions`` -> (kind, loc, scale) lists: ``['normal', loc, s]`` and ``['uniform', loc, s]`` as
    written, ``['exponential', s]`` as loc 0, scale s (scipy's ``expon(scale=s)``).  NotImplementedError names any
    other kind.  ``kinds=NODE_KINDS``: ``['queue']`` and ``['branch']`` too, as loc 0, scale 0."""
    kind, loc, scale = [], [], []
    for d in distributions:
        if d[0] not in kinds:
            raise NotImplementedError(f"{who}: distribution {d[0]!r} (the statistics entries implement "
                                      f"{', '.join(kinds)})")
        kind.append(kinds.index(d[0]))
        timeless = d[0] in ("queue", "branch")
        loc.append(0.0 if d[0] == "exponential" or timeless else float(d[1]))
        scale.append(0.0 if timeless else float(d[1]) if d[0] == "exponential" else float(d[2]))
    return kind, loc, scale


def _spec_arrays(specs, name, row):
    """The arrays of ``spec_arrays`` and ``dist_arrays``; ``name`` heads the messages, ``row`` checks a spec of the
    right size and returns its ``dist_row``."""
    if len(specs) == 0:
        raise ValueError(f"{name}: no specs")
    dim = np.asarray(specs[0].sim_matrix).shape[0]
    rows = []
    for sp in specs:
        if np.asarray(sp.sim_matrix).shape != (dim, dim) or len(sp.distributions) != dim or len(sp.queue_list) != dim:
            raise ValueError(f"{name}: every spec of a batch must have the same number of nodes")
        rows.append(row(sp))
    adj = np.ascontiguousarray([np.asarray(sp.sim_matrix, dtype=np.float64) for sp in specs])
    kind = np.ascontiguousarray([r[0] for r in rows], dtype=np.int32)
    loc = np.ascontiguousarray([r[1] for r in rows], dtype=np.float64)
    scale = np.ascontiguousarray([r[2] for r in rows], dtype=np.float64)
    qcap = np.ascontiguousarray([list(sp.queue_list) for sp in specs], dtype=np.int32)
    seed = np.ascontiguousarray([int(np.asarray(sp.seeds).reshape(-1)[0]) for sp in specs], dtype=np.int64)
    customers = np.ascontiguousarray([int(sp.num_customers) for sp in specs], dtype=np.int64)
    return adj, kind, loc, scale, qcap, seed, customers


def dist_arrays(specs, who="run_stats", kinds=DIST_KINDS):
    """``spec_arrays`` for specs whose nodes may be any of DIST_KINDS -> (adj, kind, loc, scale, queue_cap, seed,
    customers) numpy arrays with a leading B; kind (B,dim) int32, the index into DIST_KINDS."""
    def row(sp):
        _one_seed(sp, "run_stats")
        return dist_row(sp.distributions, who, kinds)

    return _spec_arrays(specs, "run_stats", row)


def net_arrays(specs, who="net_arrays"):
    """``dist_arrays`` for specs whose nodes may be any of NODE_KINDS: ``['queue']`` and ``['branch']`` get kind 3 and 4,
    loc 0 and scale 0 (neither is read).  For the entries taken with ``net=True``."""
    return dist_arrays(specs, who, NODE_KINDS)


def _device_inputs(who, adj, loc, scale, queue_cap, seed, customers, states, device, max_queue_cap, kind, net):
    """The upload of both device runners: numpy arrays go to ``device``, device tensors stay where they are; generator
    states as ``pack_states`` takes them, or the four tensors (mt_key (B,624) i32, mt_pos, has_gauss (B) i32, gauss (B)
    f64) already on the device (``ops.des_draws``), updated in place like every state the kernel is given.  -> (the
    tensors in the order the ops wrappers take them, the four state tensors among them, max_queue_cap)."""
    if net and kind is None:
        raise ValueError(f"{who}: net=True needs kind")
    import torch
    dev = torch.device(device)

    def up(a, dt):
        if torch.is_tensor(a):
            return a.to(device=dev, dtype=dt).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()

    b = adj.shape[0]
    if max_queue_cap is None:
        if torch.is_tensor(queue_cap):
            raise ValueError(f"{who}: pass max_queue_cap with a device queue_cap (it sizes the workspace)")
        max_queue_cap = max(1, int(np.asarray(queue_cap).max()))
    if isinstance(states, (tuple, list)) and len(states) == 4 and torch.is_tensor(states[0]):
        state = tuple(up(t, dt) for t, dt in zip(states, (torch.int32, torch.int32, torch.int32, torch.float64)))
    else:
        key, pos, has, gauss = pack_states(states, b)
        state = (up(key.view(np.int32), torch.int32), up(pos, torch.int32), up(has, torch.int32),
                 up(gauss, torch.float64))
    args = (up(adj, torch.float64), up(loc, torch.float64), up(scale, torch.float64),
            *(() if kind is None else (up(kind, torch.int32),)), up(queue_cap, torch.int32), up(seed, torch.int64),
            up(customers, torch.int64), *state)
    return args, state, max_queue_cap


def run_batch_device(adj, loc, scale, queue_cap, seed, customers, states=None, *, device, max_events=200000,
                     max_records=5001, max_queue_cap=None, workspace_tensor=None, kind=None, net=False):
    """``gdm_des_run_batch``: the arrays of ``run_batch_host`` (numpy, or device tensors that stay where they are --
    ``adj`` straight from ``ops.des_routing``) -> BatchLog of device tensors.  Nothing is read back.  ``kind`` as in
    ``run_batch_host``: ``gdm_des_run_batch_dist``, the kernel that draws normal, exponential and uniform nodes;
    ``net=True``: ``gdm_des_run_batch_net``, the kernel that also takes 'queue' and 'branch' nodes."""
    from . import ops
    args, state, max_queue_cap = _device_inputs("run_batch_device", adj, loc, scale, queue_cap, seed, customers, states,
                                                device, max_queue_cap, kind, net)
    kw = dict(max_queue_cap=max_queue_cap, max_events=max_events, max_records=max_records,
              workspace_tensor=workspace_tensor)
    if kind is None:
        out = ops.des_run_batch(*args, **kw)
    else:
        out = (ops.des_run_batch_net if net else ops.des_run_batch_dist)(*args, **kw)
    return BatchLog(*out, *state)


def batch_log_to(log, device):
    """A host BatchLog -> BatchLog of tensors on ``device`` (uint32 travels as int32 bit patterns, as the kernel's)."""
    import torch
    dev = torch.device(device)
    return BatchLog(*(torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)
                      for a in log))


def run_batch_auto(adj, loc, scale, queue_cap, seed, customers, states, *, device, min_device_b, max_events=200000,
                   max_records=5001, max_queue_cap=None):
    """The simulator choice of "des_batch" (arrays: numpy, or device tensors as ``run_batch_device`` takes them): the
    kernel from ``min_device_b`` samples on if it holds ``dim`` nodes, else the host mirror with portable math (the
    same bits; the launch costs 8-10 ms however small the batch is), its log uploaded once -> BatchLog of tensors on
    ``device``.  device=None: the host mirror's BatchLog of numpy arrays."""
    from . import ops
    if device is not None and adj.shape[0] >= min_device_b and adj.shape[1] <= ops.DES_BATCH_MAX_DIM:
        return run_batch_device(adj, loc, scale, queue_cap, seed, customers, states, device=device,
                                max_events=max_events, max_records=max_records, max_queue_cap=max_queue_cap)
    adj, loc, scale, queue_cap = (a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in (adj, loc, scale, queue_cap))
    host = run_batch_host(adj, loc, scale, queue_cap, seed, customers, states, math=1, max_events=max_events,
                          max_records=max_records)
    return host if device is None else batch_log_to(host, device)


def raise_for_stop(stop_reasons, who, noun):
    """ValueError for the first simulation of a batch that stopped with DES_STOP_ERROR or DES_STOP_BUDGET."""
    from . import ops
    for i, reason in enumerate(np.asarray(stop_reasons).tolist()):
        if reason in (ops.DES_STOP_ERROR, ops.DES_STOP_BUDGET):
            raise ValueError(f"{who}: the simulation of {noun} {i} stopped with {STOP_REASONS[reason]!r} (a node without "
                             "destination, a customer routed to a source, or a service distribution that never turns "
                             "positive; the reference raises or never returns)")


def run_batch(specs, *, device=None, max_events=200000, max_records=5001, states=None):
    """B ``matrix_sim_process.DesSpec`` of one size, each simulated from its own generator state (``states``: B
    ``np.random.get_state()`` tuples, or one for all; None: numpy's current global state -- which is left untouched).
    device=None: the host mirror with portable math (``gdm_des_run_batch_host``, math=1) -> BatchLog of numpy arrays;
    a HIP device: the kernel (``gdm_des_run_batch``) -> BatchLog of device tensors, bit-identical to the host's."""
    arrays = spec_arrays(specs)
    if device is None:
        return run_batch_host(*arrays, states, math=1, max_events=max_events, max_records=max_records)
    return run_batch_device(*arrays, states, device=device, max_events=max_events, max_records=max_records)


def run_batch_dist(specs, *, device=None, math=1, max_events=200000, max_records=5001, states=None):
    """``run_batch`` for specs whose nodes may be any of DIST_KINDS (``dist_arrays``) -> BatchLog, the log whose
    statistics ``run_stats`` returns.  The entries with kinds (``gdm_des_run_batch_dist[_host]``) run only when some
    node is not normal.  ``math`` is the host mirror's (device=None): 0 = libm, the reference's bits, 1 = portable, the
    device's.  The consumers of a BatchLog (``log_to_notes``, ``log_to_rolls``, ``ops.des_log_to_notes_pc``,
    ``simlog_to_vid.log_tracks``) take it as it is; ``write_music_log(sample_log(log, b), path)`` writes sample b as
    the reference's ``logs/simulation.log``.  Nodes may also be 'queue' or 'branch' (NODE_KINDS): then, and only then,
    the entries ``gdm_des_run_batch_net[_host]`` run; pass the spec's ``kind`` row to ``write_music_log``."""
    adj, kind, *rest = net_arrays(specs, "run_stats")
    kw = dict(max_events=max_events, max_records=max_records, kind=kind if kind.any() else None,   # all normal: as ever
              net=bool((kind >= len(DIST_KINDS)).any()))
    if device is None:
        return run_batch_host(adj, *rest, states, math=math, **kw)
    return run_batch_device(adj, *rest, states, device=device, **kw)


# ---- batched statistics: the same runs without a log ---------------------------------------------------------------------
STATS_NODE_FIELDS = ("served", "reneges", "generated", "max_queue", "time_in_service", "time_in_queue", "queue_area",
                     "arrival_time")
STATS_SAMPLE_FIELDS = ("clock", "end_time", "total_customers", "events", "n_records", "stop_reason")
BatchStats = collections.namedtuple("BatchStats", STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS +
                                    ("queue_time", "is_source", "mt_key", "mt_pos", "has_gauss", "gauss"))
BatchStats.__doc__ = """Per-node accumulators of B simulations (``gdm_des_stats_batch[_host]``, include/gdm.h): (B,dim)
served, reneges, generated (int64), max_queue (int32), time_in_service, time_in_queue, queue_area, arrival_time
(float64); (B) clock, end_time (float64), total_customers, events, n_records (int64), stop_reason (int32); queue_time
(B,dim,max_queue_cap+1) float64 or None; is_source (B,dim) bool; the generator states after the runs as in BatchLog."""
_STATS_DTYPES = dict(served=np.int64, reneges=np.int64, generated=np.int64, max_queue=np.int32,
                     time_in_service=np.float64, time_in_queue=np.float64, queue_area=np.float64,
                     arrival_time=np.float64, clock=np.float64, end_time=np.float64, total_customers=np.int64,
                     events=np.int64, n_records=np.int64, stop_reason=np.int32)


def run_stats_host(adj, loc, scale, queue_cap, seed, customers, states=None, *, math=1, max_events=200000,
                   max_queue_cap=None, histogram=False, kind=None, net=False):
    """``gdm_des_stats_batch_host`` on the numpy arrays of ``run_batch_host``: the same runs, no records -> BatchStats
    of numpy arrays.  math 0 = libm (the reference's bits), 1 = portable (the device's bits).  ``kind`` (B,dim), the
    index into DIST_KINDS per node: ``gdm_des_stats_batch_dist_host``; None: every node is normal.  ``net=True`` (with
    ``kind``, the index into NODE_KINDS): ``gdm_des_stats_batch_net_host``, which also takes 'queue' and 'branch' nodes."""
    x = _host_inputs("run_stats_host", adj, loc, scale, queue_cap, seed, customers, states, max_queue_cap, math,
                     max_events, kind, net)
    b, dim, (k, p, h, g) = x.b, x.dim, x.state
    out = {n: np.zeros((b, dim), dtype=_STATS_DTYPES[n]) for n in STATS_NODE_FIELDS}
    out.update({n: np.zeros(b, dtype=_STATS_DTYPES[n]) for n in STATS_SAMPLE_FIELDS})
    hist = np.zeros((b, dim, x.max_queue_cap + 1), dtype=np.float64) if histogram else None
    name = f"gdm_des_stats_batch{x.policy}_host"
    rc = getattr(_lib.load(), name)(*x.head, k.ctypes.data, p.ctypes.data, h.ctypes.data, g.ctypes.data,
                                    *(out[n].ctypes.data for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS),
                                    hist.ctypes.data if histogram else None)
    _lib.check(rc, name)
    is_source = np.diagonal(x.adj, axis1=1, axis2=2) > 0
    return BatchStats(*(out[n] for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS), hist, is_source, k, p, h, g)


def run_stats_device(adj, loc, scale, queue_cap, seed, customers, states=None, *, device, max_events=200000,
                     max_queue_cap=None, histogram=False, workspace_tensor=None, kind=None, net=False):
    """``gdm_des_stats_batch``: the arrays of ``run_batch_device`` (numpy, or device tensors that stay where they are --
    ``adj`` straight from ``ops.des_routing``) -> BatchStats of device tensors, bit-identical to
    ``run_stats_host(math=1)``.  Nothing is read back.  ``kind`` as in ``run_stats_host``: ``gdm_des_stats_batch_dist``,
    the kernel that draws normal, exponential and uniform nodes; ``net=True``: ``gdm_des_stats_batch_net``, the kernel
    that also takes 'queue' and 'branch' nodes."""
    import torch
    from . import ops
    args, state, max_queue_cap = _device_inputs("run_stats_device", adj, loc, scale, queue_cap, seed, customers, states,
                                                device, max_queue_cap, kind, net)
    kw = dict(max_queue_cap=max_queue_cap, max_events=max_events, histogram=histogram, workspace_tensor=workspace_tensor)
    if kind is None:
        out = ops.des_run_stats(*args, **kw)
    else:
        out = (ops.des_run_stats_net if net else ops.des_run_stats_dist)(*args, **kw)
    is_source = torch.diagonal(args[0], dim1=1, dim2=2) > 0
    return BatchStats(*(out[n] for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS), out["queue_time"], is_source, *state)


def run_stats(specs, *, device=None, max_events=200000, states=None, histogram=False):
    """``run_batch`` without a log: B ``DesSpec`` of one size, each from its own generator state -> BatchStats (numpy
    arrays from the host mirror with portable math for device=None, device tensors with the same bits otherwise).
    Nodes may be any of NODE_KINDS (``net_arrays``); the entries with kinds run only when some node is not normal, those
    with node kinds (``gdm_des_stats_batch_net[_host]``) only when some node is 'queue' or 'branch'."""
    adj, kind, *rest = net_arrays(specs, "run_stats")
    kw = dict(max_events=max_events, histogram=histogram, kind=kind if kind.any() else None,   # all normal: as ever
              net=bool((kind >= len(DIST_KINDS)).any()))
    if device is None:
        return run_stats_host(adj, *rest, states, math=1, **kw)
    return run_stats_device(adj, *rest, states, device=device, **kw)


# ---- snapshots: the statistics at S customer counts of ONE run -------------------------------------------------------------
StatsSnapshots = collections.namedtuple("StatsSnapshots", "snaps stop checkpoints mt_key mt_pos has_gauss gauss")
StatsSnapshots.__doc__ = """The statistics of B runs at S customer counts each (``gdm_des_stats_batch_snap_host``):
``snaps``, a BatchStats whose per-node arrays are (B,S,dim), per-sample arrays (B,S) and ``queue_time``
(B,S,dim,max_queue_cap+1) or None (``is_source`` (B,dim) and the generator states, (B), are the run's); ``stop`` (B,S)
int32, the stop reason of every snapshot (``snaps.stop_reason``); ``checkpoints`` (B,S) int64; and the generator states
after the whole run as in BatchStats.  Snapshot s of sample b is what the statistics run returns for that sample with
``checkpoints[b, s]`` customers -- bit for bit; the host mirror makes the run to the last checkpoint once, the device
makes the S runs side by side (``run_stats_snapshots_device``).  ``snapshot`` and ``window`` cut BatchStats out of it,
of numpy arrays or of device tensors alike."""
_ADDITIVE = ("served", "reneges", "generated", "time_in_service", "time_in_queue", "queue_area", "arrival_time",
             "clock", "end_time", "events", "n_records", "queue_time")


def _checkpoints(who, checkpoints, b):
    """(S,) or (B,S) customer counts -> a contiguous (B,S) int64 array.  Only the shape is checked here: the entry
    refuses a row that is not strictly ascending from >= 1 by message."""
    cp = np.asarray(checkpoints)
    if cp.ndim == 1:
        cp = np.broadcast_to(cp, (b, cp.shape[0]))
    if cp.ndim != 2 or cp.shape[0] != b or cp.shape[1] < 1 or cp.dtype.kind not in "iu":
        raise ValueError(f"{who}: checkpoints must be (S,) or (B, S) integers, S >= 1")
    return np.ascontiguousarray(cp, dtype=np.int64)


def run_stats_snapshots_host(adj, loc, scale, queue_cap, seed, checkpoints, states=None, *, math=1, max_events=200000,
                             max_queue_cap=None, histogram=False, kind=None):
    """``gdm_des_stats_batch_snap_host`` on the numpy arrays of ``run_stats_host`` with ``checkpoints`` ((S,) or (B,S),
    every row strictly ascending from >= 1) in the place of ``customers``: every sample runs ONCE, to its last
    checkpoint -> StatsSnapshots of numpy arrays.  ``kind`` (B,dim) is the index into NODE_KINDS (the entry runs the
    policy with 'queue' and 'branch' nodes, the superset); None: every node is normal."""
    adj = np.ascontiguousarray(adj, dtype=np.float64)
    b, dim = adj.shape[0], adj.shape[1]
    cp = _checkpoints("run_stats_snapshots_host", checkpoints, b)
    s = cp.shape[1]
    if kind is None:
        kind = np.zeros((b, dim), dtype=np.int32)
    x = _host_inputs("run_stats_snapshots_host", adj, loc, scale, queue_cap, seed, cp[:, -1], states, max_queue_cap,
                     math, max_events, kind, True)
    k, p, h, g = x.state
    out = {n: np.zeros((b, s, dim), dtype=_STATS_DTYPES[n]) for n in STATS_NODE_FIELDS}
    out.update({n: np.zeros((b, s), dtype=_STATS_DTYPES[n]) for n in STATS_SAMPLE_FIELDS})
    hist = np.zeros((b, s, dim, x.max_queue_cap + 1), dtype=np.float64) if histogram else None
    name = "gdm_des_stats_batch_snap_host"
    # x.head ends in (customers, max_queue_cap, math, max_events): snap_customers and S take the place of the first
    rc = getattr(_lib.load(), name)(*x.head[:-4], cp.ctypes.data, s, *x.head[-3:], k.ctypes.data, p.ctypes.data,
                                    h.ctypes.data, g.ctypes.data,
                                    *(out[n].ctypes.data for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS),
                                    hist.ctypes.data if histogram else None)
    _lib.check(rc, name)
    is_source = np.diagonal(x.adj, axis1=1, axis2=2) > 0
    snaps = BatchStats(*(out[n] for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS), hist, is_source, k, p, h, g)
    return StatsSnapshots(snaps, out["stop_reason"], cp, k, p, h, g)


def run_stats_snapshots_device(adj, loc, scale, queue_cap, seed, checkpoints, states=None, *, device, max_events=200000,
                               max_queue_cap=None, histogram=False, workspace_tensor=None, kind=None):
    """``ops.des_run_stats_snap``, one launch of ``gdm_des_stats_batch_net`` on B * S rows: the arrays of
    ``run_stats_device`` with ``checkpoints`` ((S,) or (B,S)) in the place of ``customers`` -> StatsSnapshots of device
    tensors, bit-identical to ``run_stats_snapshots_host(math=1)``.  Nothing is read back.  Cost model: the device does
    NOT make the run once -- wave (b, s) runs sample b to ``checkpoints[b, s]`` customers and the B * S waves run side
    by side, so the work is the sum of every row (about twice the last entry for doubling checkpoints, S / 2 times for
    evenly spaced ones) and the time is that of the longest run while B * S waves fit on the chip (measured at dim 61:
    no cost up to 256 waves, 1.35 times one run at 1024, 3.5 times at 4096).  Memory: every input
    row is repeated S times on the device (``adj``: B * S * dim * dim doubles, 131 KB per wave at dim 128), so what
    bounds B * S in practice is device memory, well before the entry's own 2^20 rows.  Numpy ``checkpoints`` must be strictly ascending from >= 1 (ValueError); a device tensor (B,S) i64
    is taken as it is: the kernel cannot refuse a row, every wave runs to its own count and the generator states after
    the launch are those of the last column's runs.  ``kind`` (B,dim) indexes NODE_KINDS; None: every node is normal."""
    import torch
    from . import ops
    b, dim = adj.shape[0], adj.shape[1]
    if torch.is_tensor(checkpoints):
        cp = checkpoints
        if cp.dim() != 2 or cp.shape[0] != b or cp.shape[1] < 1 or cp.dtype != torch.int64:
            raise ValueError("run_stats_snapshots_device: device checkpoints must be a (B, S) int64 tensor, S >= 1")
    else:
        cp = _checkpoints("run_stats_snapshots_device", _checked_rows("run_stats_snapshots_device", checkpoints), b)
    if kind is None:
        kind = np.zeros((b, dim), dtype=np.int32)
    args, state, max_queue_cap = _device_inputs("run_stats_snapshots_device", adj, loc, scale, queue_cap, seed,
                                                cp[:, -1], states, device, max_queue_cap, kind, True)
    dev = args[0].device
    cp = (cp.to(dev) if torch.is_tensor(cp) else torch.from_numpy(cp).to(dev)).contiguous()
    # args: adj, loc, scale, kind, queue_cap, seed, customers, then the four states; the (B, S) rows take customers' place
    out = ops.des_run_stats_snap(*args[:6], cp, *args[7:], max_queue_cap=max_queue_cap, max_events=max_events,
                                 histogram=histogram, workspace_tensor=workspace_tensor)
    is_source = torch.diagonal(args[0], dim1=1, dim2=2) > 0
    snaps = BatchStats(*(out[n] for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS), out["queue_time"], is_source, *state)
    return StatsSnapshots(snaps, out["stop_reason"], cp, *state)


def _checked_rows(who, checkpoints):
    """The value check of the spec-level functions (the array-level ones leave it to the entries)."""
    cp = np.asarray(checkpoints, dtype=np.int64)
    if cp.ndim not in (1, 2) or cp.shape[-1] < 1 or (cp[..., 0] < 1).any() or (np.diff(cp, axis=-1) <= 0).any():
        raise ValueError(f"{who}: checkpoints must be strictly ascending customer counts >= 1")
    return cp


def run_stats_snapshots(specs, checkpoints, *, device=None, max_events=200000, states=None, histogram=False):
    """``run_stats`` at S customer counts of the same runs: B ``DesSpec`` of one size (their own ``num_customers`` is not
    used: a run ends at its last checkpoint), ``checkpoints`` (S,) for all or (B,S) -> StatsSnapshots: numpy arrays
    from the host mirror with portable math for device=None, which makes every run once; device tensors with the same
    bits otherwise (``run_stats_snapshots_device``: S runs per sample side by side, the work the sum of a row of
    ``checkpoints``).  Nodes may be any of NODE_KINDS.  Nothing falls back: with a device the kernel runs or it raises."""
    adj, kind, loc, scale, qcap, seed, _customers = net_arrays(specs, "run_stats_snapshots")
    cp = _checked_rows("run_stats_snapshots", checkpoints)
    return _snapshots(adj, loc, scale, qcap, seed, cp, states, device=device, math=1, max_events=max_events,
                      histogram=histogram, kind=kind)


def _snapshots(adj, loc, scale, queue_cap, seed, cp, states, *, device, math, **kw):
    """The snapshot run of the spec-level functions: the host mirror (``math``) for device=None, else the kernel."""
    if device is None:
        return run_stats_snapshots_host(adj, loc, scale, queue_cap, seed, cp, states, math=math, **kw)
    return run_stats_snapshots_device(adj, loc, scale, queue_cap, seed, cp, states, device=device, **kw)


def snapshot(snaps, s):
    """Snapshot ``s`` of a StatsSnapshots as a BatchStats -- the statistics run of ``checkpoints[:, s]`` customers --, so
    ``metrics`` takes it as it is."""
    st = snaps.snaps
    return BatchStats(*(getattr(st, n)[:, s] for n in STATS_NODE_FIELDS + STATS_SAMPLE_FIELDS),
                      None if st.queue_time is None else st.queue_time[:, s], st.is_source, *st[-4:])


def window(snaps, s0, s1):
    """The statistics of the interval between snapshots ``s0`` and ``s1`` (s0 None: from the empty start) as a
    BatchStats: the additive fields -- served, reneges, generated, n_records, events, the sums time_in_service,
    time_in_queue, arrival_time, queue_area and queue_time, clock and end_time -- are the differences; ``max_queue``,
    ``total_customers`` and ``stop_reason`` are those of ``s1`` (max_queue is the largest since the start of the run).
    ``metrics`` of a window divides by the window's length of ``clock``.  Edge effect: ``time_in_service`` is credited
    when a service STARTS (the reference's ScheduleDeparture, simulation_v3.py:606), so a window gains the whole service
    that starts in it and none of the one running at its start: its utilisation is off by at most one service time per
    node, relative to the window's length."""
    hi = snapshot(snaps, s1)
    if s0 is None:
        return hi
    lo = snapshot(snaps, s0)
    return hi._replace(**{n: getattr(hi, n) - getattr(lo, n) for n in _ADDITIVE if getattr(hi, n) is not None})


def _window_run(adj, loc, scale, queue_cap, seed, customers, states, *, warmup, device, math, max_events,
                histogram=False, kind=None, max_queue_cap=None):
    """What ``warmup=`` does in ``replicate`` and the sweeps: one run per sample with the checkpoints (warmup, customers),
    the window between them (on a device: two runs per sample side by side, ``warmup + customers`` of work)."""
    warmup, customers = int(warmup), np.asarray(customers, dtype=np.int64).reshape(-1)
    if not 1 <= warmup < customers.min():
        raise ValueError(f"warmup must be in 1 .. customers - 1, got {warmup}")
    cp = np.stack([np.full_like(customers, warmup), customers], axis=1)
    snaps = _snapshots(adj, loc, scale, queue_cap, seed, cp, states, device=device, math=math, max_events=max_events,
                       histogram=histogram, kind=kind, max_queue_cap=max_queue_cap)
    return window(snaps, 0, 1)


METRIC_NAMES = ("avg_time_at_server", "avg_queue_time", "server_utilizations", "max_queue_lengths", "renege_rate",
                "service_times", "arrival_times", "customers_served_per_server", "avg_queue_length",
                "avg_server_length")
TOTAL_NAMES = ("total_U", "total_L", "total_LQ", "total_W", "total_WQ")


def metrics(stats):
    """The quantities of the reference's ``Sim.calculate_metrics`` (752-801) from a BatchStats, after one read-back:
    dict of float64 numpy arrays under the reference's names -- METRIC_NAMES (B,dim), ``queue_length_probabilities``
    (B,dim,K+1) when the histogram exists, TOTAL_NAMES (B) with the reference's formulas as written (797-801: total_L
    counts the utilisations, total_W the queue times twice).  NaN where the reference has no entry: a server that
    served nobody (its dict comprehensions leave it out), a server quantity on a source and the other way round, and
    every per-time quantity where ``clock == 0`` (ZeroDivisionError upstream).  Totals are ``nansum``s."""
    def host(a):
        return None if a is None else np.asarray(a.cpu() if hasattr(a, "cpu") else a)

    st = BatchStats(*(host(a) for a in stats))
    f = np.float64
    server = ~st.is_source.astype(bool)
    busy = server & (st.served > 0)
    nan = np.full(st.served.shape, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        def per(num, den, where):
            return np.where(where, np.asarray(num, dtype=f) / np.asarray(den, dtype=f), nan)

        ticking = (st.clock != 0)[:, None]
        clock = st.clock[:, None]
        m = {
            "avg_time_at_server": per(st.time_in_service + st.time_in_queue, st.served, busy),
            "avg_queue_time": per(st.time_in_queue, st.served, busy),
            "server_utilizations": per(st.time_in_service, clock, server & ticking),
            "max_queue_lengths": np.where(server, st.max_queue.astype(f), nan),
            "renege_rate": per(st.reneges, st.served, busy),
            "service_times": per(st.time_in_service, st.served, busy),
            "arrival_times": per(st.arrival_time, st.generated, ~server & (st.generated > 0)),
            "customers_served_per_server": np.where(server, st.served.astype(f), nan),
            "avg_queue_length": per(st.queue_area, clock, server & ticking),
        }
        m["avg_server_length"] = m["avg_queue_length"] + m["server_utilizations"]
        if st.queue_time is not None:
            m["queue_length_probabilities"] = np.where((server & ticking)[:, :, None],
                                                       st.queue_time / clock[:, :, None], np.nan)
    per_time = np.where(st.clock != 0, 0.0, np.nan)
    u, lq = np.nansum(m["server_utilizations"], axis=1), np.nansum(m["avg_queue_length"], axis=1)
    w, wq = np.nansum(m["avg_time_at_server"], axis=1), np.nansum(m["avg_queue_time"], axis=1)
    m["total_U"] = u + per_time
    m["total_L"] = (lq + u) + per_time
    m["total_LQ"] = lq + per_time
    m["total_W"] = w + wq
    m["total_WQ"] = wq
    return m


Replications = collections.namedtuple("Replications", "stats metrics mean std sem n valid")
Replications.__doc__ = """``replicate``'s result: the BatchStats and ``metrics`` of the R runs, and per metric name the
``mean``, ``std`` (ddof 1), ``sem`` = std / sqrt(n) and ``n`` over the runs of ``valid`` (R) bool -- those that stopped
neither with an error nor on the draw budget -- that have a value (are not NaN) at that node."""


def replication_states(seeds):
    """The default global stream of replication r: ``np.random.RandomState([seeds[r], 1])``.  Array seeding
    (init_by_array), so it is neither ``RandomState(seeds[r])`` -- the stream the per-node seeds are drawn from -- nor
    any node's own stream."""
    return [np.random.RandomState([int(s), 1]).get_state() for s in seeds]


def _replication_inputs(who, spec, seeds, states):
    """R seeded runs of ONE net as a batch: ((adj, loc, scale, queue_cap, seed, customers, states), kind or None, net)."""
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    r = len(seeds)
    if r == 0:
        raise ValueError(f"{who}: no seeds")
    kinds, locs, scales = dist_row(spec.distributions, who, NODE_KINDS)
    net = any(k >= len(DIST_KINDS) for k in kinds)
    one = np.asarray(spec.sim_matrix, dtype=np.float64)
    dim = one.shape[0]
    adj = np.ascontiguousarray(np.broadcast_to(one, (r, dim, dim)))
    loc = np.tile(np.array(locs, dtype=np.float64), (r, 1))
    scale = np.tile(np.array(scales, dtype=np.float64), (r, 1))
    kind = np.tile(np.array(kinds, dtype=np.int32), (r, 1)) if any(kinds) else None
    qcap = np.tile(np.asarray(list(spec.queue_list), dtype=np.int32), (r, 1))
    customers = np.full(r, int(spec.num_customers), dtype=np.int64)
    if states is None:
        states = replication_states(seeds)
    return (adj, loc, scale, qcap, np.asarray(seeds, dtype=np.int64), customers, states), kind, net


def _valid_runs(stop_reason):
    from . import ops
    stop = np.asarray(stop_reason.cpu() if hasattr(stop_reason, "cpu") else stop_reason)
    return (stop != ops.DES_STOP_ERROR) & (stop != ops.DES_STOP_BUDGET)


def _over_runs(m, valid):
    """Per metric name: mean, std (ddof 1), sem and n over the runs of ``valid`` that have a value."""
    mean, std, sem, n = {}, {}, {}, {}
    for name, a in m.items():
        a = a[valid]
        have = ~np.isnan(a)
        n[name] = have.sum(axis=0)
        total = np.where(have, a, 0.0).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean[name] = np.where(n[name] > 0, total / n[name], np.nan)
            dev2 = np.where(have, (a - mean[name]) ** 2, 0.0).sum(axis=0)
            std[name] = np.where(n[name] > 1, np.sqrt(dev2 / (n[name] - 1)), np.nan)
            sem[name] = std[name] / np.sqrt(n[name])
    return mean, std, sem, n


def replicate(spec, seeds, *, device=None, max_events=200000, states=None, warmup=0):
    """R = len(seeds) seeded runs of ONE net (a ``DesSpec``; its own ``seeds`` are not used) in one batch, then
    ``metrics`` and their mean / std (ddof 1) / sem / n over the replications -> Replications.  Nodes may be any of
    NODE_KINDS.  ``states``: the R global
    generator states (default ``replication_states(seeds)``).  No interval is formed: sem and n are what one needs.
    ``warmup`` (customers, default 0: the whole run from the empty system): the statistics of the ``window`` between
    ``warmup`` and ``num_customers`` customers of the same runs (``run_stats_snapshots_host``; with a ``device``
    ``run_stats_snapshots_device``, the same bits from two runs per replication side by side)."""
    arrays, kind, net = _replication_inputs("replicate", spec, seeds, states)
    if warmup:
        stats = _window_run(*arrays, warmup=warmup, device=device, math=1, max_events=max_events, kind=kind)
    elif device is None:
        stats = run_stats_host(*arrays, math=1, max_events=max_events, kind=kind, net=net)
    else:
        stats = run_stats_device(*arrays, device=device, max_events=max_events, kind=kind, net=net)
    m = metrics(stats)
    valid = _valid_runs(stats.stop_reason)
    mean, std, sem, n = _over_runs(m, valid)
    return Replications(stats, m, mean, std, sem, n, valid)


Convergence = collections.namedtuple("Convergence", "snaps checkpoints mean sem n valid")
Convergence.__doc__ = """``convergence``'s result: the StatsSnapshots of the R runs, ``checkpoints`` (S,), and per metric name
``mean``, ``sem`` (std with ddof 1 / sqrt(n)) and ``n`` over the runs of ``valid`` (R,S) that have a value, stacked over the
checkpoints: (S,dim) for METRIC_NAMES, (S,) for TOTAL_NAMES -- a metric against run length with its error band."""


def convergence(spec, seeds, checkpoints, *, device=None, max_events=200000, states=None):
    """How the metrics of ONE net converge with run length: R = len(seeds) replications as in ``replicate``, ONE batch
    that runs to ``checkpoints[-1]`` customers (``spec.num_customers`` is not used) and leaves a snapshot at every entry
    of ``checkpoints`` (S,) -> Convergence.  Row s is what ``replicate`` returns for ``num_customers = checkpoints[s]``.
    device=None: the host mirror (portable math), every run made once, without the S - 1 shorter runs.  A ``device``:
    ONE launch of R * S waves in the place of S ``replicate`` launches -- the shorter runs ARE made, beside the longest
    one (sum(checkpoints) of work per replication), which costs no time while R * S waves fit on the chip."""
    cp = _checked_rows("convergence", checkpoints)
    if cp.ndim != 1:
        raise ValueError("convergence: checkpoints must be (S,)")
    (adj, loc, scale, qcap, seed, _customers, states), kind, _net = _replication_inputs("convergence", spec, seeds, states)
    snaps = _snapshots(adj, loc, scale, qcap, seed, cp, states, device=device, math=1, max_events=max_events, kind=kind)
    valid = _valid_runs(snaps.stop)
    rows = [_over_runs(metrics(snapshot(snaps, s)), valid[:, s]) for s in range(len(cp))]
    mean, sem, n = ({name: np.stack([row[i][name] for row in rows]) for name in rows[0][0]} for i in (0, 2, 3))
    return Convergence(snaps, cp, mean, sem, n, valid)


BatchMeans = collections.namedtuple("BatchMeans", "snaps checkpoints values mean sem n lag1")
BatchMeans.__doc__ = """``batch_means``'s result: the StatsSnapshots of the one run, its ``checkpoints``, and per metric name
``values`` (n_batches,dim) -- (n_batches,) for TOTAL_NAMES --, the metric in every batch; ``mean``, ``sem`` (std with ddof
1 / sqrt(n)) and ``n`` over the batches that have a value; and ``lag1``, the lag-1 autocorrelation of the batch values
(sum of (v[j] - mean)(v[j+1] - mean) over sum of (v[j] - mean)^2; NaN where a batch has no value or the values do not
vary): near 0 when the batches are long enough for the sem to mean what it says."""


def batch_means(spec, seed, *, n_batches, batch_customers, warmup=0, device=None, max_events=200000, state=None):
    """A confidence interval from ONE long run: ``warmup`` customers are left out, then ``n_batches`` consecutive
    windows of ``batch_customers`` customers each, the checkpoints warmup + j * batch_customers, j = 0 .. n_batches (with
    warmup 0 the first window starts at the empty system and j = 0 is no checkpoint) -> BatchMeans.  ``spec.num_customers``
    is not used; ``state``: the global generator state (default ``replication_states([seed])[0]``).  ValueError when the
    run ends before its last checkpoint (raise ``max_events``).  With a ``device`` the one run becomes one run per
    checkpoint, side by side (``run_stats_snapshots_device``): about n_batches / 2 times the work, the time of the longest."""
    from . import ops
    n_batches, batch_customers, warmup = int(n_batches), int(batch_customers), int(warmup)
    if n_batches < 2 or batch_customers < 1 or warmup < 0:
        raise ValueError("batch_means: n_batches >= 2, batch_customers >= 1, warmup >= 0")
    cp = np.array([warmup + j * batch_customers for j in range(0 if warmup else 1, n_batches + 1)], dtype=np.int64)
    (adj, loc, scale, qcap, sd, _customers, states), kind, _net = _replication_inputs(
        "batch_means", spec, [seed], None if state is None else [state])
    snaps = _snapshots(adj, loc, scale, qcap, sd, cp, states, device=device, math=1, max_events=max_events, kind=kind)
    stop = np.asarray(snaps.stop.cpu() if hasattr(snaps.stop, "cpu") else snaps.stop)
    if (stop != ops.DES_STOP_CUSTOMERS).any():
        raise ValueError(f"batch_means: the run ended with {STOP_REASONS[int(stop[0, -1])]!r} before its last checkpoint")
    first = 0 if warmup else -1                           # the snapshot a batch starts at, for batch 0
    per = [metrics(window(snaps, first + j if first + j >= 0 else None, first + j + 1)) for j in range(n_batches)]
    values = {name: np.concatenate([m[name] for m in per]) for name in per[0]}
    mean, _std, sem, n = _over_runs(values, np.ones(n_batches, dtype=bool))
    lag1 = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, v in values.items():
            d = v - v.mean(axis=0)
            lag1[name] = (d[:-1] * d[1:]).sum(axis=0) / (d * d).sum(axis=0)
    return BatchMeans(snaps, cp, values, mean, sem, n, lag1)


# ---- simulation beside theory: M/M/1/K -------------------------------------------------------------------------------
SWEEP_NAMES = ("blocked_fraction", "utilisation", "avg_queue_length", "avg_queue_time", "queue_length_probabilities")
Mm1kSweep = collections.namedtuple("Mm1kSweep", "lam mu queue_cap seeds stats values mean sem n theory z")
Mm1kSweep.__doc__ = """``mm1k_sweep``'s result for C configurations x R seeds: lam, mu, queue_cap (C); the BatchStats of
the C * R runs (configuration-major: run c * R + r); and per name of SWEEP_NAMES ``values`` (C, R) -- (C, R, K + 1), K =
max(queue_cap), for ``queue_length_probabilities``, NaN beyond a configuration's own capacity --, their ``mean``,
``sem`` (std with ddof 1 / sqrt(n)) and ``n`` over the runs that neither errored nor ran out of draws, the
``queueing_theory.mm1k`` value ``theory`` and ``z`` = (mean - theory) / sem (0 where both differences are 0)."""


def mm1k_spec(lam, mu, queue_cap, customers, seed=0):
    """The 2-node net source -> server with exponential inter-arrival (mean 1 / lam) and service (mean 1 / mu) times
    and ``queue_cap`` waiting places, as a ``DesSpec``."""
    from .matrix_sim_process import DesSpec
    adj = np.array([[1.0, 1.0], [0.0, 0.0]])
    return DesSpec(adj, [["exponential", 1.0 / float(lam)], ["exponential", 1.0 / float(mu)]],
                   [int(queue_cap), int(queue_cap)], np.array([int(seed)]), int(customers), 1.0, np.zeros(2), np.zeros(2))


def mm1k_sweep(lams, mus, queue_caps, seeds, *, customers, device=None, max_events=None, math=1, warmup=0):
    """Simulated M/M/1/K beside ``queueing_theory.mm1k``: configuration c = (lams[c], mus[c], queue_caps[c]), every
    configuration with every seed, ALL of them one batch (one launch on a device; ``math`` is the host mirror's).
    Replication r of every configuration starts from the global stream ``replication_states(seeds)[r]``.  Compared
    (SWEEP_NAMES), each a property of the server node:
      blocked_fraction            reneges / (served + reneges): the fraction of arrivals turned away  ~ p[K]
                                  (``metrics``' renege_rate, reneges / served, is the reference's other quantity)
      utilisation                 time_in_service / clock                                                ~ 1 - p[0]
      avg_queue_length            queue_area / clock                                                     ~ LQ
      avg_queue_time              time_in_queue / served                                                 ~ WQ
      queue_length_probabilities  queue_time / clock                                                     ~ (p0 + p1, p2, ..)
    -> Mm1kSweep.  max_events None: 4 * customers + 64, which no run reaches (an arrival and a departure per customer).
    ``warmup`` (customers, default 0): every quantity, and ``stats``, is that of the ``window`` between ``warmup`` and
    ``customers`` customers of the same runs, the empty-system start left out (with a ``device``: two runs per sample
    side by side in the one launch, the same bits)."""
    from . import ops, queueing_theory as qt
    lams, mus = np.asarray(lams, dtype=np.float64).reshape(-1), np.asarray(mus, dtype=np.float64).reshape(-1)
    caps = np.asarray(queue_caps, dtype=np.int64).reshape(-1)
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    c, r = len(lams), len(seeds)
    if c == 0 or r == 0 or len(mus) != c or len(caps) != c:
        raise ValueError("mm1k_sweep: lams, mus and queue_caps must have one entry per configuration, and seeds be given")
    if (caps < 1).any():
        raise ValueError("mm1k_sweep: queue_cap >= 1 (the simulator's rings hold at least one customer)")
    if max_events is None:
        max_events = 4 * int(customers) + 64
    specs = [mm1k_spec(lams[i], mus[i], caps[i], customers, s) for i in range(c) for s in seeds]
    states = replication_states(seeds) * c
    adj, kind, *rest = dist_arrays(specs)
    if warmup:
        stats = _window_run(adj, *rest, states, warmup=warmup, device=device, math=math, max_events=max_events,
                            histogram=True, kind=kind)
    elif device is None:
        stats = run_stats_host(adj, *rest, states, math=math, max_events=max_events, histogram=True, kind=kind)
    else:
        stats = run_stats_device(adj, *rest, states, device=device, max_events=max_events, histogram=True, kind=kind)
    m = metrics(stats)
    st = BatchStats(*(None if a is None else np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in stats))
    k = int(caps.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        blocked = st.reneges[:, 1] / (st.served[:, 1] + st.reneges[:, 1]).astype(np.float64)
    prob = m["queue_length_probabilities"][:, 1, :].copy()
    for i in range(c):
        prob[i * r:(i + 1) * r, caps[i] + 1:] = np.nan           # lengths the configuration cannot have
    values = {"blocked_fraction": blocked.reshape(c, r), "utilisation": m["server_utilizations"][:, 1].reshape(c, r),
              "avg_queue_length": m["avg_queue_length"][:, 1].reshape(c, r),
              "avg_queue_time": m["avg_queue_time"][:, 1].reshape(c, r), "queue_length_probabilities": prob.reshape(c, r, k + 1)}
    valid = ((st.stop_reason != ops.DES_STOP_ERROR) & (st.stop_reason != ops.DES_STOP_BUDGET)).reshape(c, r)
    theory = {n: np.full((c, k + 1) if n == "queue_length_probabilities" else (c,), np.nan) for n in SWEEP_NAMES}
    for i in range(c):
        t = qt.mm1k(lams[i], mus[i], caps[i])
        theory["blocked_fraction"][i], theory["utilisation"][i] = t["blocking"], t["utilisation"]
        theory["avg_queue_length"][i], theory["avg_queue_time"][i] = t["LQ"], t["WQ"]
        theory["queue_length_probabilities"][i, :caps[i] + 1] = t["queue_length_probabilities"]
    mean, sem, n, z = _sweep_summary(values, valid, theory)
    return Mm1kSweep(lams, mus, caps, np.asarray(seeds, dtype=np.int64), stats, values, mean, sem, n, theory, z)


def _sweep_summary(values, valid, theory):
    """Per name: mean, sem (std with ddof 1 / sqrt(n)) and n of ``values[name]`` (C, R[, K + 1]) over the runs of
    ``valid`` (C, R) that have a value, and z = (mean - theory) / sem (0 where the difference is 0)."""
    mean, sem, n, z = {}, {}, {}, {}
    for name, v in values.items():
        ok = valid if v.ndim == 2 else valid[:, :, None]
        have = ok & ~np.isnan(v)
        n[name] = have.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean[name] = np.where(n[name] > 0, np.where(have, v, 0.0).sum(axis=1) / n[name], np.nan)
            dev2 = np.where(have, (v - np.expand_dims(mean[name], 1)) ** 2, 0.0).sum(axis=1)
            sem[name] = np.where(n[name] > 1, np.sqrt(dev2 / (n[name] - 1)) / np.sqrt(n[name]), np.nan)
            d = mean[name] - theory[name]
            z[name] = np.where(d == 0, 0.0, d / sem[name])
    return mean, sem, n, z


# ---- simulation beside theory: M/M/c/N, a queue node in front of c servers -----------------------------------------------
MmckSweep = collections.namedtuple("MmckSweep", "c lam mu queue_cap seeds stats values mean sem n theory z")
MmckSweep.__doc__ = """``mmck_sweep``'s result: Mm1kSweep's fields (C configurations x R seeds, run c * R + r) with ``c`` (C),
the number of servers, in front; ``theory`` is ``queueing_theory.mmck(lam, mu, c, max(queue_cap, 1))`` and K =
max(max(queue_cap), 1).  Nets of different c have different sizes, so ``stats`` is a host BatchStats (numpy arrays,
whatever the device) with THREE node rows per run: the source, the queue node, and the c servers taken together (sums;
the largest ``max_queue``)."""


def mmck_spec(c, lam, mu, queue_cap, customers, seed=0):
    """The multi-server station as the reference builds it, as a ``DesSpec`` of c + 2 nodes: node 0 an exponential source
    (mean 1 / lam), node 1 a ``['queue']`` node with ``queue_cap`` places, nodes 2 .. c + 1 exponential servers (mean
    1 / mu) without a queue of their own (capacity 0), each a sink.  The queue node hands a customer to the first idle
    server and holds the next one back (a delayed departure) while all are busy: M/M/c/N, N = c + max(queue_cap, 1)."""
    from .matrix_sim_process import DesSpec
    c = int(c)
    if c < 1:
        raise ValueError("mmck_spec: c >= 1")
    dim = c + 2
    adj = np.zeros((dim, dim))
    adj[0, 0] = adj[0, 1] = 1.0
    adj[1, 2:] = 1.0
    dist = [["exponential", 1.0 / float(lam)], ["queue"]] + [["exponential", 1.0 / float(mu)] for _ in range(c)]
    return DesSpec(adj, dist, [0, int(queue_cap)] + [0] * c, np.array([int(seed)]), int(customers), 1.0, np.zeros(dim),
                   np.zeros(dim))


def mmck_sweep(cs, lams, mus, queue_caps, seeds, *, customers, device=None, max_events=None, math=1, warmup=0):
    """Simulated M/M/c/N beside ``queueing_theory.mmck``, shaped like ``mm1k_sweep``: configuration i = (cs[i], lams[i],
    mus[i], queue_caps[i]) on the net of ``mmck_spec``, every configuration with every seed from the global stream
    ``replication_states(seeds)[r]``.  Configurations of one c are one batch (one launch on a device: a batch has one
    dim); the result is in the order given.  Compared (SWEEP_NAMES), with N = c + max(queue_cap, 1):
      blocked_fraction            reneges / (served + reneges) at the queue node                          ~ p[N]
      utilisation                 the mean over the c servers of time_in_service / clock                  ~ sum min(n, c) p[n] / c
      avg_queue_length            queue_area / clock at the queue node (queue + delayed departure)        ~ LQ
      avg_queue_time              time_in_queue / served at the queue node (waits and delays)             ~ WQ
      queue_length_probabilities  queue_time / clock at the queue node                                    ~ (p[0] + .. + p[c], p[c + 1], ..)
    -> MmckSweep.  max_events None: 16 * customers + 64 (an arrival and two departures per customer, and a re-pop for
    every delayed departure that loses its tie).  ``warmup`` as in ``mm1k_sweep``."""
    from . import ops, queueing_theory as qt
    cs = np.asarray(cs, dtype=np.int64).reshape(-1)
    lams, mus = np.asarray(lams, dtype=np.float64).reshape(-1), np.asarray(mus, dtype=np.float64).reshape(-1)
    caps = np.asarray(queue_caps, dtype=np.int64).reshape(-1)
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    c, r = len(lams), len(seeds)
    if c == 0 or r == 0 or len(mus) != c or len(caps) != c or len(cs) != c:
        raise ValueError("mmck_sweep: cs, lams, mus and queue_caps must have one entry per configuration, and seeds be "
                         "given")
    if (caps < 0).any() or (cs < 1).any():
        raise ValueError("mmck_sweep: c >= 1 and queue_cap >= 0")
    if max_events is None:
        max_events = 16 * int(customers) + 64
    k = max(int(caps.max()), 1)
    rows = {name: [None] * c for name in ("blocked", "util", "lq", "wq", "prob", "valid") + BatchStats._fields}
    for servers in sorted(set(cs.tolist())):
        idx = [i for i in range(c) if cs[i] == servers]
        specs = [mmck_spec(servers, lams[i], mus[i], caps[i], customers, s) for i in idx for s in seeds]
        adj, kind, *rest = net_arrays(specs, "mmck_sweep")
        kw = dict(max_events=max_events, histogram=True, kind=kind, net=True, max_queue_cap=k)
        if warmup:
            stats = _window_run(adj, *rest, replication_states(seeds) * len(idx), warmup=warmup, device=device,
                                math=math, **{k_: v for k_, v in kw.items() if k_ != "net"})
        elif device is None:
            stats = run_stats_host(adj, *rest, replication_states(seeds) * len(idx), math=math, **kw)
        else:
            stats = run_stats_device(adj, *rest, replication_states(seeds) * len(idx), device=device, **kw)
        m = metrics(stats)
        st = BatchStats(*(None if a is None else np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in stats))
        with np.errstate(divide="ignore", invalid="ignore"):
            blocked = st.reneges[:, 1] / (st.served[:, 1] + st.reneges[:, 1]).astype(np.float64)
        valid = (st.stop_reason != ops.DES_STOP_ERROR) & (st.stop_reason != ops.DES_STOP_BUDGET)
        for j, i in enumerate(idx):
            sl = slice(j * r, (j + 1) * r)
            prob = m["queue_length_probabilities"][sl, 1, :].copy()
            prob[:, max(caps[i], 1) + 1:] = np.nan               # lengths the configuration cannot have
            rows["blocked"][i], rows["util"][i] = blocked[sl], m["server_utilizations"][sl, 2:].mean(axis=1)
            rows["lq"][i], rows["wq"][i] = m["avg_queue_length"][sl, 1], m["avg_queue_time"][sl, 1]
            rows["prob"][i], rows["valid"][i] = prob, valid[sl]
            for name in BatchStats._fields:                      # node rows: source, queue node, the servers together
                a = getattr(st, name)[sl]
                if name == "mt_key":
                    a = a.view(np.uint32)                        # (int32 bit patterns from a device)
                if name in STATS_NODE_FIELDS + ("queue_time", "is_source"):
                    rest = a[:, 2:].max(axis=1) if name in ("max_queue", "is_source") else a[:, 2:].sum(axis=1)
                    a = np.stack([a[:, 0], a[:, 1], rest], axis=1)
                rows[name][i] = a
    values = {"blocked_fraction": np.stack(rows["blocked"]), "utilisation": np.stack(rows["util"]),
              "avg_queue_length": np.stack(rows["lq"]), "avg_queue_time": np.stack(rows["wq"]),
              "queue_length_probabilities": np.stack(rows["prob"])}
    theory = {n: np.full((c, k + 1) if n == "queue_length_probabilities" else (c,), np.nan) for n in SWEEP_NAMES}
    for i in range(c):
        t = qt.mmck(lams[i], mus[i], cs[i], max(caps[i], 1))
        theory["blocked_fraction"][i], theory["utilisation"][i] = t["blocking"], t["utilisation"]
        theory["avg_queue_length"][i], theory["avg_queue_time"][i] = t["LQ"], t["WQ"]
        theory["queue_length_probabilities"][i, :max(caps[i], 1) + 1] = t["queue_length_probabilities"]
    mean, sem, n, z = _sweep_summary(values, np.stack(rows["valid"]), theory)
    stats = BatchStats(*(np.concatenate(rows[name]) for name in BatchStats._fields))
    return MmckSweep(cs, lams, mus, caps, np.asarray(seeds, dtype=np.int64), stats, values, mean, sem, n, theory, z)


# ---- the log customer by customer: per-visit and per-customer tables ---------------------------------------------------
VISIT_UNSERVED, VISIT_IN_SERVICE, VISIT_DEPARTED = 0, 1, 2                      # GDM_DES_VISIT_*
CUST_ABSENT, CUST_UNSERVED, CUST_IN_NET, CUST_EXITED = -1, 0, 1, 2              # GDM_DES_CUST_*
VISITS_ERECORD, VISITS_EPTR = 1, 2                                              # GDM_DES_VISITS_*
_VISIT_I32 = ("node", "n_departures", "outcome")
_VISIT_I64 = ("event_id", "rec_arrival", "rec_start", "rec_first_depart", "rec_depart", "prev_visit", "next_visit")
_VISIT_F64 = ("t_arrival", "t_start", "service", "t_first_depart", "t_depart")
_CUST_I32 = ("cust_n_visits", "cust_outcome")
_CUST_I64 = ("cust_first_visit", "cust_last_visit")
_CUST_F64 = ("cust_t_enter", "cust_t_exit", "cust_service_sum", "cust_wait_sum")
LogVisits = collections.namedtuple("LogVisits", _VISIT_I32 + _VISIT_I64 + _VISIT_F64 + ("visit_ptr",) + _CUST_I32 +
                                   _CUST_I64 + _CUST_F64 + ("cust_ptr", "status"))
LogVisits.__doc__ = """``log_visits``'s result (``gdm_des_log_visits_host``, include/gdm.h; numpy arrays).  One row per VISIT
-- a customer's stay at one node, opened by every ``arrival`` record --, sample b's at [visit_ptr[b], visit_ptr[b+1]),
every index relative to the sample (records to its first record, visits to its first visit), -1 / NaN = none:
``node``, ``n_departures``, ``outcome`` (int32; VISIT_DEPARTED: a departure was logged, VISIT_IN_SERVICE: started and no
departure, VISIT_UNSERVED: never started), ``event_id``, ``rec_arrival``, ``rec_start``, ``rec_first_depart``,
``rec_depart``, ``prev_visit``, ``next_visit`` (int64), ``t_arrival``, ``t_start``, ``service``, ``t_first_depart``,
``t_depart`` (float64, copies of log values: ``t_start`` is the value of the latest arrival or departure record before
the visit's ``processing`` record, ``t_depart`` that of its LAST departure record -- a 'queue' node's delayed departures
are several).  One row per CUSTOMER, sample b's at [cust_ptr[b], cust_ptr[b+1]), row = event id, 0 .. the largest id
seen: ``cust_n_visits`` (0: the id has no record), ``cust_outcome`` (int32; from the last visit: CUST_EXITED,
CUST_IN_NET, CUST_UNSERVED; CUST_ABSENT without records), ``cust_first_visit``, ``cust_last_visit`` (int64),
``cust_t_enter``, ``cust_t_exit`` (the last visit's ``t_depart`` when it departed), ``cust_service_sum`` and
``cust_wait_sum`` (float64: service and ``t_start - t_arrival`` summed over the started visits in visit order).
``status`` (B) int32: 0, VISITS_ERECORD or VISITS_EPTR; such a sample has no rows (``raise_for_visits``).
What a log cannot tell: an UNSERVED visit was turned away or was still waiting when the log ended; a queue node's
customer whose last logged departure was a delayed one reads as DEPARTED at that clock (at most one per queue node and
log); EXITED says that no later arrival was logged."""


def log_visits(log, *, dim):
    """The 'Music' logs of B runs over ``dim`` nodes, customer by customer -> LogVisits.  ``log``: a host BatchLog; a
    BatchLog of device tensors, which is read back once (there is no kernel: the walk runs on the host either way); or
    ONE EVENT_DTYPE record array (``Sim.music_log``, ``sample_log(...)``), walked as B = 1.  A sample the walk refuses
    has status != 0 and no rows; nothing is raised here (``raise_for_visits``)."""
    if isinstance(log, np.ndarray) and log.dtype == EVENT_DTYPE:
        cols = [log[name] for name in ("value", "event_id", "node", "kind")]
        rec_ptr = np.array([0, len(log)], dtype=np.int64)
    else:
        host = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (log.value, log.event_id, log.node, log.kind,
                                                                         log.rec_ptr)]
        cols, rec_ptr = host[:4], host[4]
    value, eid, node, kind = (np.ascontiguousarray(a, dtype=dt)
                              for a, dt in zip(cols, (np.float64, np.int64, np.int32, np.int32)))
    rec_ptr = np.ascontiguousarray(rec_ptr, dtype=np.int64)
    b = int(rec_ptr.shape[0]) - 1
    n = min(a.size for a in (value, eid, node, kind))
    entry = _lib.load().gdm_des_log_visits_host
    visit_ptr, cust_ptr = np.zeros(b + 1, dtype=np.int64), np.zeros(b + 1, dtype=np.int64)
    status = np.zeros(b, dtype=np.int32)
    nv = nc = 0
    while True:                                           # count, then fill
        tables = [np.zeros((len(names), cap), dtype=dt) for names, cap, dt in
                  ((_VISIT_I32, nv, np.int32), (_VISIT_I64, nv, np.int64), (_VISIT_F64, nv, np.float64),
                   (_CUST_I32, nc, np.int32), (_CUST_I64, nc, np.int64), (_CUST_F64, nc, np.float64))]
        ptrs = [t.ctypes.data if nv or nc else None for t in tables]
        rc = entry(value.ctypes.data, eid.ctypes.data, node.ctypes.data, kind.ctypes.data, rec_ptr.ctypes.data, n, b,
                   int(dim), visit_ptr.ctypes.data, cust_ptr.ctypes.data, status.ctypes.data, *ptrs[:3], nv, *ptrs[3:], nc)
        need = (int(visit_ptr[b]), int(cust_ptr[b]))
        if rc not in (0, -3) or need == (nv, nc):         # (-3, GDM_EWORKSPACE: the pointers hold the counts needed)
            _lib.check(rc, "gdm_des_log_visits_host")
            break
        nv, nc = need
    vi32, vi64, vf64, ci32, ci64, cf64 = tables
    return LogVisits(*vi32, *vi64, *vf64, visit_ptr, *ci32, *ci64, *cf64, cust_ptr, status)


def raise_for_visits(status):
    """ValueError for the first sample ``log_visits`` refused."""
    for i, st in enumerate(np.asarray(status).tolist()):
        if st == VISITS_ERECORD:
            raise ValueError(f"log_visits: sample {i} holds a record the walk cannot place (a kind, node or event id out "
                             "of range, or a processing or departure record without its customer's open visit at that "
                             "node in the state it needs)")
        if st:
            raise ValueError(f"log_visits: sample {i}: record offsets outside the log (status {st})")


VisitStats = collections.namedtuple("VisitStats", "started unserved departed wait_sum service_sum blocked_sum")
VisitStats.__doc__ = """``visit_stats``'s result, (B, dim) arrays per node: ``started``, ``unserved``, ``departed`` (int64, the
visits that were started / never started / have a departure record), ``wait_sum`` = the sum of ``t_start - t_arrival``
and ``service_sum`` = the sum of ``service`` over the node's started visits, added one by one from 0.0 in ``rec_start``
order -- the order and the terms of the statistics run's ``time_in_queue`` and ``time_in_service`` on a net without
queue nodes --, and ``blocked_sum`` = the sum of ``t_depart - t_first_depart`` over its departed visits in the order of
their first departures: the time a queue node's customers were held back after their first departure.  On a net with
queue nodes ``wait_sum + blocked_sum`` is ``time_in_queue`` up to the order of the additions -- less one delay where the
run ended while the queue node held a customer back: the statistics run counts a delay when it schedules it, the log
shows it when it is over."""


def _sum_in_order(x):
    """x[0] + x[1] + .. one by one from the left (numpy's ``sum`` adds pairwise)."""
    return float(np.add.accumulate(x)[-1]) if len(x) else 0.0


def _per_node(node, key, dim, terms):
    """Over one sample's visits with key >= 0, in key order: their number per node (dim), and for every array of
    ``terms`` the sum of each node's entries, one by one."""
    idx = np.flatnonzero(key >= 0)
    idx = idx[np.argsort(key[idx], kind="stable")]
    count = np.bincount(node[idx], minlength=dim)
    sums = np.zeros((len(terms), dim), dtype=np.float64)
    for j in np.flatnonzero(count):
        at = idx[node[idx] == j]
        for k, x in enumerate(terms):
            sums[k, j] = _sum_in_order(x[at])
    return count, sums


def visit_stats(v, dim):
    """A LogVisits per node -> VisitStats of (B, dim) arrays: what ties the log run to the statistics run
    (``served``, ``time_in_service``, ``time_in_queue``, and ``reneges`` from below and above)."""
    b = len(v.visit_ptr) - 1
    started, unserved, departed = (np.zeros((b, dim), dtype=np.int64) for _ in range(3))
    wait_sum, service_sum, blocked_sum = (np.zeros((b, dim), dtype=np.float64) for _ in range(3))
    for s in range(b):
        sl = slice(int(v.visit_ptr[s]), int(v.visit_ptr[s + 1]))
        node, rec_start = v.node[sl], v.rec_start[sl]
        unserved[s] = np.bincount(node[rec_start < 0], minlength=dim)
        started[s], (wait_sum[s], service_sum[s]) = _per_node(node, rec_start, dim, (v.t_start[sl] - v.t_arrival[sl],
                                                                                   v.service[sl]))
        departed[s], (blocked_sum[s],) = _per_node(node, v.rec_first_depart[sl], dim,
                                                   (v.t_depart[sl] - v.t_first_depart[sl],))
    return VisitStats(started, unserved, departed, wait_sum, service_sum, blocked_sum)


def waiting_times(v, b, node, skip=0):
    """``t_start - t_arrival`` of the started visits of sample b at ``node``, in start order (``rec_start``), the first
    ``skip`` of them left out (a warm-up)."""
    sl = slice(int(v.visit_ptr[b]), int(v.visit_ptr[b + 1]))
    idx = np.flatnonzero((v.node[sl] == node) & (v.rec_start[sl] >= 0))
    idx = idx[np.argsort(v.rec_start[sl][idx], kind="stable")][int(skip):]
    return v.t_start[sl][idx] - v.t_arrival[sl][idx]


def sojourn_times(v, b):
    """``cust_t_exit - cust_t_enter`` of sample b's EXITED customers, by event id: the time from the first arrival record
    to the last departure record."""
    sl = slice(int(v.cust_ptr[b]), int(v.cust_ptr[b + 1]))
    out = v.cust_outcome[sl] == CUST_EXITED
    return v.cust_t_exit[sl][out] - v.cust_t_enter[sl][out]


def wait_tail(v, node, ts, skip=0):
    """(B, len(ts)): per sample the fraction of ``waiting_times(v, b, node, skip)`` that are > t, for every t of ``ts``;
    NaN for a sample without such a visit."""
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    out = np.full((len(v.visit_ptr) - 1, len(ts)), np.nan)
    for b in range(out.shape[0]):
        w = waiting_times(v, b, node, skip)
        if len(w):
            out[b] = (w[:, None] > ts[None, :]).sum(axis=0) / float(len(w))
    return out


Mm1kWaitSweep = collections.namedtuple("Mm1kWaitSweep", "lam mu queue_cap seeds ts visits stop_reason values mean sem n "
                                                        "theory z")
Mm1kWaitSweep.__doc__ = """``mm1k_wait_sweep``'s result for C configurations x R seeds x T times: lam, mu, queue_cap (C), seeds
(R), ts (T); the LogVisits and the stop reasons of the C * R runs (configuration-major: run c * R + r); ``values``
(C, R, T), per run the fraction of the server's waits that are > ts[t]; their ``mean``, ``sem`` (std with ddof 1 /
sqrt(n)) and ``n`` (C, T) over the runs that neither errored nor ran out of draws; ``theory`` (C, T),
``queueing_theory.mm1k_wait_tail``; and ``z`` = (mean - theory) / sem (0 where the difference is 0)."""


def mm1k_wait_sweep(lams, mus, queue_caps, seeds, ts, *, customers, skip, device=None, math=1):
    """The waiting-time LAW of simulated M/M/1/K beside ``queueing_theory.mm1k_wait_tail``, shaped like ``mm1k_sweep``:
    configuration c = (lams[c], mus[c], queue_caps[c]) on the net of ``mm1k_spec``, every configuration with every seed
    from the global stream ``replication_states(seeds)[r]``, ALL of them one batch.  The log comes from
    ``run_batch_host(..., max_records=0)`` (``math`` is the host mirror's) or, with a ``device``, from one launch of
    ``run_batch_device`` with a record cap no run reaches (four records per event); ``log_visits`` walks it on the host
    either way.  Per run: the fraction of the server's started visits -- the accepted customers, in start order, the
    first ``skip`` left out -- that waited longer than each t of ``ts`` -> Mm1kWaitSweep."""
    from . import ops, queueing_theory as qt
    lams, mus = np.asarray(lams, dtype=np.float64).reshape(-1), np.asarray(mus, dtype=np.float64).reshape(-1)
    caps = np.asarray(queue_caps, dtype=np.int64).reshape(-1)
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    c, r = len(lams), len(seeds)
    if c == 0 or r == 0 or len(mus) != c or len(caps) != c or len(ts) == 0:
        raise ValueError("mm1k_wait_sweep: lams, mus and queue_caps must have one entry per configuration, and seeds and "
                         "ts be given")
    if (caps < 1).any():
        raise ValueError("mm1k_wait_sweep: queue_cap >= 1 (the simulator's rings hold at least one customer)")
    max_events = 4 * int(customers) + 64                  # which no run reaches (an arrival and a departure per customer)
    specs = [mm1k_spec(lams[i], mus[i], caps[i], customers, s) for i in range(c) for s in seeds]
    states = replication_states(seeds) * c
    adj, kind, *rest = dist_arrays(specs)
    if device is None:
        log = run_batch_host(adj, *rest, states, math=math, max_events=max_events, max_records=0, kind=kind)
    else:
        log = run_batch_device(adj, *rest, states, device=device, max_events=max_events,
                               max_records=4 * max_events + 4 * adj.shape[1] + 64, kind=kind)
    visits = log_visits(log, dim=adj.shape[1])
    raise_for_visits(visits.status)
    stop = np.asarray(log.stop_reason.cpu() if hasattr(log.stop_reason, "cpu") else log.stop_reason)
    valid = ((stop != ops.DES_STOP_ERROR) & (stop != ops.DES_STOP_BUDGET)).reshape(c, r)
    values = wait_tail(visits, 1, ts, skip).reshape(c, r, len(ts))
    theory = np.stack([qt.mm1k_wait_tail(lams[i], mus[i], caps[i], ts) for i in range(c)])
    mean, sem, n, z = _sweep_summary({"w": values}, valid, {"w": theory})
    return Mm1kWaitSweep(lams, mus, caps, np.asarray(seeds, dtype=np.int64), ts, visits, stop, values, mean["w"], sem["w"],
                         n["w"], theory, z["w"])


def math_probe_host(x):
    """(des_log(x), sqrt(-2 des_log(x) / x)) on the host: the portable math of the batch simulator alone."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    lg, fac = np.empty_like(x), np.empty_like(x)
    _lib.check(_lib.load().gdm_des_math_probe_host(x.ctypes.data, x.size, lg.ctypes.data, fac.ctypes.data),
               "gdm_des_math_probe_host")
    return lg, fac
