"""Drop-in surface of the G -> DES bridges' numpy prologue on MI355X.

    matrix_to_midi(gen1_output, gen2_output, adj_size=(32,32), instrument=None, start=0, end=150, count=0,
                   generate=False)                      MMGAN_MIDI_DES/matrix_sim_process.py:15-195
    matrix_to_midis(gen1_output, gen2_output, adj_size, instrument, start, end, simulate="des_batch", midi_paths=None)
                                                        the generate=True route for a batch: every sample's track
    matrix_to_wav(matrices, size=20, use_same_instrument=None, start=0, end=174, device='cpu')
                                                        GAN_DES/matrix_sim_process.py:17-137

Both reference functions do, per generated sample, (1) a block of numpy arithmetic that turns the generator's matrix
into the constructor arguments of the discrete-event simulator and (2) the simulation / MIDI / audio rendering.  Part
(2) is INJECTED here as ``simulate``, exactly where the reference constructs ``Sim``: a callable, or the string "des" for
the built-in back end -- simulation_v3's deterministic DES core on the host, then batched device stages over all B
event logs: for matrix_to_midi one log -> MIDI -> piano-roll launch (sim_log_to_midi.py / csrc/des_midi.hip); for
matrix_to_wav log -> notes (sim_log_process_music.py / csrc/des_notes.hip), the integer synth evaluated straight into
the STFT frame matrix (csrc/synth.hip) and the mel chain (util._db_from_frames).  The synth stands where the reference
calls FluidSynth: its sound font is not reproducible and is not imitated.  Part (1) runs batched
on the device (``ops.des_scan`` / ``ops.des_routing``, csrc/des_prologue.hip): the
generator output never leaves HBM as a whole; what crosses to the host is the per-row masks the RNG bookkeeping needs
and the final float64 routing matrices the simulator consumes.

numpy's GLOBAL legacy RNG is part of the reference's behaviour (random sources, the random column that takes a row's
rounding residue, the per-sample reseed ``np.random.seed(np.random.randint(0, 99999, size=1))``); how much of the
stream a draw consumes depends on the data, so the draws are made here on the host, per sample, with the same calls in
the same order -- under the same ``np.random.seed`` the specs are bit-identical to the reference's and the stream ends
at the same position (tests/golden/des_prologue.npz).

The reference INTERLEAVES the samples: draws of sample i, ``Sim(...).run`` of sample i -- which consumes the same global
stream (simulation_v3.py:57,62: ``np.random.choice(self.children, ...)``) from the per-sample seed --, then the draws of
sample i+1.  ``matrix_to_midi`` / ``matrix_to_wav`` keep that order: the RNG-free scan is ONE batched launch, then per
sample: draws, a one-sample ``des_routing`` launch, ``simulate(spec)``, next sample (tests/golden/des_prologue_rng.npz:
recorded with a stand-in Sim that draws from ``np.random`` the way Sim does).  ``midi_prologue`` / ``wav_prologue``
return ALL specs before any simulation runs (one batched routing launch): equal to the reference only for a back end
that leaves numpy's global stream alone.  Reference quirks kept: matrix_to_midi ALWAYS draws random
sources (its emptiness test at line 42 is always true); matrix_to_wav raises ValueError for more than one thresholded
source (line 30) and IndexError for a thresholded column >= dim (line 67); an all-zero row raises ValueError from
``np.random.choice([])``.

simulate="des_batch" (opt-in; "des" is unchanged) batches the one stage "des" leaves per sample and on the host: the
batched prologue (``batched_prologue_midi`` / ``batched_prologue_wav``: one scan launch, ALL host draws in the
reference's order with a snapshot of ``np.random.get_state()`` after each sample's reseed, one routing launch whose
output stays on the device), then ``gdm_des_run_batch`` (one wave per sample, csrc/des_batch.hip) simulates every
sample from ITS snapshot, and the batched consumers read the device log in place.  Below DES_BATCH_DEVICE_MIN_B samples
the host mirror ``gdm_des_run_batch_host`` simulates instead -- the same source compiled for the host, the same bits --
because the launch costs 8-10 ms however small the batch is.  Four differences from "des":
  1. order: all draws come first, then all simulations -- sample i+1's draws no longer continue from where simulation i
     left numpy's global stream, they continue from sample i's reseed.  Each sample is still simulated exactly as the
     reference would simulate it from the state it is given;
  2. last bits: the device has no libm, so ``log`` is the portable one of csrc/des_sim.h -- same events, ids, nodes,
     kinds and ``floor(value)`` on the golden runs, values within 7.7e-14 relative;
  3. record cap: a simulation stops once 5001 records are written (both consumers look at the first 5000 and count up
     to 5001 lines), so ``max_events`` is rarely reached;
  4. final stream position: after the call numpy's global stream is where the batched prologue left it (where
     ``midi_prologue`` / ``wav_prologue`` leave it), not where the last simulation would have.

simulate="des_device" (opt-in; "des" and "des_batch" keep their behaviour and their bits) moves the last host stage of
"des_batch" -- the draws and the float32 parameter arithmetic of ``_midi_spec`` / ``_wav_spec`` -- onto the device
(``device_prologue_midi`` / ``device_prologue_wav``: scan, ``ops.des_draws`` (csrc/des_draws.hip, one wave per sample),
routing), always simulates with the kernel and enqueues scan, draws, routing, simulator and log consumers without a
host synchronisation; ONE read-back at the end carries the draw status words, the scan's finite flags, the stop
reasons and the tracks.  The draws of "des_batch" cannot be reproduced bit for bit in parallel -- they run through ONE
global stream, sample i+1 continuing from sample i's reseed -- so this is a back end of its own.  Differences from
"des_batch":
  1. per-sample streams: sample i draws from ``RandomState(int(base[i]))`` with the same calls in the same order as
     ``_midi_draws`` / ``_wav_draws`` (numpy itself is the oracle: tests/test_des_draws.py), and its simulation starts
     from where those draws leave that stream.  The samples are independent: permuting the batch (and ``base``)
     permutes the results;
  2. one host draw: ``base = np.random.randint(0, 2**32, size=B, dtype=np.uint32)`` (``draw_base_seeds``) is the only
     call on numpy's global stream per bridge call, so ``np.random.seed`` stays the reproducibility handle;
  3. status codes instead of mid-loop exceptions: what raises inside the reference's draws (an empty candidate list,
     more than one thresholded source, a thresholded column >= dim; ``ops.DES_DRAWS_ERRORS``) marks the sample, the
     simulator skips it (DES_STOP_ERROR, no records), and after the read-back ``matrix_to_midi`` / ``matrix_to_wav``
     raise the reference's exception type for the first such sample while ``matrix_to_midis`` marks it failed with
     the text in ``reasons``.  A non-finite generated matrix raises ValueError after the read-back as well;
  4. final stream position: numpy's global stream ends exactly one ``randint`` call after where it started;
  5. no host-mirror switch: the kernel simulates whatever B is.  The launch costs 8-10 ms and is the bridge's floor:
     measured at B = 30 the bridge takes 11.4 ms against 21.8 ms (model 2) and 9.7 against 11.3 ms (model 1), at
     B = 256 12.0 against 122 ms and 16.8 against 49 ms -- it pays from B = 30 on; below
     that size it was not measured, and a handful of samples is where the host mirror of "des_batch" should win.
At most 64 nodes (a row's candidate set is one 64-bit word), which covers both models (61 and 15).
"""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops


@dataclass
class DesSpec:
    """Arguments the reference hands to ``Sim(sim_matrix, distributions, queue_list, seeds=..., max_sim_time=...)``,
    ``Sim.run(number_of_customers=...)`` and ``process_adjsim_log(instruments=..., note_levels=...)``."""
    sim_matrix: np.ndarray            # (dim, dim) float64: row-stochastic routing, diagonal +1 (source) / -1 (server)
    distributions: list               # dim x ['normal', mean, std] (np.float32 scalars, as upstream)
    queue_list: list                  # [254] * dim
    seeds: np.ndarray                 # shape (1,)
    num_customers: int
    max_sim_time: float
    instruments: np.ndarray           # (dim,) float64 holding integers (np.zeros(dim) upstream), or int array
    note_levels: np.ndarray           # (dim,) float64
    sources: np.ndarray = field(default=None)   # node indices that are sources


def _draw_residue_columns(zero_mask, src, dim):
    """One ``np.random.choice`` per row over the columns that are off-diagonal and non-zero after source zeroing
    (matrix_sim_process.py:101-102 / 85-86).  zero_mask: (dim,) int64 bit patterns."""
    cols = np.empty(dim, dtype=np.int32)
    zm = zero_mask.view(np.uint64)
    shifts = np.arange(dim, dtype=np.uint64)
    for i in range(dim):
        nz = ((zm[i] >> shifts) & np.uint64(1)) == 0
        nz &= ~src
        nz[i] = False
        cols[i] = np.random.choice(np.flatnonzero(nz).tolist())       # ValueError on an empty list, like upstream
    return cols


def _reseed():
    np.random.seed(np.random.randint(0, 99999, size=1))
    return np.random.randint(0, 99999, size=1)


def _check_finite(flags):
    if int(flags.max()) != 0:
        raise ValueError("generated matrix holds non-finite values: the DES prologue is defined for finite inputs only")


def _midi_scan(gen1_output, gen2_output, adj_size):
    size = adj_size[0]
    dim = size - 3
    g1 = gen1_output.detach()
    if not g1.is_cuda:
        raise ops.GdmError("matrix_sim_process runs the prologue on a HIP device; move the generator outputs there")
    g1 = g1.float()
    scan = ops.des_scan(g1, size, dim, note_mod=True)
    h = {"g1": g1, "size": size, "dim": dim, "b": g1.shape[0],
         "g2": gen2_output.detach().float().cpu().numpy(), "inst": scan["instruments"].cpu().numpy(),
         "notes": scan["note_levels"].cpu().numpy(), "zmask": scan["zero_mask"].cpu().numpy()}
    _check_finite(scan["flags"].cpu().numpy())
    return h


def _midi_draws(h, i):
    """Sample i's draws from numpy's global stream, in the reference's order (lines 43, 101-102, 119-120)."""
    dim = h["dim"]
    src = np.zeros(dim, dtype=bool)
    sources = np.random.choice(dim, size=dim // 4, replace=False)       # line 43 (the test at 42 is always true)
    src[sources] = True
    cols = _draw_residue_columns(h["zmask"][i], src, dim)
    return src, cols, _reseed()


def _midi_spec(h, i, routing, src, seeds, instrument):
    dim = h["dim"]
    p = h["g2"][i]
    if isinstance(instrument, (list, tuple, np.ndarray)):             # matrix_to_midis: one entry per sample
        instrument = instrument[i]
    d_src = (np.abs(p[1] * 50), np.abs(p[2] * 50))
    d_srv = (np.abs(p[3] * 10), np.abs(p[4] * 10))
    dist = [["normal", *(d_src if src[k] else d_srv)] for k in range(dim)]
    instruments = h["inst"][i].astype(np.float64) if instrument is None else np.array([instrument] * dim)
    return DesSpec(routing, dist, [2 * 127] * dim, seeds, max(200, max(1000, int(3000 * p[6]))), min(float(p[5]), 1.0),
                   instruments, h["notes"][i].astype(np.float64), np.flatnonzero(src))


def _routing(h, lo, hi, src, cols):
    """des_routing for samples [lo, hi) of the scanned batch: src (n,dim) bool, cols (n,dim) int32 -> (n,dim,dim) f64."""
    dev = h["g1"].device
    return ops.des_routing(h["g1"][lo:hi], h["size"], h["dim"],
                           torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(dev)).cpu().numpy()


def _batched_specs(h, draws, spec_of):
    b, dim = h["b"], h["dim"]
    src_all = np.zeros((b, dim), dtype=bool)
    cols_all = np.empty((b, dim), dtype=np.int32)
    seeds = []
    for i in range(b):                                                   # global-RNG order of the reference, per sample
        src_all[i], cols_all[i], sd = draws(h, i)
        seeds.append(sd)
    routing = _routing(h, 0, b, src_all, cols_all)
    return [spec_of(h, i, routing[i], src_all[i], seeds[i]) for i in range(b)]


# "des_batch" simulates on the device from this batch size on and with the host mirror below it.  The two give the same
# bits, so the choice is one of speed only: the launch takes 8-10 ms whatever B is (one wave per sample, a latency-bound
# chain), the sequential host mirror 0.15 ms (15 nodes) to 0.22 ms (61 nodes) per sample plus the transfers of the
# routing matrices and the logs -- measured crossover B = 45-55.
DES_BATCH_DEVICE_MIN_B = 48


class BatchedPrologue:
    """What the batched prologue leaves, each product where its consumer needs it: ``routing`` (B,dim,dim) fp64 on the
    device; ``loc``, ``scale`` (B,dim) f64, ``queue_cap`` (B,dim) i32, ``seed``, ``customers`` (B) i64, ``instruments``,
    ``note_levels`` (B,dim) i32 on the host (built with the float32 arithmetic of ``_midi_spec`` / ``_wav_spec``);
    ``states``: the B snapshots of ``np.random.get_state()`` taken right after each sample's reseed; ``h``: the scan."""

    def __init__(self, h, routing, src, seeds, states, spec_of):
        self.h, self.routing, self.states = h, routing, states
        self._src, self._seeds, self._spec_of = src, seeds, spec_of
        heads = [spec_of(h, i, None, src[i], seeds[i]) for i in range(h["b"])]       # the per-node parameters
        self.loc = np.ascontiguousarray([[float(d[1]) for d in sp.distributions] for sp in heads], dtype=np.float64)
        self.scale = np.ascontiguousarray([[float(d[2]) for d in sp.distributions] for sp in heads], dtype=np.float64)
        self.queue_cap = np.ascontiguousarray([sp.queue_list for sp in heads], dtype=np.int32)
        self.seed = np.ascontiguousarray([int(np.asarray(sp.seeds).reshape(-1)[0]) for sp in heads], dtype=np.int64)
        self.customers = np.ascontiguousarray([sp.num_customers for sp in heads], dtype=np.int64)
        self.instruments = np.ascontiguousarray([[int(x) for x in sp.instruments] for sp in heads], dtype=np.int32)
        self.note_levels = np.ascontiguousarray([[int(x) for x in sp.note_levels] for sp in heads], dtype=np.int32)

    def specs(self):
        """The DesSpecs ``midi_prologue`` / ``wav_prologue`` return (downloads the routing matrices)."""
        routing = self.routing.cpu().numpy()
        return [self._spec_of(self.h, i, routing[i], self._src[i], self._seeds[i]) for i in range(self.h["b"])]

    def simulate(self, device, max_events=200000, max_records=5001):
        """``gdm_des_run_batch`` (device: a HIP device) or the host mirror with portable math (device=None), every
        sample from its snapshot -> simulation_v3.BatchLog."""
        from . import simulation_v3
        if device is None:
            return simulation_v3.run_batch_host(self.routing.cpu().numpy(), self.loc, self.scale, self.queue_cap,
                                                self.seed, self.customers, self.states, math=1, max_events=max_events,
                                                max_records=max_records)
        return simulation_v3.run_batch_device(self.routing, self.loc, self.scale, self.queue_cap, self.seed,
                                              self.customers, self.states, device=device, max_events=max_events,
                                              max_records=max_records, max_queue_cap=max(1, int(self.queue_cap.max())))


    def simulate_on(self, device, max_events=200000, max_records=5001):
        """``simulate`` for the bridges: a BatchLog of tensors on ``device`` either way -- from the kernel when the batch
        holds at least DES_BATCH_DEVICE_MIN_B samples, else from the host mirror (same bits), uploaded once."""
        from . import simulation_v3
        if self.h["b"] >= DES_BATCH_DEVICE_MIN_B:
            return self.simulate(device, max_events=max_events, max_records=max_records)
        host = self.simulate(None, max_events=max_events, max_records=max_records)
        dev = torch.device(device)
        fields = [torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)
                  for a in host]
        return simulation_v3.BatchLog(*fields)


def _batched_prologue(h, draws, spec_of):
    b, dim = h["b"], h["dim"]
    src_all = np.zeros((b, dim), dtype=bool)
    cols_all = np.empty((b, dim), dtype=np.int32)
    seeds, states = [], []
    for i in range(b):                                                   # global-RNG order of the reference, per sample
        src_all[i], cols_all[i], sd = draws(h, i)
        seeds.append(sd)
        states.append(np.random.get_state())                             # where simulation i starts
    dev = h["g1"].device
    routing = ops.des_routing(h["g1"], h["size"], dim, torch.from_numpy(src_all.astype(np.uint8)).to(dev),
                              torch.from_numpy(cols_all).to(dev))
    return BatchedPrologue(h, routing, src_all, seeds, states, spec_of)


def batched_prologue_midi(gen1_output, gen2_output, adj_size=(32, 32), instrument=None):
    """``midi_prologue`` with its products left where "des_batch" needs them -> BatchedPrologue."""
    h = _midi_scan(gen1_output, gen2_output, adj_size)
    return _batched_prologue(h, _midi_draws, lambda h_, i, r, src, sd: _midi_spec(h_, i, r, src, sd, instrument))


def batched_prologue_wav(matrices, size=20, use_same_instrument=None):
    """``wav_prologue`` with its products left where "des_batch" needs them -> BatchedPrologue."""
    h = _wav_scan(matrices, size)
    return _batched_prologue(h, _wav_draws, lambda h_, i, r, src, sd: _wav_spec(h_, i, r, src, sd, use_same_instrument))


# ---- "des_device": the draws and parameters on the device, one stream per sample --------------------------------------
DES_DEVICE_QUEUE_CAP = 2 * 127           # queue_list = [2 * 127] * dim: sizes the simulator's workspace without a read-back


def draw_base_seeds(b):
    """The ONE call "des_device" makes on numpy's global stream per bridge call: sample i draws from
    ``RandomState(int(base[i]))``."""
    return np.random.randint(0, 2 ** 32, size=b, dtype=np.uint32)


def _instrument_override(instrument, b):
    """None, one program, or a list of B (None or a program) -> (B,) int32 array, or None when nothing is overridden."""
    if instrument is None:
        return None
    if isinstance(instrument, (list, tuple, np.ndarray)):
        if len(instrument) != b:
            raise ops.GdmError(f"des_device: {len(instrument)} instruments for {b} samples")
        return np.array([ops.DES_DRAWS_NO_INSTRUMENT if x is None else int(x) for x in instrument], dtype=np.int32)
    return np.full(b, int(instrument), dtype=np.int32)


def des_draws_host(route, s, dim, base, zero_mask, scan_instruments, scan_note_levels, params, thr_mask=None,
                   instrument_override=None):
    """``gdm_des_draws_host`` on numpy arrays: the device kernel's source compiled for the host, the same bits (see
    ``ops.des_draws`` for the arguments and the dict that comes back; mt_key is uint32 here)."""
    from . import _lib
    base = np.ascontiguousarray(base, dtype=np.uint32).reshape(-1)
    b = base.size
    zm = np.ascontiguousarray(zero_mask).view(np.uint64).reshape(b, dim)
    inst = np.ascontiguousarray(scan_instruments, dtype=np.int32).reshape(b, dim)
    notes = np.ascontiguousarray(scan_note_levels, dtype=np.int32).reshape(b, dim)
    params = np.ascontiguousarray(params, dtype=np.float32).reshape(b, -1)
    thr = None if thr_mask is None else np.ascontiguousarray(thr_mask, dtype=np.uint8).reshape(b, s)
    over = None if instrument_override is None else np.ascontiguousarray(instrument_override, dtype=np.int32).reshape(b)
    shapes = {"d": (b, dim), "": (b,), "k": (b, 624)}
    np_dt = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64, torch.float64: np.float64}
    out = {name: np.zeros(shapes[kind], dtype=np.uint32 if name == "mt_key" else np_dt[dt])
           for name, dt, kind in ops._DES_DRAWS_FIELDS}
    ptr = lambda a: None if a is None else a.ctypes.data                                         # noqa: E731
    rc = _lib.load().gdm_des_draws_host(int(route), b, int(s), int(dim), ptr(base), ptr(zm), ptr(thr), ptr(inst),
                                        ptr(notes), ptr(params), params.shape[1], ptr(over),
                                        *(ptr(out[name]) for name, _dt, _k in ops._DES_DRAWS_FIELDS))
    _lib.check(rc, "gdm_des_draws_host")
    return out


def draws_error(status):
    """Status word of one sample -> the exception the reference raises for it."""
    kind, text = ops.DES_DRAWS_ERRORS[int(status)]
    return kind(text)


class DevicePrologue:
    """What the device prologue leaves -- the fields of ``BatchedPrologue``, every one a device tensor: ``routing``
    (B,dim,dim) f64, ``loc``, ``scale`` (B,dim) f64, ``queue_cap`` (B,dim) i32, ``seed``, ``customers`` (B) i64,
    ``instruments``, ``note_levels`` (B,dim) i32, ``states`` = (mt_key (B,624) i32, mt_pos, has_gauss (B) i32, gauss (B)
    f64): every sample's stream after its last draw; plus ``src`` (B,dim) u8, ``cols`` (B,dim) i32, ``status`` (B) i32
    (``ops.DES_DRAWS_ERRORS``), ``flags`` (B) i32 of the scan and ``base`` (B,) uint32 on the host.  Nothing was read
    back: ``status`` and ``flags`` travel with the consumer's one read-back (``readback_words`` / ``raise_for``)."""

    def __init__(self, h, base, draws, routing):
        self.h, self.base, self.routing = h, base, routing
        for name, _dt, _kind in ops._DES_DRAWS_FIELDS:
            setattr(self, name, draws[name])
        self.states = (draws["mt_key"], draws["mt_pos"], draws["has_gauss"], draws["gauss"])
        self.flags = h["flags"]

    def simulate_on(self, device, max_events=200000, max_records=5001):
        """``gdm_des_run_batch`` from the device streams, whatever B is -> BatchLog of device tensors.  The kernel
        advances ``states`` in place: simulate once per prologue."""
        from . import simulation_v3
        return simulation_v3.run_batch_device(self.routing, self.loc, self.scale, self.queue_cap, self.seed,
                                              self.customers, self.states, device=device, max_events=max_events,
                                              max_records=max_records, max_queue_cap=DES_DEVICE_QUEUE_CAP)

    simulate = simulate_on

    def readback_words(self):
        """int32 device tensors to append to the consumer's read-back: draw status, scan flags."""
        return [self.status, self.flags]

    @staticmethod
    def check_flags(flags):
        _check_finite(np.asarray(flags))

    @staticmethod
    def raise_for(status):
        """Raise what the reference raises for the first sample with a draw status."""
        for i in np.flatnonzero(np.asarray(status)):
            raise draws_error(status[i])


def _device_prologue(route, h, scan, params, override, base):
    b, dim, dev = h["b"], h["dim"], h["g1"].device
    if dim > ops.DES_DRAWS_MAX_DIM:
        raise ops.GdmError(f"des_device: at most {ops.DES_DRAWS_MAX_DIM} nodes (a row's candidates are one 64-bit word)")
    base = draw_base_seeds(b) if base is None else np.ascontiguousarray(base, dtype=np.uint32).reshape(b)
    base_dev = torch.from_numpy(base.view(np.int32)).to(dev)
    over = None if override is None else torch.from_numpy(override).to(dev)
    draws = ops.des_draws(route, h["size"], dim, base_dev, scan, params, over)
    routing = ops.des_routing(h["g1"], h["size"], dim, draws["src"], draws["cols"])
    h["flags"] = scan["flags"]
    return DevicePrologue(h, base, draws, routing)


def device_prologue_midi(gen1_output, gen2_output, adj_size=(32, 32), instrument=None, *, base=None):
    """The MIDI route's prologue entirely on the device: scan, ``ops.des_draws`` (sample i on the stream
    ``RandomState(base[i])``; base=None: ``draw_base_seeds``, the one call on numpy's global stream), routing.  No host
    synchronisation, nothing read back -> DevicePrologue."""
    size = adj_size[0]
    dim = size - 3
    g1 = gen1_output.detach()
    if not g1.is_cuda:
        raise ops.GdmError("matrix_sim_process runs the prologue on a HIP device; move the generator outputs there")
    g1 = g1.float()
    g2 = gen2_output.detach().to(device=g1.device, dtype=torch.float32).contiguous()
    if g2.dim() != 2 or g2.shape[0] != g1.shape[0] or g2.shape[1] < 7:
        raise ops.GdmError("des_device: gen2_output must be (B, n) with n >= 7 (columns 1..6 drive the simulator)")
    scan = ops.des_scan(g1, size, dim, note_mod=True)
    h = {"g1": g1, "size": size, "dim": dim, "b": g1.shape[0], "g2": g2}
    return _device_prologue(ops.DES_DRAWS_MIDI, h, scan, g2, _instrument_override(instrument, g1.shape[0]), base)


def device_prologue_wav(matrices, size=20, use_same_instrument=None, *, base=None):
    """The wav route's prologue entirely on the device (see ``device_prologue_midi``) -> DevicePrologue."""
    dim = size - 5
    m = matrices.detach() if isinstance(matrices, torch.Tensor) else torch.as_tensor(np.asarray(matrices))
    if not m.is_cuda:
        raise ops.GdmError("matrix_sim_process runs the prologue on a HIP device; move the generated matrices there")
    m = m.float()
    scan = ops.des_scan(m, size, dim, threshold=0.75, norm_aux=True)
    h = {"g1": m, "size": size, "dim": dim, "b": m.shape[0]}
    return _device_prologue(ops.DES_DRAWS_WAV, h, scan, scan["aux"],
                            _instrument_override(use_same_instrument, m.shape[0]), base)


def _interleaved_specs(h, draws, spec_of):
    """The reference's order: a sample's spec is complete (and handed to the caller, who simulates) before the next
    sample draws anything."""
    for i in range(h["b"]):
        src, cols, sd = draws(h, i)
        routing = _routing(h, i, i + 1, src[None], cols[None])[0]
        yield spec_of(h, i, routing, src, sd)


def midi_prologue(gen1_output, gen2_output, adj_size=(32, 32), instrument=None):
    """Device-batched head of matrix_to_midi: gen1_output (B,1,S,S), gen2_output (B,n2) device tensors -> [DesSpec].
    All draws are made before the first spec is returned (see the module docstring)."""
    h = _midi_scan(gen1_output, gen2_output, adj_size)
    return _batched_specs(h, _midi_draws, lambda h_, i, r, src, sd: _midi_spec(h_, i, r, src, sd, instrument))


def matrix_to_midi(gen1_output, gen2_output, adj_size=(32, 32), instrument=None, start=0, end=150, count=0,
                   generate=False, simulate=None, *, return_tensor=False, midi_path=None, max_events=200000):
    """Reference signature + ``simulate``.

    simulate=callable: ``simulate(spec, count=..., start=..., end=..., generate=..., gen2_tail=...)`` stands in for Sim +
    process_adjsim_log and returns (roll, durations) as (128, end-start) arrays, or None for a failed / timed-out
    simulation.
    simulate="des": the built-in back end.  Per sample, in the reference's order: draws, routing, ``run_spec`` (the
    deterministic DES core; it consumes numpy's global stream like upstream's Sim, so the next sample's draws start
    where the reference's do); then ONE ``des_log_to_roll`` launch turns all B event logs into the planes
    (sim_log_to_midi.log_to_rolls).  A sample whose simulation raises counts as failed and keeps a zero roll.  With
    ``generate`` the last sample's track is also written to ``midi_path`` (default adj_sim_outputs/midi/generation.mid,
    the file upstream overwrites per sample).  The reference's 2.5 s wall-clock timeout has no counterpart: the core
    stops after ``max_events`` events instead.

    simulate="des_batch": batched prologue, ONE device simulator launch for all B samples (each from its own snapshot
    of numpy's stream, 5001-record cap), then the same ``des_log_to_roll`` launch fed from the device log; the save
    flags come from the device counts, and the one read-back at the end brings the stop reasons with the tracks.  A
    sample whose simulation errors (or exhausts its draw budget) counts as failed and keeps a zero roll.  See the
    module docstring for the four differences from "des".

    simulate="des_device": "des_batch" with the draws and the parameter arithmetic on the device too, one independent
    stream per sample, no host synchronisation before the one read-back; a sample whose draws the reference would
    raise for raises here after that read-back (ValueError).  See the module docstring for the differences.

    Returns (list of (2,128,end-start) float64 arrays, failed_simulations); with ``return_tensor`` (built-in back end)
    the rolls stay on the device as one (B,2,128,end-start) fp32 tensor."""
    if simulate is None:
        raise ops.GdmError("matrix_to_midi: pass simulate=\"des\" for the built-in DES / MIDI back end or "
                           "simulate=callable (it receives the DesSpec the reference would construct Sim from)")
    start, end = int(start), int(end)
    if isinstance(simulate, str):
        if simulate not in ("des", "des_batch", "des_device"):
            raise ops.GdmError(f"matrix_to_midi: unknown back end {simulate!r} (the built-in ones are \"des\", "
                               "\"des_batch\" and \"des_device\")")
        if simulate == "des":
            return _matrix_to_midi_des(gen1_output, gen2_output, adj_size, instrument, start, end, generate,
                                       return_tensor, midi_path, max_events)
        return _matrix_to_midi_des_batch(gen1_output, gen2_output, adj_size, instrument, start, end, generate,
                                         return_tensor, midi_path, max_events, device_draws=simulate == "des_device")
    if return_tensor:
        raise ops.GdmError("matrix_to_midi: return_tensor needs the built-in back end (simulate=\"des\")")
    h = _midi_scan(gen1_output, gen2_output, adj_size)
    g2 = h["g2"]
    midi_rolls, failed = [], 0
    specs = _interleaved_specs(h, _midi_draws, lambda h_, i, r, src, sd: _midi_spec(h_, i, r, src, sd, instrument))
    for index, spec in enumerate(specs):
        this_count = count if index == 0 else 1
        output = np.zeros((2, 128, end - start))
        res = simulate(spec, count=this_count, start=start, end=end, generate=generate, gen2_tail=g2[index][10:])
        if res is None or res[0] is None:
            failed += 1
        else:
            output[0], output[1] = res[0], res[1]
        midi_rolls.append(output)
    return midi_rolls, failed


def _des_run(gen1_output, gen2_output, adj_size, instrument, start, end, generate, max_events, raise_for_status=True):
    """The body "des" shares between ``matrix_to_midi`` and ``matrix_to_midis`` -> (planes on the device, tracks, status
    (B,), reasons (None or why the simulation failed), ok, save)."""
    from . import sim_log_to_midi, simulation_v3
    _check_midi_window(start, end)
    h = _midi_scan(gen1_output, gen2_output, adj_size)
    if h["g2"].shape[1] < 16:
        raise ops.GdmError("matrix_to_midi: gen2_output needs at least 16 columns (gen2_output[10:16] drive the MIDI)")
    specs = _interleaved_specs(h, _midi_draws, lambda h_, i, r, src, sd: _midi_spec(h_, i, r, src, sd, instrument))
    logs, ok, insts, notes, reasons = [], [], [], [], []
    for spec in specs:
        try:
            log, _reason = simulation_v3.run_spec(spec, max_events=max_events)
            ok.append(True)
            reasons.append(None)
        except (ValueError, KeyError) as e:
            log = np.zeros(0, dtype=simulation_v3.EVENT_DTYPE)
            ok.append(False)
            reasons.append(f"error ({e})")
        logs.append(log)
        insts.append(spec.instruments)
        notes.append(spec.note_levels)
    save = [good and (bool(generate) or sim_log_to_midi.lines_read(len(lg)) % 100 == 0) for good, lg in zip(ok, logs)]
    rolls, tracks, status = sim_log_to_midi.log_to_rolls(logs, h["g2"][:, 10:], insts, notes, start=start, end=end,
                                                         save=save, device=h["g1"].device, return_status=True,
                                                         raise_for_status=raise_for_status)
    return rolls, tracks, status, reasons, ok, save


def _matrix_to_midi_des(gen1_output, gen2_output, adj_size, instrument, start, end, generate, return_tensor, midi_path,
                        max_events):
    from . import sim_log_to_midi
    rolls, tracks, _status, _reasons, ok, save = _des_run(gen1_output, gen2_output, adj_size, instrument, start, end,
                                                          generate, max_events)
    failed = len(ok) - sum(ok)
    if generate:
        done = [i for i, sv in enumerate(save) if sv]
        if done:
            sim_log_to_midi.write_midi(tracks[done[-1]], midi_path or "adj_sim_outputs/midi/generation.mid")
    if return_tensor:
        return rolls, failed
    return [r for r in rolls.double().cpu().numpy()], failed


def _check_midi_window(start, end):
    if end - start <= 0:
        raise ValueError("negative dimensions are not allowed")          # np.zeros((2, 128, end - start)) upstream
    if ops.des_roll_width(start, end) != end - start:
        # generate_piano_roll's `[:, start:end]` of planes that are only end - start wide: upstream's assignment
        # into the (2, 128, end - start) output fails to broadcast and the bare except re-raises ValueError
        raise ValueError("Error in simulation thread, using blank piano roll instead. (start/end: the reference's "
                         "final slice does not leave end - start columns; use start == 0 or end >= 128)")


def _on(a, dev):
    """numpy array or tensor -> contiguous tensor on ``dev``."""
    return a.contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _des_batch_run(gen1_output, gen2_output, adj_size, instrument, start, end, generate, max_events,
                   device_draws=False):
    """The body "des_batch" and "des_device" share between ``matrix_to_midi`` and ``matrix_to_midis``: batched (or
    device) prologue, simulator, one ``des_log_to_roll`` launch, ONE read-back -> (planes (B,2,128,W) on the device;
    status, track_len, good, save, stop (B,) and tracks (B, cap, 4) int32 host arrays; draw status (B,) or None)."""
    from . import sim_log_to_midi
    _check_midi_window(start, end)
    if device_draws and gen2_output.shape[1] < 16:
        raise ops.GdmError("matrix_to_midi: gen2_output needs at least 16 columns (gen2_output[10:16] drive the MIDI)")
    pro = (device_prologue_midi if device_draws else batched_prologue_midi)(gen1_output, gen2_output, adj_size,
                                                                              instrument)
    h = pro.h
    if h["g2"].shape[1] < 16:
        raise ops.GdmError("matrix_to_midi: gen2_output needs at least 16 columns (gen2_output[10:16] drive the MIDI)")
    dev = h["g1"].device
    log = pro.simulate_on(dev, max_events=max_events, max_records=sim_log_to_midi.MAX_LINES + 1)
    good = (log.stop_reason != ops.DES_STOP_ERROR) & (log.stop_reason != ops.DES_STOP_BUDGET)
    lines = torch.clamp(log.n_records, max=sim_log_to_midi.MAX_LINES + 1)             # lines_read, on the device
    save = (good & ((lines % 100 == 0) | bool(generate))).to(torch.int32)
    tails = _on(h["g2"][:, 10:], dev)
    planes, track, track_len, status = ops.des_log_to_roll(
        log.value, log.event_id, log.node, log.kind, log.rec_ptr, tails, _on(pro.instruments, dev),
        _on(pro.note_levels, dev), save, start, end, check_rec_ptr=not device_draws)
    # the one read-back: stop reasons (and the device prologue's status words) with the tracks
    extra = pro.readback_words() if device_draws else []
    words = torch.cat([status, track_len, good.to(torch.int32), save, log.stop_reason.to(torch.int32), *extra,
                       track.reshape(-1)]).cpu().numpy()
    b = h["b"]
    status, track_len, good, save, stop = (words[k * b:(k + 1) * b] for k in range(5))
    draw_status = None
    if device_draws:
        draw_status = words[5 * b:6 * b]
        pro.check_flags(words[6 * b:7 * b])
    tracks = words[(5 + len(extra)) * b:].reshape(b, ops.DES_MIDI_TRACK_CAP, 4)
    return planes, status, track_len, good, save, stop, tracks, draw_status


def _matrix_to_midi_des_batch(gen1_output, gen2_output, adj_size, instrument, start, end, generate, return_tensor,
                              midi_path, max_events, device_draws=False):
    from . import sim_log_to_midi
    planes, status, track_len, good, save, _stop, tracks, draw_status = _des_batch_run(
        gen1_output, gen2_output, adj_size, instrument, start, end, generate, max_events, device_draws)
    if draw_status is not None:
        DevicePrologue.raise_for(draw_status)
    b = len(status)
    for i in range(b):
        if status[i] >> 8:
            raise ValueError(f"Error in processing log file (sample {i}: {ops.DES_MIDI_ERRORS[int(status[i]) >> 8]})")
    failed = int(b - good.sum())
    if generate:
        done = np.flatnonzero(save)
        if len(done):
            last = int(done[-1])
            sim_log_to_midi.write_midi(tracks[last, :track_len[last]], midi_path or "adj_sim_outputs/midi/generation.mid")
    if return_tensor:
        return planes, failed
    return [r for r in planes.double().cpu().numpy()], failed


@dataclass
class MidiBatch:
    """What ``matrix_to_midis`` returns: ``rolls`` (B,2,128,end-start) fp32 on the device (zero for a failed sample);
    ``tracks``: per sample the (len, 4) int32 track (kind, a, b, time) or None; ``ok`` (B,) bool; ``reasons``: None for
    an ok sample, else the simulator's stop reason or the ``ops.DES_MIDI_ERRORS`` text; ``paths``: the files written
    (``generate_midis``; None where nothing was written)."""
    rolls: torch.Tensor
    tracks: list
    ok: np.ndarray
    reasons: list
    paths: list = None


def matrix_to_midis(gen1_output, gen2_output, adj_size, instrument, start, end, *, simulate="des_batch", midi_paths=None,
                    max_events=200000):
    """``matrix_to_midi(..., generate=True)`` for a batch that keeps EVERY sample's track instead of the last one's
    (upstream overwrites one generation.mid per sample, MMGAN_MIDI_DES/sim_log_to_midi.py): the same prologue, the same
    simulations and the same ``des_log_to_roll`` launch as the built-in back ends "des" / "des_batch", hence the same
    rolls under the same ``np.random.seed``, with one read-back ("des_device":
    see the module docstring).  instrument: None, one program for all samples, or a
    list of B (None or a program).  midi_paths: B paths (file i is ``write_midi(tracks[i], midi_paths[i])`` for every
    ok sample) or None to write nothing.  A failed simulation or a per-sample MIDI error marks that sample failed --
    zero roll, no track, no file, its reason in ``reasons`` -- and nothing is raised for it.  -> MidiBatch."""
    from . import sim_log_to_midi, simulation_v3
    start, end = int(start), int(end)
    if simulate not in ("des", "des_batch", "des_device"):
        raise ops.GdmError(f"matrix_to_midis: unknown back end {simulate!r} (the built-in ones are \"des\", "
                           "\"des_batch\" and \"des_device\")")
    b = gen1_output.shape[0]
    if midi_paths is not None and len(midi_paths) != b:
        raise ops.GdmError(f"matrix_to_midis: {len(midi_paths)} midi_paths for {b} samples")
    if simulate in ("des_batch", "des_device"):
        planes, status, track_len, good, _save, stop, track, draw_status = _des_batch_run(
            gen1_output, gen2_output, adj_size, instrument, start, end, True, max_events, simulate == "des_device")
        tracks = [track[i, :track_len[i]].copy() for i in range(b)]
        reasons = [None if good[i] else simulation_v3.STOP_REASONS[int(stop[i])] for i in range(b)]
        for i in np.flatnonzero(draw_status if draw_status is not None else []):
            reasons[i] = f"error ({draws_error(draw_status[i])})"
    else:
        planes, tracks, status, reasons = _des_run(gen1_output, gen2_output, adj_size, instrument, start, end, True,
                                                   max_events, raise_for_status=False)[:4]
    ok = np.array([reasons[i] is None for i in range(b)])
    for i in np.flatnonzero(np.asarray(status) >> 8):
        ok[i], reasons[i] = False, ops.DES_MIDI_ERRORS[int(status[i]) >> 8]
    if not ok.all():
        planes[torch.from_numpy(~ok).to(planes.device)] = 0.0
    tracks = [tr if ok[i] else None for i, tr in enumerate(tracks)]
    res = MidiBatch(planes, tracks, ok, reasons)
    if midi_paths is not None:
        res.paths = [sim_log_to_midi.write_midi(tracks[i], str(midi_paths[i])) if ok[i] else None for i in range(b)]
    return res


def _batch_to_mel(pro, max_events):
    """The built-in batched back end behind matrix_to_wav: BatchedPrologue -> ((B, 128, 216) dB device tensor, (notes,
    n_notes, clip_len) device tensors).  Simulator, log -> notes, synth and mel are enqueued without a read-back in
    between; the status words and stop reasons come back once, and a sample the reference would raise for raises."""
    from . import sim_log_process_music, util
    dev = pro.h["g1"].device
    log = pro.simulate_on(dev, max_events=max_events, max_records=sim_log_process_music.MAX_LINES + 1)
    notes, n_notes, clip_len, status = ops.des_log_to_notes(log.value, log.event_id, log.node, log.kind, log.rec_ptr,
                                                            _on(pro.note_levels, dev),
                                                            check_rec_ptr=not isinstance(pro, DevicePrologue))
    frames = ops.synth_frames(notes, n_notes, clip_len)
    mel = util._db_from_frames(frames, pro.h["b"], ops.SYNTH_FRAMES, ops.SYNTH_RATE, ops.SYNTH_NFFT, 128, 20, 8300, 80)
    extra = pro.readback_words() if isinstance(pro, DevicePrologue) else []
    words = torch.stack([status, log.stop_reason, *extra]).cpu()
    if extra:                                    # the device prologue's own errors come first, as in the reference
        pro.check_flags(words[3].numpy())
        pro.raise_for(words[2].numpy())
    for i, reason in enumerate(words[1].tolist()):
        if reason in (ops.DES_STOP_ERROR, ops.DES_STOP_BUDGET):
            from . import simulation_v3
            raise ValueError(f"matrix_to_wav: the simulation of sample {i} stopped with "
                             f"{simulation_v3.STOP_REASONS[reason]!r} (a node without destination, a customer routed "
                             "to a source, or a service distribution that never turns positive; the reference raises "
                             "or never returns)")
    sim_log_process_music.raise_for_status(words[0])
    return mel, (notes, n_notes, clip_len)


def _wav_scan(matrices, size):
    dim = size - 5
    m = matrices.detach() if isinstance(matrices, torch.Tensor) else torch.as_tensor(np.asarray(matrices))
    if not m.is_cuda:
        raise ops.GdmError("matrix_sim_process runs the prologue on a HIP device; move the generated matrices there")
    m = m.float()
    scan = ops.des_scan(m, size, dim, threshold=0.75, norm_aux=True)
    h = {"g1": m, "size": size, "dim": dim, "b": m.shape[0], "thr": scan["thr_mask"].cpu().numpy().astype(bool),
         "inst": scan["instruments"].cpu().numpy(), "notes": scan["note_levels"].cpu().numpy(),
         "zmask": scan["zero_mask"].cpu().numpy(), "aux": scan["aux"].cpu().numpy()}
    _check_finite(scan["flags"].cpu().numpy())
    return h


def _wav_draws(h, i):
    dim, size = h["dim"], h["size"]
    hit = np.flatnonzero(h["thr"][i])
    if len(hit) == 0:
        sources = np.random.choice(dim, size=size // 8, replace=False)     # line 27
    elif len(hit) == 1:
        sources = hit
    else:
        raise ValueError("The truth value of an array with more than one element is ambiguous (matrix_to_wav keeps "
                         "np.where's tuple: more than one thresholded source cannot be processed, line 30)")
    if sources.max() >= dim:
        raise IndexError(f"index {int(sources.max())} is out of bounds for axis 1 with size {dim}")   # line 67
    src = np.zeros(dim, dtype=bool)
    src[sources] = True
    cols = _draw_residue_columns(h["zmask"][i], src, dim)
    return src, cols, _reseed()


def _wav_spec(h, i, routing, src, seeds, use_same_instrument):
    dim = h["dim"]
    r3, r4 = h["aux"][i, 0], h["aux"][i, 1]
    dist = [["normal", 30 * r3[k], 15 * r4[k]] if src[k] else ["normal", 5 * r3[k], 3 * r4[k]] for k in range(dim)]
    instruments = h["inst"][i].astype(np.float64) if use_same_instrument is None else \
        np.array([use_same_instrument] * dim)
    return DesSpec(routing, dist, [2 * 127] * dim, seeds, 1000, 0.5, instruments, h["notes"][i].astype(np.float64),
                   np.flatnonzero(src))


def wav_prologue(matrices, size=20, use_same_instrument=None):
    """Device-batched head of matrix_to_wav: matrices (B,size,size) device tensor -> [DesSpec].  All draws are made
    before the first spec is returned (see the module docstring)."""
    h = _wav_scan(matrices, size)
    return _batched_specs(h, _wav_draws, lambda h_, i, r, src, sd: _wav_spec(h_, i, r, src, sd, use_same_instrument))


def matrix_to_wav(matrices, size=20, use_same_instrument=None, start=0, end=174, device="cpu", simulate=None, *,
                  max_events=200000):
    """Reference signature + ``simulate``.  Returns the stacked (B,128,end-start) dB tensor on ``device``.

    simulate=callable: ``simulate(spec, index=...)`` stands in for Sim + log->MIDI + FluidSynth + mel featuriser and
    returns the (128, T) dB spectrogram tensor of one sample.
    simulate="des": the built-in back end.  Per sample, in the reference's order: draws, routing, ``run_spec`` (the
    deterministic DES core; it consumes numpy's global stream like upstream's Sim); then the B logs are uploaded once and
    three batched device stages follow without a host round trip between them: log -> notes, notes -> the (B*216, 2048)
    STFT frame matrix of the integer synth, frames -> mel dB.  A clip without notes is the reference's "blank wav":
    -100 dB everywhere.  Exceptions of the prologue and of ``run_spec`` propagate (the reference has no ``try``
    either).  The reference's 0.5 s wall-clock cap has no counterpart: the core stops after ``max_events`` events.
    simulate="des_batch": batched prologue, ONE device simulator launch for all B samples (each from its own snapshot
    of numpy's stream, 5001-record cap), then the same three stages reading the device log in place.  A sample whose
    simulation errors raises ValueError after all stages are enqueued (one read-back).  See the module docstring for
    the four differences from "des".
    simulate="des_device": "des_batch" with the draws and the parameter arithmetic on the device too, one independent
    stream per sample; ValueError / IndexError of the reference's draws are raised after the one read-back.  See the
    module docstring for the differences."""
    if simulate is None:
        raise ops.GdmError("matrix_to_wav: pass simulate=\"des\" for the built-in DES / synth back end or "
                           "simulate=callable (it receives the DesSpec the reference would construct Sim from)")
    if isinstance(simulate, str) and simulate in ("des_batch", "des_device"):
        prologue = batched_prologue_wav if simulate == "des_batch" else device_prologue_wav
        mel, _notes = _batch_to_mel(prologue(matrices, size, use_same_instrument), max_events)
        return mel[:, :, start:end].to(device)
    h = _wav_scan(matrices, size)
    specs = _interleaved_specs(h, _wav_draws, lambda h_, i, r, src, sd: _wav_spec(h_, i, r, src, sd, use_same_instrument))
    if isinstance(simulate, str):
        if simulate != "des":
            raise ops.GdmError(f"matrix_to_wav: unknown back end {simulate!r} (the built-in ones are \"des\", "
                               "\"des_batch\" and \"des_device\")")
        mel, _notes = _specs_to_mel(specs, h["g1"].device, max_events)
        return mel[:, :, start:end].to(device)
    spectrograms = [torch.as_tensor(simulate(spec, index=i)) for i, spec in enumerate(specs)]
    return torch.stack([s[:, start:end] for s in spectrograms]).to(device)


def _specs_to_mel(specs, dev, max_events):
    """The built-in back end behind matrix_to_wav: DesSpecs (consumed one by one, so that each simulation runs before
    the next sample's draws) -> ((B, 128, 216) dB device tensor, (notes, n_notes, clip_len) device tensors)."""
    from . import sim_log_process_music, simulation_v3, util
    logs, insts, notes = [], [], []
    for spec in specs:
        log, _reason = simulation_v3.run_spec(spec, max_events=max_events)
        logs.append(log)
        insts.append(spec.instruments)
        notes.append(spec.note_levels)
    *staged, status = sim_log_process_music.stage_notes(logs, insts, notes, device=dev)
    frames = ops.synth_frames(*staged)
    mel = util._db_from_frames(frames, len(logs), ops.SYNTH_FRAMES, ops.SYNTH_RATE, ops.SYNTH_NFFT, 128, 20, 8300, 80)
    sim_log_process_music.raise_for_status(status)           # read back once, after all three stages are enqueued
    return mel, tuple(staged)
