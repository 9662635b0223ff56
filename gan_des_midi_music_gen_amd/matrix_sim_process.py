"""Drop-in surface of the G -> DES bridges' numpy prologue on MI355X.

    matrix_to_midi(gen1_output, gen2_output, adj_size=(32,32), instrument=None, start=0, end=150, count=0,
                   generate=False)                      MMGAN_MIDI_DES/matrix_sim_process.py:15-195
    matrix_to_midis(gen1_output, gen2_output, adj_size, instrument, start, end, simulate="des_batch", midi_paths=None)
                                                        the generate=True route for a batch: every sample's track
    matrix_to_wav(matrices, size=20, use_same_instrument=None, start=0, end=174, device='cpu')
                                                        GAN_DES/matrix_sim_process.py:17-137
    matrices_to_mel(matrices, size=20, use_same_instrument=None, *, simulate)
                                                        matrix_to_wav's built-in back ends, keeping the note lists

How the module is laid out: what differs between the two bridges is one ``Route`` record each (``MIDI``, ``WAV``: the
scan's arguments, the host draws ``_midi_draws`` / ``_wav_draws``, the spec builders ``_midi_spec`` / ``_wav_spec``, the
``ops.des_draws`` route), and the stages are written once over it: ``Route.scan`` (validation + the scan launch, its
products downloaded or left on the device), ``Route.specs`` (the reference's interleaved order), ``Route.batched`` ->
``BatchedPrologue`` and ``Route.device`` -> ``DevicePrologue``.  The two prologues show their consumers one surface
(the per-node fields, ``simulate_on``, ``readback_words``, ``check``, ``check_rec_ptr``); ``BACK_ENDS`` /
``check_back_end`` name the built-in back ends for every module that takes one, and the back-end name picks the
prologue in ``Route.prologue``.  ``midi_prologue`` ... ``device_prologue_wav`` are the public wrappers.

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
``np.random.choice([])``.  One deviation: upstream's ``int(matrix[dim + 1, i] * 126)`` is a Python integer without an
upper limit, the scan's is an int32.  A sample with an instrument or note-level entry whose float32 product with 126 is
not below 2^31 (|m| from about 1.7044e7 on; a generator's sigmoid output stays below 1) is flagged by the scan and
raises the ValueError a non-finite matrix raises, where that one is raised; upstream would carry the big integer
further, into the MIDI program or note number, before failing there.

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
from functools import cached_property

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
        raise ValueError("generated matrix holds non-finite values or an instrument / note-level entry whose product "
                         "with 126 does not fit an int32: the DES prologue is defined for finite inputs below that only")


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


BACK_ENDS = ("des", "des_batch", "des_device")


def check_back_end(name, who, exc=ops.GdmError):
    """Raise ``exc`` unless ``name`` is a built-in back end; ``who`` opens the message ("f: unknown back end")."""
    if name not in BACK_ENDS:
        names = ", ".join(f'"{n}"' for n in BACK_ENDS[:-1])
        raise exc(f"{who} {name!r} (the built-in ones are {names} and \"{BACK_ENDS[-1]}\")")


@dataclass(frozen=True)
class Route:
    """What differs between the two bridges; everything below is written once over it (``MIDI``, ``WAV``)."""
    inputs: str               # what the error for a host tensor calls the input
    aux_rows: int             # dim = size - aux_rows
    scan_args: dict           # keyword arguments of ops.des_scan
    host_fields: tuple        # (key in h, key of the scan) of what the host draws and specs read
    draws: object             # (h, i) -> (src, cols, seeds): sample i's draws from numpy's global stream
    spec: object              # (h, i, routing, src, seeds, instrument) -> DesSpec
    draws_id: int             # ops.DES_DRAWS_*
    params: str               # key in a device scan of the ``params`` argument of ops.des_draws

    def scan(self, g, size, g2=None, *, download=True, tail=False):
        """Validate the inputs and launch the RNG-free scan -> the dict ``h`` every later stage reads: ``g1``, ``size``,
        ``dim``, ``b``; with ``download`` the host copies the numpy draws and specs need (``g2``, ``inst``, ``notes``,
        ``zmask``, ``thr``, ``aux``: whichever the route has) after a finite check; without, nothing is read back and
        ``h`` holds the device tensors (``g2``, ``scan``, ``aux``, ``flags``).  ``tail``: gen2_output[10:16] will be
        read (the built-in MIDI back ends)."""
        g = g.detach() if isinstance(g, torch.Tensor) else torch.as_tensor(np.asarray(g))
        if not g.is_cuda:
            raise ops.GdmError(f"matrix_sim_process runs the prologue on a HIP device; move the {self.inputs} there")
        if tail and g2.shape[1] < 16:
            raise ops.GdmError("matrix_to_midi: gen2_output needs at least 16 columns (gen2_output[10:16] drive the "
                               "MIDI)")
        g = g.float()
        h = {"g1": g, "size": size, "dim": size - self.aux_rows, "b": g.shape[0]}
        if g2 is not None and not download:
            h["g2"] = g2.detach().to(device=g.device, dtype=torch.float32).contiguous()
            if h["g2"].dim() != 2 or h["g2"].shape[0] != h["b"] or h["g2"].shape[1] < 7:
                raise ops.GdmError("des_device: gen2_output must be (B, n) with n >= 7 (columns 1..6 drive the "
                                   "simulator)")
        scan = ops.des_scan(g, size, h["dim"], **self.scan_args)
        if not download:
            h.update(scan=scan, aux=scan["aux"], flags=scan["flags"])
            return h
        if g2 is not None:
            h["g2"] = g2.detach().float().cpu().numpy()
        h.update((key, scan[name].cpu().numpy()) for key, name in self.host_fields)
        _check_finite(scan["flags"].cpu().numpy())
        return h

    def specs(self, h, instrument=None):
        """The reference's order: a sample's spec is complete (and handed to the caller, who simulates) before the
        next sample draws anything.  One one-sample routing launch each."""
        for i in range(h["b"]):
            src, cols, sd = self.draws(h, i)
            routing = _routing(h, slice(i, i + 1), src[None], cols[None]).cpu().numpy()[0]
            yield self.spec(h, i, routing, src, sd, instrument)

    def batched(self, h, instrument=None):
        """A downloaded scan -> BatchedPrologue: ALL host draws in the reference's order with a snapshot of numpy's
        stream after each sample's reseed, then one routing launch whose output stays on the device."""
        b, dim = h["b"], h["dim"]
        src_all = np.zeros((b, dim), dtype=bool)
        cols_all = np.empty((b, dim), dtype=np.int32)
        seeds, states = [], []
        for i in range(b):                                               # global-RNG order of the reference, per sample
            src_all[i], cols_all[i], sd = self.draws(h, i)
            seeds.append(sd)
            states.append(np.random.get_state())                         # where simulation i starts
        return BatchedPrologue(self, h, _routing(h, slice(None), src_all, cols_all), src_all, seeds, states, instrument)

    def device(self, h, instrument=None, base=None):
        """A scan left on the device -> DevicePrologue: ``ops.des_draws`` (sample i on ``RandomState(base[i])``;
        base=None: ``draw_base_seeds``, the one call on numpy's global stream), routing.  Nothing is read back."""
        b, dim, dev = h["b"], h["dim"], h["g1"].device
        if dim > ops.DES_DRAWS_MAX_DIM:
            raise ops.GdmError(f"des_device: at most {ops.DES_DRAWS_MAX_DIM} nodes (a row's candidates are one 64-bit "
                               "word)")
        override = _instrument_override(instrument, b)
        base = draw_base_seeds(b) if base is None else np.ascontiguousarray(base, dtype=np.uint32).reshape(b)
        draws = ops.des_draws(self.draws_id, h["size"], dim, torch.from_numpy(base.view(np.int32)).to(dev), h["scan"],
                              h[self.params], None if override is None else torch.from_numpy(override).to(dev))
        return DevicePrologue(h, base, draws, ops.des_routing(h["g1"], h["size"], dim, draws["src"], draws["cols"]))

    def prologue(self, back_end, g, size, g2=None, instrument=None, *, tail=False):
        """Scan and prologue of "des_batch" or "des_device" -> BatchedPrologue or DevicePrologue."""
        download, make = _PROLOGUES[back_end]
        return make(self, self.scan(g, size, g2, download=download, tail=tail), instrument)


_PROLOGUES = {"des_batch": (True, Route.batched), "des_device": (False, Route.device)}
MIDI = Route("generator outputs", 3, {"note_mod": True},
             (("inst", "instruments"), ("notes", "note_levels"), ("zmask", "zero_mask")),
             _midi_draws, _midi_spec, ops.DES_DRAWS_MIDI, "g2")
WAV = Route("generated matrices", 5, {"threshold": 0.75, "norm_aux": True},
            (("thr", "thr_mask"), ("inst", "instruments"), ("notes", "note_levels"), ("zmask", "zero_mask"),
             ("aux", "aux")), _wav_draws, _wav_spec, ops.DES_DRAWS_WAV, "aux")


def _routing(h, rows, src, cols):
    """des_routing for the samples ``rows`` (a slice) of the scanned batch: src (n,dim) bool, cols (n,dim) int32 host
    arrays -> (n,dim,dim) f64 on the device."""
    dev = h["g1"].device
    return ops.des_routing(h["g1"][rows], h["size"], h["dim"],
                           torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(dev))


# "des_batch" simulates on the device from this batch size on and with the host mirror below it.  The two give the same
# bits, so the choice is one of speed only: the launch takes 8-10 ms whatever B is (one wave per sample, a latency-bound
# chain), the sequential host mirror 0.15 ms (15 nodes) to 0.22 ms (61 nodes) per sample plus the transfers of the
# routing matrices and the logs -- measured crossover B = 45-55.
DES_BATCH_DEVICE_MIN_B = 48


def _per_sample(build, dtype):
    """A BatchedPrologue array, built from the samples' DesSpecs when it is first read (``specs()`` needs none)."""
    return cached_property(lambda self: np.ascontiguousarray([build(sp) for sp in self._heads], dtype=dtype))


class BatchedPrologue:
    """What the batched prologue leaves, each product where its consumer needs it: ``routing`` (B,dim,dim) fp64 on the
    device; ``loc``, ``scale`` (B,dim) f64, ``queue_cap`` (B,dim) i32, ``seed``, ``customers`` (B) i64, ``instruments``,
    ``note_levels`` (B,dim) i32 on the host (built with the float32 arithmetic of ``_midi_spec`` / ``_wav_spec``);
    ``states``: the B snapshots of ``np.random.get_state()`` taken right after each sample's reseed; ``h``: the scan.
    The consumers' surface is DevicePrologue's: ``simulate_on``, ``readback_words``, ``check``, ``check_rec_ptr``."""
    check_rec_ptr = True                  # the log may come from the host mirror: the consumer checks its row pointers

    def __init__(self, route, h, routing, src, seeds, states, instrument=None):
        self.route, self.h, self.routing, self.states = route, h, routing, states
        self._src, self._seeds, self._instrument = src, seeds, instrument

    def _spec(self, i, routing):
        return self.route.spec(self.h, i, routing, self._src[i], self._seeds[i], self._instrument)

    _heads = cached_property(lambda self: [self._spec(i, None) for i in range(self.h["b"])])   # the per-node parameters
    loc = _per_sample(lambda sp: [float(d[1]) for d in sp.distributions], np.float64)
    scale = _per_sample(lambda sp: [float(d[2]) for d in sp.distributions], np.float64)
    queue_cap = _per_sample(lambda sp: sp.queue_list, np.int32)
    seed = _per_sample(lambda sp: int(np.asarray(sp.seeds).reshape(-1)[0]), np.int64)
    customers = _per_sample(lambda sp: sp.num_customers, np.int64)
    instruments = _per_sample(lambda sp: [int(x) for x in sp.instruments], np.int32)
    note_levels = _per_sample(lambda sp: [int(x) for x in sp.note_levels], np.int32)

    def specs(self):
        """The DesSpecs ``midi_prologue`` / ``wav_prologue`` return (downloads the routing matrices)."""
        routing = self.routing.cpu().numpy()
        return [self._spec(i, routing[i]) for i in range(self.h["b"])]

    def simulate(self, device, max_events=200000, max_records=5001, min_device_b=0):
        """``gdm_des_run_batch`` (device: a HIP device) or the host mirror with portable math (device=None), every
        sample from its snapshot -> simulation_v3.BatchLog."""
        from . import simulation_v3
        return simulation_v3.run_batch_auto(
            self.routing, self.loc, self.scale, self.queue_cap, self.seed, self.customers, self.states, device=device,
            min_device_b=min_device_b, max_events=max_events, max_records=max_records,
            max_queue_cap=max(1, int(self.queue_cap.max())))

    def simulate_on(self, device, max_events=200000, max_records=5001):
        """``simulate`` for the bridges: a BatchLog of tensors on ``device`` either way -- from the kernel when the batch
        holds at least DES_BATCH_DEVICE_MIN_B samples, else from the host mirror (same bits), uploaded once."""
        return self.simulate(device, max_events, max_records, min_device_b=DES_BATCH_DEVICE_MIN_B)

    def readback_words(self):
        """Nothing of the prologue is left to read back: the host draws raised what there was to raise."""
        return {}

    def check(self, words, raise_draws=True):
        return ()


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
    back: ``status`` and ``flags`` travel with the consumer's one read-back (``readback_words`` / ``check``)."""
    check_rec_ptr = False                 # the log comes from the kernel, and checking would need a read-back

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

    def readback_words(self):
        """int32 device tensors to add to the consumer's read-back, by name: draw status, scan flags."""
        return {"draw_status": self.status, "flags": self.flags}

    def check(self, words, raise_draws=True):
        """After the read-back: ValueError for a non-finite generated matrix, then (``raise_draws``) what the
        reference raises for the first sample with a draw status.  -> the draw status words (B,)."""
        _check_finite(words["flags"])
        for i in np.flatnonzero(words["draw_status"]) if raise_draws else ():
            raise draws_error(words["draw_status"][i])
        return words["draw_status"]


def _read_back(tensors):
    """name -> integer device tensor, in order -> name -> int32 numpy view of the same shape: ONE transfer for all."""
    host = torch.cat([t.reshape(-1).to(torch.int32) for t in tensors.values()]).cpu().numpy()
    ends = np.cumsum([t.numel() for t in tensors.values()])
    return {name: host[end - t.numel():end].reshape(tuple(t.shape)) for (name, t), end in zip(tensors.items(), ends)}


def batched_prologue_midi(gen1_output, gen2_output, adj_size=(32, 32), instrument=None):
    """``midi_prologue`` with its products left where "des_batch" needs them -> BatchedPrologue."""
    return MIDI.prologue("des_batch", gen1_output, adj_size[0], gen2_output, instrument)


def batched_prologue_wav(matrices, size=20, use_same_instrument=None):
    """``wav_prologue`` with its products left where "des_batch" needs them -> BatchedPrologue."""
    return WAV.prologue("des_batch", matrices, size, None, use_same_instrument)


def device_prologue_midi(gen1_output, gen2_output, adj_size=(32, 32), instrument=None, *, base=None):
    """The MIDI route's prologue entirely on the device: scan, ``ops.des_draws`` (sample i on the stream
    ``RandomState(base[i])``; base=None: ``draw_base_seeds``, the one call on numpy's global stream), routing.  No host
    synchronisation, nothing read back -> DevicePrologue."""
    return MIDI.device(MIDI.scan(gen1_output, adj_size[0], gen2_output, download=False), instrument, base)


def device_prologue_wav(matrices, size=20, use_same_instrument=None, *, base=None):
    """The wav route's prologue entirely on the device (see ``device_prologue_midi``) -> DevicePrologue."""
    return WAV.device(WAV.scan(matrices, size, download=False), use_same_instrument, base)


def midi_prologue(gen1_output, gen2_output, adj_size=(32, 32), instrument=None):
    """Device-batched head of matrix_to_midi: gen1_output (B,1,S,S), gen2_output (B,n2) device tensors -> [DesSpec].
    All draws are made before the first spec is returned (see the module docstring)."""
    return batched_prologue_midi(gen1_output, gen2_output, adj_size, instrument).specs()


def wav_prologue(matrices, size=20, use_same_instrument=None):
    """Device-batched head of matrix_to_wav: matrices (B,size,size) device tensor -> [DesSpec].  All draws are made
    before the first spec is returned (see the module docstring)."""
    return batched_prologue_wav(matrices, size, use_same_instrument).specs()


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
        check_back_end(simulate, "matrix_to_midi: unknown back end")
        if simulate == "des":
            return _matrix_to_midi_des(gen1_output, gen2_output, adj_size, instrument, start, end, generate,
                                       return_tensor, midi_path, max_events)
        return _matrix_to_midi_des_batch(simulate, gen1_output, gen2_output, adj_size, instrument, start, end, generate,
                                         return_tensor, midi_path, max_events)
    if return_tensor:
        raise ops.GdmError("matrix_to_midi: return_tensor needs the built-in back end (simulate=\"des\")")
    h = MIDI.scan(gen1_output, adj_size[0], gen2_output)
    g2 = h["g2"]
    midi_rolls, failed = [], 0
    for index, spec in enumerate(MIDI.specs(h, instrument)):
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
    h = MIDI.scan(gen1_output, adj_size[0], gen2_output, tail=True)
    logs, ok, insts, notes, reasons = [], [], [], [], []
    for spec in MIDI.specs(h, instrument):
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


def _des_batch_run(simulate, gen1_output, gen2_output, adj_size, instrument, start, end, generate, max_events,
                   raise_draws=True):
    """The body "des_batch" and "des_device" share between ``matrix_to_midi`` and ``matrix_to_midis``: batched or
    device prologue, simulator, one ``des_log_to_roll`` launch, ONE read-back -> (planes (B,2,128,W) on the device;
    the words read back, int32 host arrays by name: status, track_len, good, save, stop (B,) and tracks (B, cap, 4);
    the draw status words ``pro.check`` returns)."""
    from . import sim_log_to_midi
    _check_midi_window(start, end)
    pro = MIDI.prologue(simulate, gen1_output, adj_size[0], gen2_output, instrument, tail=True)
    dev = pro.h["g1"].device
    log = pro.simulate_on(dev, max_events=max_events, max_records=sim_log_to_midi.MAX_LINES + 1)
    good = (log.stop_reason != ops.DES_STOP_ERROR) & (log.stop_reason != ops.DES_STOP_BUDGET)
    lines = torch.clamp(log.n_records, max=sim_log_to_midi.MAX_LINES + 1)             # lines_read, on the device
    save = (good & ((lines % 100 == 0) | bool(generate))).to(torch.int32)
    planes, track, track_len, status = ops.des_log_to_roll(
        log.value, log.event_id, log.node, log.kind, log.rec_ptr, _on(pro.h["g2"][:, 10:], dev),
        _on(pro.instruments, dev), _on(pro.note_levels, dev), save, start, end, check_rec_ptr=pro.check_rec_ptr)
    # the one read-back: stop reasons (and the device prologue's status words) with the tracks
    words = _read_back({"status": status, "track_len": track_len, "good": good, "save": save, "stop": log.stop_reason,
                        **pro.readback_words(), "tracks": track})
    return planes, words, pro.check(words, raise_draws)


def _matrix_to_midi_des_batch(simulate, gen1_output, gen2_output, adj_size, instrument, start, end, generate,
                              return_tensor, midi_path, max_events):
    from . import sim_log_to_midi
    planes, words, _draw_status = _des_batch_run(simulate, gen1_output, gen2_output, adj_size, instrument, start, end,
                                                 generate, max_events)
    status, track_len, good, save, tracks = (words[k] for k in ("status", "track_len", "good", "save", "tracks"))
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
    check_back_end(simulate, "matrix_to_midis: unknown back end")
    b = gen1_output.shape[0]
    if midi_paths is not None and len(midi_paths) != b:
        raise ops.GdmError(f"matrix_to_midis: {len(midi_paths)} midi_paths for {b} samples")
    if simulate != "des":
        planes, words, draw_status = _des_batch_run(simulate, gen1_output, gen2_output, adj_size, instrument, start, end,
                                                    True, max_events, raise_draws=False)
        status = words["status"]
        tracks = [words["tracks"][i, :words["track_len"][i]].copy() for i in range(b)]
        reasons = [None if words["good"][i] else simulation_v3.STOP_REASONS[int(words["stop"][i])] for i in range(b)]
        for i in np.flatnonzero(draw_status):
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
    """The built-in batched back ends behind matrix_to_wav: Batched- or DevicePrologue -> ((B, 128, 216) dB device tensor, (notes,
    n_notes, clip_len) device tensors).  Simulator, log -> notes, synth and mel are enqueued without a read-back in
    between; the status words and stop reasons come back once, and a sample the reference would raise for raises."""
    from . import sim_log_process_music, simulation_v3, util
    dev = pro.h["g1"].device
    log = pro.simulate_on(dev, max_events=max_events, max_records=sim_log_process_music.MAX_LINES + 1)
    notes, n_notes, clip_len, status = ops.des_log_to_notes(log.value, log.event_id, log.node, log.kind, log.rec_ptr,
                                                            _on(pro.note_levels, dev), check_rec_ptr=pro.check_rec_ptr)
    frames = ops.synth_frames(notes, n_notes, clip_len)
    mel = util._db_from_frames(frames, pro.h["b"], ops.SYNTH_FRAMES, ops.SYNTH_RATE, ops.SYNTH_NFFT, 128, 20, 8300, 80)
    words = _read_back({"status": status, "stop": log.stop_reason, **pro.readback_words()})
    pro.check(words)                             # the device prologue's own errors come first, as in the reference
    simulation_v3.raise_for_stop(words["stop"], "matrix_to_wav", "sample")
    sim_log_process_music.raise_for_status(torch.from_numpy(words["status"]))
    return mel, (notes, n_notes, clip_len)


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
    if isinstance(simulate, str):
        mel, _notes = matrices_to_mel(matrices, size, use_same_instrument, simulate=simulate, max_events=max_events)
        return mel[:, :, start:end].to(device)
    specs = WAV.specs(WAV.scan(matrices, size), use_same_instrument)
    spectrograms = [torch.as_tensor(simulate(spec, index=i)) for i, spec in enumerate(specs)]
    return torch.stack([s[:, start:end] for s in spectrograms]).to(device)


def matrices_to_mel(matrices, size=20, use_same_instrument=None, *, simulate, max_events=200000):
    """``matrix_to_wav`` with a built-in back end, before its ``[start:end]`` cut and keeping the note lists (what the
    MIDI and WAV files of a clip are written from): -> (mel (B, 128, 216) dB on the matrices' device, (notes, n_notes,
    clip_len) device tensors)."""
    check_back_end(simulate, "matrix_to_wav: unknown back end")
    if simulate != "des":
        return _batch_to_mel(WAV.prologue(simulate, matrices, size, None, use_same_instrument), max_events)
    h = WAV.scan(matrices, size)
    return _specs_to_mel(WAV.specs(h, use_same_instrument), h["g1"].device, max_events)


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
