"""Drop-in surface of the reference's stand-alone demo (SIMULATOR/simulation_to_wav.py) on MI355X:

    sim_to_wav(matrices=[None], size=32, use_same_instrument=None, sound_font='FluidR3_GM.sf2', *, simulate="des",
               out_dir="adj_sim_outputs", max_events=200000, max_seconds=None, device="cuda", return_batch=False)

random (or given) matrix -> DES -> MIDI -> WAV, for a batch of matrices.  Per matrix it writes
``<out_dir>/wav/output_<index>.wav`` and ``<out_dir>/midi/output_<index>.mid``; ``<out_dir>/midi/output.mid`` is the
last sample's file (upstream overwrites that one path).  Returns the list of WAV paths, or with ``return_batch=True`` a
``SimWavBatch``.  ``python -m gan_des_midi_music_gen_amd.simulation_to_wav --help`` is the command line.

The chain: ``ops.s2w_prologue`` (csrc/s2w_prologue.hip: the demo's own matrix prologue, float64, up to 256 x 256) ->
the DES core -> ``ops.des_log_to_notes_pc`` (csrc/des_notes.hip: the demo's own MidiGenerator, whose program_change
lines are live) -> the MIDI writer and ``ops.synth_windows_gm`` (csrc/synth.hip: the integer synth with one timbre per
General MIDI family, rendered in bounded chunks).

``simulate`` names the back end as the two bridges do:
  "des"        the reference's loop, one matrix after another on numpy's GLOBAL stream: the ``None`` matrix is drawn
               with ``np.random.rand`` exactly as lines 12-22 do, then the reseed pair (76-77), then ``gdm_des_run`` on
               the global stream.  Under ``np.random.seed(k)`` the event log is the reference's, record for record
               (tests/golden/sim_to_wav.npz).  One prologue launch per matrix: the next draw waits for the simulation.
  "des_batch"  sample b gets a stream of its own: ``base = np.random.randint(0, 2**32, size=B)`` once from the global
               stream; on ``np.random.RandomState(base[b])``, on the host and with numpy itself, the ``None``-matrix
               draws and the reseed pair; the simulation starts from the state of ``RandomState(seed1)`` after its one
               ``randint``.  One prologue launch for the batch; the simulations run through ``simulation_v3``'s batch
               entries with the split the bridges use (the kernel from ``matrix_sim_process.DES_BATCH_DEVICE_MIN_B``
               samples on, the host mirror with the same bits below it) -- and on the host for more than 128 nodes
               (``GDM_DES_BATCH_MAX_DIM``).  Portable math: the event structure is the reference's, values differ in
               their last bits, and the log is capped at 5001 records (all the reader looks at).
  "des_device" accepted as an alias of "des_batch" for now: the per-sample draws are host numpy either way.

Kept as upstream:
  * ``len(sources) == 0`` tests np.where's 1-tuple and is never true: with no entry of the source row above 0.75 there
    is no source, the log is empty, the MIDI file holds no note and the WAV is the blank clip ``datasets.midi_notes``
    defines for a file without notes (five seconds of silence);
  * instruments and note levels are ``int(x * 127)`` (``matrix_to_wav`` uses 126 and ``abs``; this path does not);
  * a row is divided by Python's sequential ``sum`` over ALL ``size`` columns -- the five parameter columns, which a
    given matrix may fill, included -- after every column whose source-row entry passes 0.75 and the diagonal have
    been zeroed; only afterwards are the first ``dim = size - 5`` columns sliced;
  * queue capacity 127, ``number_of_customers=1000``;
  * MidiGenerator emits a program_change before every note_on and every note_off with the same delta time, so every
    delta counts twice; ``generate_midi`` is never called, so the file has no header messages and plays at the default
    tempo 500 000 (the recording says so): one tick is 735 / 16 samples, the rule ``datasets.midi_notes`` applies to
    the written file.
Different on purpose:
  * no NaN repair and no NaN simulation: a row whose sum is 0 or not finite makes that sample raise ValueError with
    its index before it is simulated (what the reference does with NaN probabilities is not pinned);
  * ``max_sim_time`` is wall clock upstream; here the cap is ``max_events``, as everywhere in ``simulation_v3``;
  * ``sound_font`` is accepted and unused: the synth is defined here (include/gdm.h), FluidSynth is not imitated;
  * valid sizes are 6 .. 256 (1 .. 251 nodes); anything else raises ValueError on the host;
  * ``logs/simulation.log`` is not written: the records go to the device as arrays.
"""
import argparse
import os

import numpy as np
import torch

from . import matrix_sim_process as msp, ops, sim_log_process_music, sim_log_to_midi, simulation_v3, util
from .matrix_sim_process import BACK_ENDS, check_back_end

NUM_AUG = 5
QUEUE_CAPACITY = 127
NUMBER_OF_CUSTOMERS = 1000


class SimWavBatch:
    """What ``sim_to_wav(return_batch=True)`` returns, like ``SIMNN.SongBatch``: ``notes`` (B, 5000, 5) int64 rows
    (on_tick, off_tick, pitch, velocity, program), ``n_notes`` (B,) int32, ``clip_len`` (B,) int64 in samples (0: a
    blank clip), ``programs`` (B, dim) int32 -- device tensors --, ``midi_paths`` and ``wav_paths``."""

    def __init__(self, notes, n_notes, clip_len, programs, midi_paths, wav_paths):
        self.notes, self.n_notes, self.clip_len, self.programs = notes, n_notes, clip_len, programs
        self.midi_paths, self.wav_paths = midi_paths, wav_paths


def draw_matrix(size, rand=None):
    """The ``None`` matrix of lines 12-22 on ``rand`` (default ``np.random.rand``, the global stream)."""
    rand = np.random.rand if rand is None else rand
    dim = size - NUM_AUG
    matrix = rand(size, size)
    matrix[dim:, :] = 0
    matrix[:, dim:] = 0
    for r in range(NUM_AUG):
        matrix[dim + r, :dim] = rand(dim)
    return matrix


def _as_matrix(matrix, size, index):
    m = np.array(matrix, dtype=np.float64)
    if m.shape != (size, size):
        raise ValueError(f"sim_to_wav: matrix {index} has shape {m.shape}, expected ({size}, {size})")
    return m


def _override(use_same_instrument, b, dev):
    if use_same_instrument is None:
        return None
    return torch.full((b,), int(use_same_instrument), dtype=torch.int32, device=dev)


def _refuse(status, first_index=0):
    for i, code in enumerate(status.tolist()):
        if code:
            raise ValueError(f"sim_to_wav: matrix {first_index + i} has a row whose sum is 0 or not finite: its routing "
                             "probabilities are undefined and it is not simulated")


def notes_to_track_pc(notes):
    """(n, 5) (on_tick, off_tick, pitch, velocity, program) -> the (kind, a, b, delta time) track ``write_midi`` takes,
    message for message what the demo's MidiGenerator appends: program_change, note_on, program_change, note_off per
    note, each pair sharing its delta; no header."""
    track, t = [], 0
    for on, off, pitch, vel, prog in np.asarray(notes, dtype=np.int64).reshape(-1, 5).tolist():
        d_on, d_off = (on - t) // 2, (off - on) // 2
        track += [(sim_log_to_midi.PROGRAM_CHANGE, prog, 0, d_on), (sim_log_to_midi.NOTE_ON, pitch, vel, d_on),
                  (sim_log_to_midi.PROGRAM_CHANGE, prog, 0, d_off), (sim_log_to_midi.NOTE_OFF, pitch, vel, d_off)]
        t = off
    return track


def _simulate_des(matrices, size, use_same_instrument, max_events, dev):
    """The reference's loop -> (logs, instruments (B, dim) i32 device, note_levels (B, dim) i32 device)."""
    dim = size - NUM_AUG
    logs, insts, levels = [], [], []
    for index, matrix in enumerate(matrices):
        m = draw_matrix(size) if matrix is None else _as_matrix(matrix, size, index)
        pro = ops.s2w_prologue(torch.from_numpy(m).to(dev)[None].contiguous(), _override(use_same_instrument, 1, dev))
        _refuse(pro["status"].cpu(), index)
        np.random.seed(np.random.randint(0, 99999, size=1))                              # lines 76-77
        seeds = np.random.randint(0, 99999, size=1)
        loc, scale = pro["loc"][0].cpu().numpy(), pro["scale"][0].cpu().numpy()
        sim = simulation_v3.Sim(pro["adj"][0].cpu().numpy(), [["normal", loc[i], scale[i]] for i in range(dim)],
                                [QUEUE_CAPACITY] * dim, seeds=seeds, generate_log=False, animation=False,
                                record_history=False, logging_mode='Music', max_events=max_events)
        sim.run(number_of_customers=NUMBER_OF_CUSTOMERS)
        logs.append(sim.music_log)
        insts.append(pro["instruments"][0])
        levels.append(pro["note_levels"][0])
    return logs, torch.stack(insts).contiguous(), torch.stack(levels).contiguous()


def batch_draws(matrices, size, base):
    """The host draws of "des_batch": sample b on ``np.random.RandomState(base[b])`` -> (matrices (B, size, size)
    float64, seed (B,) int64, states: B generator states the simulations start from)."""
    out, seeds, states = [], [], []
    for index, matrix in enumerate(matrices):
        rs = np.random.RandomState(int(base[index]))
        out.append(draw_matrix(size, rs.rand) if matrix is None else _as_matrix(matrix, size, index))
        inner = np.random.RandomState(rs.randint(0, 99999, size=1))
        seeds.append(int(inner.randint(0, 99999, size=1)[0]))
        states.append(inner.get_state())
    return np.ascontiguousarray(out, dtype=np.float64), np.asarray(seeds, dtype=np.int64), states


def _simulate_batch(matrices, size, use_same_instrument, max_events, dev):
    """"des_batch" -> (simulation_v3.BatchLog of device tensors, instruments, note_levels (B, dim) i32 device)."""
    b = len(matrices)
    base = np.random.randint(0, 2 ** 32, size=b)
    ms, seed, states = batch_draws(matrices, size, base)
    pro = ops.s2w_prologue(torch.from_numpy(ms).to(dev), _override(use_same_instrument, b, dev))
    _refuse(pro["status"].cpu())
    customers = np.full(b, NUMBER_OF_CUSTOMERS, dtype=np.int64)
    log = simulation_v3.run_batch_auto(pro["adj"], pro["loc"], pro["scale"], pro["queue_cap"], seed, customers, states,
                                       device=dev, min_device_b=msp.DES_BATCH_DEVICE_MIN_B, max_events=max_events,
                                       max_records=sim_log_to_midi.MAX_LINES + 1, max_queue_cap=QUEUE_CAPACITY)
    simulation_v3.raise_for_stop(log.stop_reason.cpu(), "sim_to_wav", "matrix")
    return log, pro["instruments"], pro["note_levels"]


def _render(rows, count, total, wav_path, max_seconds, dev):
    """Clip ``rows`` ((count, 5) device rows in ticks) as a mono 16-bit 44 100 Hz WAV file of ``total`` samples; a clip
    without notes is the blank one ``datasets.midi_notes`` defines for such a file."""
    if count:
        mul, div = ops.tick_rule()
        notes = rows.clone()
        notes[:, :2] = torch.div(notes[:, :2] * mul, div, rounding_mode="floor")        # ticks -> samples, exact
        release = ops.synth_gm_tables(dev)[1][:, 1].to(torch.int64)
        end_max = torch.cummax(notes[:, 1] + release[(notes[:, 4] & 127) >> 3], dim=0).values.contiguous()
        note_ptr = torch.tensor([0, count], dtype=torch.int64, device=dev)
        win_clip = torch.zeros(1, dtype=torch.int32, device=dev)

    def render(first, chunk):
        start = torch.full((1,), first, dtype=torch.int64, device=dev)
        return ops.synth_windows_gm(notes, end_max, note_ptr, win_clip, start, chunk)[0, :chunk]
    return util.write_wav_chunks(wav_path, total, render, blank=count == 0, max_seconds=max_seconds)


def sim_to_wav(matrices=[None], size=32, use_same_instrument=None, sound_font='FluidR3_GM.sf2', *, simulate="des",
               out_dir="adj_sim_outputs", max_events=200000, max_seconds=None, device="cuda", return_batch=False):
    """See the module docstring.  matrices: ``(size, size)`` array-likes or None (a random matrix is drawn)."""
    check_back_end(simulate, "sim_to_wav: unknown back end", ValueError)
    size = int(size)
    if not ops.S2W_MIN_SIZE <= size <= ops.S2W_MAX_SIZE:
        raise ValueError(f"sim_to_wav: size {size} (valid sizes are {ops.S2W_MIN_SIZE} .. {ops.S2W_MAX_SIZE}: 1 .. "
                         f"{ops.S2W_MAX_SIZE - NUM_AUG} nodes)")
    matrices = list(matrices)
    if len(matrices) == 0:
        raise ValueError("sim_to_wav: no matrices")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ops.GdmError("sim_to_wav runs on a HIP device; there is no CPU path")
    if simulate == "des":
        logs, inst, levels = _simulate_des(matrices, size, use_same_instrument, max_events, dev)
        _logs, _dev, _up, records = sim_log_to_midi._upload_logs(logs, dev, "sim_to_wav")
        rec, check = records(), True
    else:
        log, inst, levels = _simulate_batch(matrices, size, use_same_instrument, max_events, dev)
        rec, check = (log.value, log.event_id, log.node, log.kind, log.rec_ptr), True
    notes, n_notes, clip_len, status = ops.des_log_to_notes_pc(*rec, inst, levels, check_rec_ptr=check)
    sim_log_process_music.raise_for_status(status)
    counts, lengths = n_notes.cpu().tolist(), clip_len.cpu().tolist()
    midi_paths, wav_paths = [], []
    for i in range(len(matrices)):
        track = notes_to_track_pc(notes[i, :counts[i]].cpu().numpy())
        midi_paths.append(sim_log_to_midi.write_midi(track, os.path.join(out_dir, "midi", f"output_{i}.mid")))
        if i == len(matrices) - 1:
            sim_log_to_midi.write_midi(track, os.path.join(out_dir, "midi", "output.mid"))
        wav_paths.append(os.path.join(out_dir, "wav", f"output_{i}.wav"))
        _render(notes[i, :counts[i]], counts[i], lengths[i], wav_paths[-1], max_seconds, dev)
    if return_batch:
        return SimWavBatch(notes, n_notes, clip_len, inst, midi_paths, wav_paths)
    return wav_paths


def main(argv=None):
    ap = argparse.ArgumentParser(description="random matrix -> DES -> MIDI -> WAV (the reference's sim_to_wav demo)")
    ap.add_argument("-n", type=int, default=1, help="number of random matrices")
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--instrument", type=int, default=None, help="use_same_instrument: one program for every node")
    ap.add_argument("--simulate", choices=BACK_ENDS, default="des")
    ap.add_argument("--out-dir", default="adj_sim_outputs")
    ap.add_argument("--max-seconds", type=float, default=None)
    ap.add_argument("--seed", type=int, default=None, help="np.random.seed before the first draw")
    a = ap.parse_args(argv)
    if a.seed is not None:
        np.random.seed(a.seed)
    batch = sim_to_wav([None] * a.n, size=a.size, use_same_instrument=a.instrument, simulate=a.simulate,
                       out_dir=a.out_dir, max_seconds=a.max_seconds, return_batch=True)
    for midi, wav in zip(batch.midi_paths, batch.wav_paths):
        print(midi)
        print(wav)


if __name__ == "__main__":
    main()
