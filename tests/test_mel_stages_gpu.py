"""GPU: the mel featuriser's kernels (csrc/mel.hip) stage by stage against float64.  tests/mel_ref.py states the
references, the derived bounds, the case tables and the planted faults; tests/test_mel_ref.py proves on the CPU that
those tables reject every planted fault.

  gdm_stft_frames: bit-equal to the reflect-padded gather (NaN payloads, -0 and denormals included) at one chunk per
    row, the minimum length, hop 1 and hop > n_fft, the last frame centred on L, a strided batch with NaN behind every
    row, two trips of the grid-stride loop; its refusals leave the output untouched.
  gdm_power_spectrum: within 3 u of re^2 + im^2 on a caller-owned buffer prefilled with NaN between sentinel rows: pad
    columns +0, nothing outside written, overflow to +inf and NaN kept, two trips.
  gdm_power_to_db: within LOG10_ULPS ulp of 10 log10(max(p, amin)) and of the floor, for every shape class of its
    one-workgroup loop (n below, at and above multiples of 1024, frames and n_mels coprime both ways), top_db 80, 0 and
    None, many small windows, both sides of the LDS limit; +inf and NaN as torch treats them.
  the chain (util.melspectrogram_db_batch) at three small geometries and the reference one: frames bit-equal, spectrum,
    power, mel power and dB inside the propagated bounds, per element.  The stages are called here the way
    util._db_from_frames calls them, to keep the mel power; the test also asserts that what it assembles equals
    util._db_from_frames and util.melspectrogram_db_batch bit for bit, so the two cannot drift apart.

helpers.record("mel_stage_vs_float64", ...) keeps each test's worst |err| / bound.  Measured on MI355X: frames
bit-equal everywhere; power 0.66; dB 0.51 (2 of the 4 ulp); chain 0.09 spectrum, 0.07 power, 0.06 mel power, 0.20 dB
(the small geometries; 0.012 / 0.011 / 0.006 / 0.16 at the reference geometry, where the GEMM bound grows with K).
Before the kernel told NaN by its bits, the six NaN cases failed: the NaN came out as -100 dB, or as the floor.  The
whole file -- 44 tests -- takes 3.3 s, the slowest test 0.4 s.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import _lib, ops, util  # noqa: E402
from gan_des_midi_music_gen_amd.ops import F32  # noqa: E402

import mel_ref as mr  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"


def _ptr(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _last_error():
    return _lib.load().gdm_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("c", mr.FRAME_CASES, ids=[c.name for c in mr.FRAME_CASES])
def test_stft_frames_bit_exact(c):
    bits = mr.frame_input(c)
    buf = torch.from_numpy(np.array(bits, copy=True)).view(torch.float32).to(DEV)
    x = buf[:, :c.L]
    assert x.stride(0) == c.L + c.extra
    out, frames = ops.stft_frames(x, c.hop, c.n_fft)
    assert frames == c.frames and out.shape == (c.B * c.frames, c.n_fft)
    fails = mr.check_frames(out, mr.frames_ref(c, bits), what=c.name)
    assert not fails, "\n".join(fails)
    assert np.array_equal(buf.cpu().numpy().view(np.int32), bits), "the input was written to"


def test_stft_frames_refusals_leave_the_output_untouched():
    lib = _lib.load()
    n_fft, hop, L = 8, 2, 20
    frames = 1 + L // hop
    x = torch.randn(L, device=DEV)
    out = torch.full(((frames + 2) * n_fft,), mr.SENTINEL, device=DEV)
    ok = (_ptr(x), 1, L, L, hop, n_fft, frames, _ptr(out))
    refusals = [
        ("L = n_fft / 2", (_ptr(x), 1, n_fft // 2, L, hop, n_fft, 1, _ptr(out)), "reflect padding needs more than"),
        ("one frame too many", (_ptr(x), 1, L, L, hop, n_fft, frames + 1, _ptr(out)), f"{frames + 1} frames of hop"),
        ("n_fft % 4 != 0", (_ptr(x), 1, L, L, hop, 6, frames, _ptr(out)), "bad arguments"),
        ("misaligned out", (_ptr(x), 1, L, L, hop, n_fft, frames, _ptr(out, 4)), "16-byte aligned"),
        ("null x", (None, 1, L, L, hop, n_fft, frames, _ptr(out)), "null pointer"),
        ("null out", (_ptr(x), 1, L, L, hop, n_fft, frames, None), "null pointer"),
    ]
    for name, args, msg in refusals:
        rc = lib.gdm_stft_frames(*args, _stream())
        assert rc != 0 and msg in _last_error(), (name, rc, _last_error())
        torch.cuda.synchronize()
        assert bool((out == mr.SENTINEL).all()), f"{name}: refused, but the output was written"
    assert lib.gdm_stft_frames(*ok, _stream()) == 0                       # the neighbour of every refusal runs
    c = mr.FrameCase("ok", n_fft, hop, L)
    want = mr.frames_ref(c, x.cpu().numpy().view(np.int32)[None, :])
    assert not mr.check_frames(out[:frames * n_fft], want) and bool((out[frames * n_fft:] == mr.SENTINEL).all())


# -------------------------------------------------------------------------------------------------- power
def _run_power(c, fails):
    x = mr.power_input(c)
    buf = torch.full((c.rows + 2 * mr.GUARD, c.ldp), mr.SENTINEL, device=DEV)
    buf[mr.GUARD:mr.GUARD + c.rows] = float("nan")
    xd = x.to(DEV)
    rc = _lib.load().gdm_power_spectrum(_ptr(xd), c.rows, c.nfreq, c.ldp, _ptr(buf[mr.GUARD]), _stream())
    assert rc == 0, _last_error()
    got = buf.cpu()
    if not bool((got[:mr.GUARD] == mr.SENTINEL).all() and (got[mr.GUARD + c.rows:] == mr.SENTINEL).all()):
        fails.append(f"{c.name}: wrote outside its {c.rows} rows")
    f, worst = mr.check_power(got[mr.GUARD:mr.GUARD + c.rows], c, mr.power_expected(c, x), what=c.name)
    fails += f
    return worst


@pytest.mark.parametrize("nfreq", [1, 5, 33, 1025])
def test_power_spectrum_bound_pads_and_guards(nfreq):
    fails, worst = [], 0.0
    cases = [c for c in mr.POWER_CASES if c.nfreq == nfreq]
    assert len(cases) == 12
    for c in cases:
        worst = max(worst, _run_power(c, fails))
    record("mel_stage_vs_float64", stage="power", case=f"nfreq {nfreq}", worst=worst)
    assert not fails, "\n".join(fails)


def test_power_spectrum_second_grid_trip():
    fails = []
    worst = _run_power(mr.POWER_SECOND_TRIP, fails)
    record("mel_stage_vs_float64", stage="power", case="second trip", worst=worst)
    assert not fails, "\n".join(fails)


def test_power_spectrum_wrapper_is_the_same_kernel_call():
    c = mr.PowerCase(217, 1025, 3)
    x = mr.power_input(c)
    got = ops.power_spectrum(x.to(DEV), c.nfreq, c.ldp)
    fails, _ = mr.check_power(got, c, mr.power_expected(c, x), what="ops.power_spectrum")
    assert not fails, "\n".join(fails)


# ----------------------------------------------------------------------------------------------------- dB
def _run_db(c, fails):
    p = mr.db_input(c)
    got = ops.power_to_db(p.to(DEV), c.B, c.frames, top_db=c.top_db)
    assert got.shape == (c.B, c.n_mels, c.frames)
    exp = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db)
    f, worst = mr.check_values(got, exp["out"], exp["E"], what=c.name)
    fails += f
    return worst


@pytest.mark.parametrize("shape", mr.DB_SHAPES, ids=[f"{f}x{k}" for f, k in mr.DB_SHAPES])
def test_power_to_db_shapes(shape):
    fails, worst = [], 0.0
    cases = [c for c in mr.DB_CASES if (c.frames, c.n_mels) == shape]
    assert len(cases) == 6
    for c in cases:
        worst = max(worst, _run_db(c, fails))
    record("mel_stage_vs_float64", stage="db", case=f"{shape[0]}x{shape[1]}", worst=worst)
    assert not fails, "\n".join(fails)


def test_power_to_db_many_small_windows():
    fails, worst = [], 0.0
    for c in mr.DB_MANY_WINDOWS:
        worst = max(worst, _run_db(c, fails))
    record("mel_stage_vs_float64", stage="db", case="5x3 B=300", worst=worst)
    assert not fails, "\n".join(fails)


def test_power_to_db_at_the_lds_limit():
    fails, worst = [], 0.0
    for c in mr.DB_LDS_FITS:
        worst = max(worst, _run_db(c, fails))
    record("mel_stage_vs_float64", stage="db", case="299x128 (LDS limit)", worst=worst)
    assert not fails, "\n".join(fails)
    frames, n_mels = mr.DB_LDS_REFUSED
    p = torch.ones(frames, n_mels, device=DEV)
    out = torch.full((n_mels * frames,), mr.SENTINEL, device=DEV)
    rc = _lib.load().gdm_power_to_db(_ptr(p), 1, frames, n_mels, 80.0, mr.AMIN, _ptr(out), _stream())
    assert rc != 0 and f"a {n_mels} x {frames} window does not fit the LDS staging (150 KB)" in _last_error()
    torch.cuda.synchronize()
    assert bool((out == mr.SENTINEL).all())
    with pytest.raises(ops.GdmError, match="does not fit the LDS staging"):
        ops.power_to_db(p, 1, frames)


@pytest.mark.parametrize("c", mr.DB_NONFINITE, ids=[c.name for c in mr.DB_NONFINITE])
def test_power_to_db_non_finite_input_follows_torch(c):
    """+inf: the whole window +inf under a floor, only that element without.  NaN: torch.clamp keeps it and amax /
    maximum spread it over the window under a floor.  The clean windows beside it stay within their bounds."""
    fails = []
    p = mr.db_input(c)
    got = ops.power_to_db(p.to(DEV), c.B, c.frames, top_db=c.top_db).cpu()
    want = mr.db_torch(p, c.B, c.frames, c.n_mels, c.top_db)
    bad = {"inf": torch.isinf, "nan": torch.isnan}[c.kind]
    assert int(bad(want[1]).sum()) == (1 if c.top_db is None else c.n) and not bool(bad(want[[0, 2]]).any())
    if not torch.equal(bad(got), bad(want)):
        fails.append(f"{c.name}: {int(bad(got).sum())} {c.kind} element(s) in the result, torch gives "
                     f"{int(bad(want).sum())}; window 1 holds {got[1].min().item()} .. {got[1].max().item()}")
    exp = mr.db_expected(p, c.B, c.frames, c.n_mels, c.top_db)
    f, worst = mr.check_values(got, exp["out"], exp["E"], what=c.name)
    record("mel_stage_vs_float64", stage="db", case=c.name, worst=worst)
    assert not fails + f, "\n".join(fails + f)


# -------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("c", mr.CHAIN_CASES, ids=[c.name for c in mr.CHAIN_CASES])
def test_chain_stage_by_stage(c):
    torch.set_num_threads(16)
    x = mr.chain_input(c).to(DEV)
    frames_m, frames = ops.stft_frames(x, c.hop, c.n_fft)
    assert frames == c.frames
    dft, mel_m = util._dft_matrix(c.n_fft, x.device), util._mel_matrix(*c.mel_args(), x.device)
    assert torch.equal(dft.cpu(), util._dft_matrix(c.n_fft, "cpu"))
    assert torch.equal(mel_m.cpu(), util._mel_matrix(*c.mel_args(), "cpu"))
    spec = ops.gemm(frames_m, dft, compute=F32)
    power = ops.power_spectrum(spec, c.nfreq, c.ldp)
    mel = ops.gemm(power, mel_m, compute=F32)
    db = ops.power_to_db(mel, c.B, frames, top_db=c.top_db)
    splits = [ops.gemm_plan(a, b, compute=F32)["split_k"] for a, b in ((frames_m, dft), (power, mel_m))]
    # what is assembled here is what the package computes
    kw = dict(sr=c.sr, n_fft=c.n_fft, n_mels=c.n_mels, fmin=c.fmin, fmax=c.fmax, top_db=c.top_db)
    assert torch.equal(db, util._db_from_frames(frames_m, c.B, frames, c.sr, c.n_fft, c.n_mels, c.fmin, c.fmax,
                                                c.top_db))
    assert torch.equal(db, util.melspectrogram_db_batch(x, hop=c.hop, **kw))
    fails = mr.check_frames(frames_m, mr.frames_ref(mr.FrameCase(c.name, c.n_fft, c.hop, c.L, c.B),
                                                    mr.chain_input(c).numpy().view(np.int32)), what="frames")
    exp = mr.chain_expected(c, frames_m, dft, mel_m, *splits)
    worst = {}
    for name, got, (ref, E) in (("spectrum", spec, exp["spec"]), ("power", power, exp["power"]),
                                ("mel", mel, exp["mel"]), ("db", db, (exp["db"]["out"], exp["db"]["E"]))):
        f, worst[name] = mr.check_values(got, ref, E, what=f"{c.name} {name}")
        fails += f
    if bool(power[:, c.nfreq:].cpu().view(torch.int32).ne(0).any()):
        fails.append(f"{c.name}: pad columns of the power are not +0")
    record("mel_stage_vs_float64", stage="chain", case=c.name, split_k=splits, **worst)
    assert not fails, "\n".join(fails)
    assert bool((db[3] == db[3, 0, 0]).all()) and abs(float(db[3, 0, 0]) + 100.0) < 1e-4          # the silent window
