"""float64 reference, bounds, case tables and planted faults for the mel featuriser's kernels (csrc/mel.hip:
gdm_stft_frames, gdm_power_spectrum, gdm_power_to_db) and for the chain util._db_from_frames drives through them.
A plain module next to gemm_ref.py: tests/test_mel_ref.py (CPU) proves that the checkers reject every planted fault on
the tables below and holds the host-built constants; tests/test_mel_stages_gpu.py (GPU) holds the kernels to it.

Every bound is derived per element (u = 2^-24) and none is tuned to what a kernel returns.

  frames: a gather -- bit equality, compared as int32 so that NaN payloads, -0 and denormals count.  The reference is
    np.pad(., n_fft // 2, "reflect") of the first L samples of each row, frame f starting at f hop.
  power: re^2 + im^2 in float64 on the fp32 inputs; |got - ref| <= 3 u ref: two products and a sum of non-negative
    terms, two or three roundings with or without FMA contraction.  Below the normal range a rounding's error is
    absolute, at most 2^-150 each (gradual underflow): + 3 2^-150.  A result that float64 rounded to fp32 makes +inf
    or NaN must be +inf or NaN.  Pad columns nfreq .. ldp-1 are bit-equal to +0.
  dB: d = 10 log10(max(p, amin)) in float64 on the fp32 inputs, amin rounded to fp32 as the kernel receives it;
    E_d = LOG10_ULPS 2^-23 |d| + 2^-126 with LOG10_ULPS = 4: the HIP math API documents log10f at 2 ulp, the multiply
    by 10 adds half an ulp, the rest is slack for a faithful rather than nearest result.  With a floor,
    out = max(d, mx - top_db), mx the window maximum; the element that is the maximum is known only within the bounds,
    so E_top is the largest E_d among the elements whose d + E_d reaches the largest d - E_d of the window, and an
    element gets max(E_d, E_top) unless it lies above the floor by more than both (then E_d alone).  The subtraction
    mx - top_db is one more rounding, u |mx - top_db|, which the 1.5 ulp of slack in E_top (1.5 2^-23 |mx|) covers when
    |mx - top_db| <= 3 |mx|: db_expected asserts that of every window it is given, so the tables' inputs are loud (or
    silent) enough for the stated bound to be sound.  NaN and +inf follow torch: torch.clamp, amax and torch.maximum
    propagate NaN, so one NaN makes its whole window NaN under a floor and only itself NaN without.
  chain (frames -> fp32 DFT GEMM -> power -> fp32 mel GEMM -> dB), on the fp32 constants exactly as the device holds
    them: the spectrum gets gemm_ref's continuous fp32 bound (K + split_k + 2) 2^-23 sum|x||D| with split_k from the
    library's own plan of that call; the power gets 2|re|E_re + E_re^2 + 2|im|E_im + E_im^2 plus the power stage's
    3 u of (ref + that); the mel power the same GEMM bound on (p + E_p)|M| plus E_p|M|; the dB what the interval
    [mel - E_mel, mel + E_mel] clamped at amin maps to -- never more than 10 / ln 10 E_mel / max(mel - E_mel, amin),
    and the wider of clamp and log where the interval straddles amin -- plus the log bound.

Planted faults (FRAME_FAULTS, POWER_FAULTS, DB_FAULTS) are applied to the mirrors and evaluated on the CPU.
"""
import dataclasses
import functools
import math

import numpy as np
import torch

from lowering_ref import F32_TINY, U, check_bound

LOG10_ULPS = 4
AMIN = float(np.float32(1e-10))             # the amin the kernel receives
GRID_LANES = 16384 * 256                    # mel.hip blocks_for: grid-stride loops of at most 16384 blocks x 256
DB_BLOCK = 1024                             # power_to_db_kernel: one workgroup of 1024 per window
LDS_FLOATS = 150 * 1024 // 4                # its LDS staging: n_mels (frames + 1) floats
GUARD = 4                                   # sentinel rows above and below a caller-owned output
SENTINEL = -12352.0

FRAME_FAULTS = ("symmetric_right", "reflect_about_L", "start_off_by_one", "stride_ignored", "last_row_dropped",
                "second_trip_dropped")
POWER_FAULTS = ("im_off_by_one", "pads_unwritten", "last_row_dropped", "second_trip_dropped")
DB_FAULTS = ("floor_window0", "floor_batch_max", "not_transposed", "no_amin_clamp", "none_as_zero",
             "ragged_tail_dropped", "nan_swallowed")


def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def trips(total):
    """trips of a grid-stride loop over `total` lanes, blocks of 256 capped at 16384"""
    blocks = min(16384, max(1, (total + 255) // 256))
    return (total + blocks * 256 - 1) // (blocks * 256)


def check_values(got, ref, E, *, what=""):
    """|got - ref| <= E per element where the float64 reference rounded to fp32 is finite; where it is +-inf or NaN,
    got must be the same.  -> (failures, worst err / bound over the finite elements)"""
    got, ref, E = _d(got).reshape(ref.shape), ref.double(), E.double()
    want = ref.float().double()                               # overflow of the one rounding to fp32 -> inf
    special = ~torch.isfinite(want)
    fails = []
    same = torch.where(torch.isnan(want), torch.isnan(got), got == want)
    bad = special & ~same
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        fails.append(f"{what}: {int(bad.sum())} non-finite element(s) differ; first at {list(idx)}: got "
                     f"{float(got[idx])!r} want {float(want[idx])!r}")
    zero = torch.zeros_like(ref)
    f, worst = check_bound(torch.where(special, zero, got), torch.where(special, zero, ref),
                           torch.where(special, zero, E), what=what)
    return fails + f, worst


# ============================================================================================== stft frames
@dataclasses.dataclass(frozen=True)
class FrameCase:
    name: str
    n_fft: int
    hop: int
    L: int
    B: int = 1
    extra: int = 0               # x is the first L columns of a (B, L + extra) buffer: x_stride = L + extra

    @property
    def frames(self):
        return 1 + self.L // self.hop

    @property
    def total4(self):
        return self.B * self.frames * (self.n_fft // 4)


FRAME_CASES = [
    FrameCase("one chunk per row, minimum L", 4, 1, 3),
    FrameCase("one chunk per row", 4, 1, 9),
    FrameCase("gaps: hop > n_fft", 8, 13, 40),
    FrameCase("minimum L, both sides reflected in one frame", 64, 7, 33),
    FrameCase("last frame centred on L", 64, 16, 64),
    FrameCase("last frame short of L", 64, 16, 70),
    FrameCase("hop of 1", 2048, 1, 1025),
    FrameCase("reference geometry", 2048, 1025, 220500, B=2),
    FrameCase("strided batch", 64, 16, 70, B=3, extra=37),
    FrameCase("strided batch, last frame centred on L", 64, 16, 64, B=3, extra=37),
    FrameCase("second grid trip", 4096, 1, 4096),
]

# NaNs with payloads (quiet, negative quiet, signalling), both zeros, denormals of both signs
_FRAME_SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x00000000, 0x80000000, 0x00000001, 0x807fffff],
                           dtype=np.uint32).view(np.int32)
TRAILING_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.int32)[0]      # the default NaN: not a planted one


@functools.lru_cache(maxsize=4)
def frame_input(c):
    """int32 bit patterns of the (B, L + extra) fp32 buffer: seeded normals, the specials planted inside the valid
    samples of every row (the first and the last sample among them), the trailing columns all the default NaN"""
    g = np.random.default_rng(c.n_fft * 1000003 + c.hop * 10007 + c.L)
    bits = g.standard_normal((c.B, c.L + c.extra)).astype(np.float32).view(np.int32).copy()
    for b in range(c.B):
        inner = np.unique(g.integers(1, c.L - 1, size=12))[:max(0, c.L // 2 - 2)]     # (at most half of a short row)
        pos = np.concatenate([[0, c.L - 1], inner]).astype(np.int64)
        bits[b, pos] = _FRAME_SPECIALS[(np.arange(len(pos)) + b + c.L) % len(_FRAME_SPECIALS)]
    bits[:, c.L:] = TRAILING_NAN
    bits.setflags(write=False)
    return bits


def frames_ref(c, bits, *, faults=()):
    """(B frames, n_fft) int32: row (b, f) = reflect-padded x_b[f hop - n_fft / 2 + n], n < n_fft"""
    pad, L = c.n_fft // 2, c.L
    idx = np.pad(np.arange(L), pad, mode="reflect")          # sample index of every padded position
    j = np.arange(pad)
    if "symmetric_right" in faults:
        idx[pad + L:] = L - 1 - j
    if "reflect_about_L" in faults:                           # s >= L reads 2 L - s (s = L itself: the last sample)
        idx[pad + L:] = np.minimum(L - j, L - 1)
    if "stride_ignored" in faults:
        flat = bits.reshape(-1)
        x = np.stack([flat[b * L:(b + 1) * L] for b in range(c.B)])
    else:
        x = bits[:, :L]
    xp = x[:, idx]
    first = 0
    if "start_off_by_one" in faults:
        xp, first = np.concatenate([xp, xp[:, -1:]], axis=1), 1
    win = np.lib.stride_tricks.sliding_window_view(xp, c.n_fft, axis=1)[:, first::c.hop][:, :c.frames]
    assert win.shape == (c.B, c.frames, c.n_fft), (win.shape, c)
    out = np.ascontiguousarray(win).reshape(c.B * c.frames, c.n_fft)
    if "last_row_dropped" in faults:
        out[-1] = 0
    if "second_trip_dropped" in faults:
        out.reshape(-1)[4 * min(GRID_LANES, (c.total4 + 255) // 256 * 256):] = 0
    return out


def check_frames(got, want, *, what=""):
    """bit equality of int32 views, the first difference named"""
    got = np.ascontiguousarray(torch.as_tensor(got).detach().cpu().numpy()).view(np.int32).reshape(-1)
    want = np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return [f"{what}: {got.shape} elements, want {want.shape}"]
    ne = np.flatnonzero(got != want)
    if ne.size == 0:
        return []
    return [f"{what}: {ne.size} element(s) differ; first at flat index {int(ne[0])}: got bits "
            f"{int(got[ne[0]]) & 0xffffffff:#010x} want {int(want[ne[0]]) & 0xffffffff:#010x}"]


# ============================================================================================ power spectrum
@dataclasses.dataclass(frozen=True)
class PowerCase:
    rows: int
    nfreq: int
    pad: int

    @property
    def ldp(self):
        return self.nfreq + self.pad

    @property
    def name(self):
        return f"{self.rows}x{self.nfreq}+{self.pad}"


POWER_CASES = [PowerCase(r, n, p) for n in (1, 5, 33, 1025) for p in (0, 1, 3, 7) for r in (1, 3, 217)]
POWER_SECOND_TRIP = PowerCase(4097, 1021, 3)
# 0, -0, denormals, 1e19 (its square 1e38 is still finite in fp32), 2e19 (its square is not: +inf, as float64 rounded
# to fp32 gives), NaN
_POWER_SPECIALS = [0.0, -0.0, 1e-40, -1e-42, 1e19, -1e19, 2e19, math.nan]


@functools.lru_cache(maxsize=4)
def power_input(c):
    """(rows, 2 nfreq) fp32 [re | im]: seeded normals with the specials planted (at most a third of the elements;
    which ones rotates with the case, so the small cases see all of them between them)"""
    g = torch.Generator().manual_seed(c.rows * 10007 + c.nfreq * 101 + c.pad)
    x = torch.randn(c.rows, 2 * c.nfreq, generator=g)
    n = x.numel()
    k = min(2 * len(_POWER_SPECIALS), max(1, n // 3))
    pos = torch.randperm(n, generator=g)[:k]
    rot = c.rows + c.nfreq + c.pad
    x.view(-1)[pos] = torch.tensor([_POWER_SPECIALS[(i + rot) % len(_POWER_SPECIALS)] for i in range(k)])
    return x


def power_expected(c, x, *, faults=()):
    """-> dict(out (rows, ldp) float64 with NaN where a faulty kernel leaves the NaN-prefilled buffer unwritten, E)"""
    x = _d(x)
    re, im = x[:, :c.nfreq], x[:, c.nfreq:]
    if "im_off_by_one" in faults:
        flat = torch.cat([x.reshape(-1), torch.zeros(1, dtype=torch.float64)])
        at = torch.arange(c.rows)[:, None] * 2 * c.nfreq + c.nfreq + torch.arange(c.nfreq)[None, :] + 1
        im = flat[at]
    out = torch.zeros(c.rows, c.ldp, dtype=torch.float64)
    out[:, :c.nfreq] = re * re + im * im
    if "pads_unwritten" in faults:
        out[:, c.nfreq:] = math.nan
    if "last_row_dropped" in faults:
        out[-1] = math.nan
    if "second_trip_dropped" in faults:
        out.view(-1)[min(GRID_LANES, (c.rows * c.ldp + 255) // 256 * 256):] = math.nan
    E = 3 * U * out.abs() + 3 * 2.0 ** -150
    E[:, c.nfreq:] = 0
    return dict(out=out, E=torch.nan_to_num(E, nan=0.0, posinf=0.0))


def check_power(got, c, exp, *, what=""):
    """the bound on columns < nfreq, +0 bit for bit in the pad columns -> (failures, worst err / bound)"""
    got = torch.as_tensor(got).detach().cpu().reshape(c.rows, c.ldp)
    fails, worst = check_values(got[:, :c.nfreq], exp["out"][:, :c.nfreq], exp["E"][:, :c.nfreq], what=what)
    bad = got[:, c.nfreq:].float().contiguous().view(torch.int32) != 0
    if bool(bad.any()):
        r, k = (int(i) for i in bad.nonzero()[0])
        fails.append(f"{what}: {int(bad.sum())} pad element(s) are not +0; first at row {r} column {c.nfreq + k}")
    return fails, worst


# ===================================================================================================== dB
@dataclasses.dataclass(frozen=True)
class DbCase:
    frames: int
    n_mels: int
    B: int
    top_db: object               # 80, 0 or None
    kind: str = "finite"         # "inf" / "nan": window 1 of 3 holds one +inf / NaN

    @property
    def n(self):
        return self.frames * self.n_mels

    @property
    def name(self):
        return f"{self.frames}x{self.n_mels} B={self.B} top_db={self.top_db}" + \
            ("" if self.kind == "finite" else f" {self.kind}")


DB_SHAPES = [(1, 1), (1, 7), (5, 3), (31, 33), (33, 31), (216, 128), (217, 128), (37, 1000)]
TOP_DBS = (80, 0, None)
DB_CASES = [DbCase(f, k, b, t) for (f, k) in DB_SHAPES for b in (1, 3) for t in TOP_DBS]
DB_MANY_WINDOWS = [DbCase(5, 3, 300, t) for t in TOP_DBS]
DB_LDS_FITS = [DbCase(299, 128, 2, t) for t in TOP_DBS]               # n_mels (frames + 1) = 38400 = LDS_FLOATS
DB_LDS_REFUSED = (300, 128)
DB_NONFINITE = [DbCase(f, k, 3, t, kind) for (f, k) in ((31, 33), (216, 128)) for t in TOP_DBS
                for kind in ("inf", "nan")]
assert DB_LDS_FITS[0].n_mels * (DB_LDS_FITS[0].frames + 1) == LDS_FLOATS


def _amin_neighbours():
    a = np.float32(AMIN)
    return [0.0, float(a), float(np.nextafter(a, np.float32(0))), float(np.nextafter(a, np.float32(1))), 1.0]


@functools.lru_cache(maxsize=8)
def db_input(c):
    """(B frames, n_mels) fp32 powers: log-uniform over 1e-14 .. 1e6 times a loudness of its own per window (-17 ..
    +13 dB), each window's maximum 1e6 times that loudness planted at a seeded position -- in window 0 at the last
    element, which is in the ragged tail of the kernel's loop when n % 1024 != 0 -- and 0, amin, amin's two fp32
    neighbours and 1.0 planted where the window has room (rotated over the windows).  The last window of a batch, and
    every window when there is no floor, also holds 3.0e38 (with a floor it raises everything else to the floor).
    kind "inf" / "nan": one element of window 1 is +inf / NaN."""
    g = torch.Generator().manual_seed(c.frames * 10007 + c.n_mels * 101 + c.B)
    n = c.n
    p = 10.0 ** (torch.rand(c.B, n, generator=g, dtype=torch.float64) * 20.0 - 14.0)
    plants = _amin_neighbours()
    for w in range(c.B):
        loud = 10.0 ** ((((w * 7) % 31) - 17) / 10.0)
        p[w] *= loud
        perm = torch.randperm(n, generator=g).tolist()
        if w == 0:
            perm.remove(n - 1)
            perm.insert(0, n - 1)
        p[w, perm[0]] = 1e6 * loud
        for j in range(min(len(plants), n - 1)):
            p[w, perm[1 + j]] = plants[(j + w) % len(plants)]
        if n > 1 + len(plants) and (c.top_db is None or (c.B > 1 and w == c.B - 1)):
            p[w, perm[1 + len(plants)]] = 3.0e38
        if c.kind != "finite" and w == 1:
            p[w, perm[-1]] = math.inf if c.kind == "inf" else math.nan
    return p.float().reshape(c.B * c.frames, c.n_mels)


def db_expected(p, B, frames, n_mels, top_db, *, E_in=None, amin=AMIN, faults=()):
    """p (B frames, n_mels): the float64 reference of the kernel's input, known within E_in (None: exactly).
    -> dict(out (B, n_mels, frames) float64, E).  See the module docstring for the bound."""
    n = frames * n_mels
    p = _d(p).reshape(B, n)
    E_in = torch.zeros_like(p) if E_in is None else _d(E_in).reshape(B, n)
    tiny = torch.full_like(p, amin)

    def db(v):
        return 10.0 * torch.log10(v)

    d = db(p) if "no_amin_clamp" in faults else db(torch.clamp(p, min=amin))
    if "nan_swallowed" in faults:
        d = torch.where(torch.isnan(p), db(tiny), d)
    fin = torch.isfinite(d)
    d0 = torch.where(fin, d, torch.zeros_like(d))
    prop = torch.maximum(db(torch.maximum(p + E_in, tiny)) - d0, d0 - db(torch.maximum(p - E_in, tiny)))
    prop = torch.where(fin & (E_in > 0), prop, torch.zeros_like(d))
    # (never wider than the first-order expression 10 / ln 10 E / max(p - E, amin): log is concave)
    first_order = 10.0 / math.log(10.0) * E_in / torch.maximum(p - E_in, tiny)
    assert faults or bool((prop <= first_order * (1 + 1e-9) + 1e-300)[fin].all())
    E_d = LOG10_ULPS * 2.0 ** -23 * (d0.abs() + prop) + F32_TINY + prop
    E_d = torch.where(fin, E_d, torch.zeros_like(E_d))
    td = 0.0 if (top_db is None and "none_as_zero" in faults) else top_db
    if td is None:
        out, E = d, E_d
    else:
        dm = d
        tail = n % DB_BLOCK if "ragged_tail_dropped" in faults else 0
        if tail:
            dm = d[:, :n - tail]
        mx = dm.amax(1, keepdim=True) if dm.shape[1] else torch.full((B, 1), -math.inf, dtype=torch.float64)
        if "floor_window0" in faults:
            mx = mx[:1].expand(B, 1)
        if "floor_batch_max" in faults:
            mx = mx.amax().expand(B, 1)
        floor = mx - td
        out = torch.maximum(d, floor)
        if tail:
            out[:, n - tail:] = 0.0
        neg = torch.full_like(d, -math.inf)
        low = torch.where(fin, d - E_d, neg).amax(1, keepdim=True)          # the maximum is at least this
        cand = fin & (d + E_d >= low)
        E_top = torch.where(cand, E_d, torch.zeros_like(E_d)).amax(1, keepdim=True)
        clear = d - E_d > floor + E_top                                      # above the floor whatever the errors
        E = torch.where(clear, E_d, torch.maximum(E_d, E_top))
        if not faults:
            ok = ~torch.isfinite(mx) | ((mx - td).abs() <= 3.0 * mx.abs())
            assert bool(ok.all()), "a window's maximum is too close to 0 dB for the floor's own rounding to fit E_top"
    E = torch.where(torch.isfinite(out), E, torch.zeros_like(E))
    if "not_transposed" in faults:
        return dict(out=out.reshape(B, n_mels, frames), E=E.reshape(B, n_mels, frames))

    def t(v):
        return v.reshape(B, frames, n_mels).transpose(1, 2).contiguous()
    return dict(out=t(out), E=t(E))


def db_torch(p, B, frames, n_mels, top_db, amin=AMIN):
    """torch's own semantics (clamp / amax / maximum propagate NaN), float64: (B, n_mels, frames)"""
    d = 10.0 * torch.log10(torch.clamp(_d(p).reshape(B, frames, n_mels), min=amin))
    if top_db is not None:
        d = torch.maximum(d, d.amax((1, 2), keepdim=True) - top_db)
    return d.transpose(1, 2).contiguous()


# ========================================================================================== host constants
def dft_matrix_ref(n_fft, *, symmetric=False):
    """float64 [w cos | w sin] written independently of util._dft_matrix: torch.hann_window (periodic; symmetric is
    the planted fault) times numpy's cos / sin of 2 pi (k n mod N) / N; the sine exactly 0 where 2 k n is a multiple of
    N (k = 0, k = N / 2), as it is mathematically"""
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    kn = (n * k) % n_fft
    ang = 2.0 * np.pi * kn.astype(np.float64) / n_fft
    sin = np.where((2 * kn) % n_fft == 0, 0.0, np.sin(ang))
    win = torch.hann_window(n_fft, periodic=not symmetric, dtype=torch.float64).numpy()[:, None]
    return np.concatenate([np.cos(ang) * win, sin * win], axis=1)


def check_dft_matrix(m, n_fft, *, what=""):
    """m (n_fft, 2 nfreq) fp32 against dft_matrix_ref rounded once: within 1 fp32 ulp (the two float64 cosines may
    differ in the last bit), and exactly zero in row 0 and in the sine columns k = 0 and k = n_fft / 2"""
    nfreq = n_fft // 2 + 1
    m = torch.as_tensor(m).detach().cpu()
    want = torch.from_numpy(dft_matrix_ref(n_fft)).float()
    fails = []
    if m.shape != want.shape or m.dtype != torch.float32:
        return [f"{what}: {tuple(m.shape)} {m.dtype}"]
    ulp = torch.maximum(torch.ldexp(torch.ones_like(want), (torch.frexp(want)[1] - 24).to(torch.int32)),
                        torch.full_like(want, 2.0 ** -149))
    bad = ~((m.double() - want.double()).abs() <= ulp.double())
    if bool(bad.any()):
        r, k = (int(i) for i in bad.nonzero()[0])
        fails.append(f"{what}: {int(bad.sum())} element(s) more than 1 ulp off; first at [{r}, {k}]: "
                     f"{float(m[r, k])!r} want {float(want[r, k])!r}")
    for name, part in (("row 0", m[0]), ("sine column k = 0", m[:, nfreq]), ("sine column k = N/2", m[:, 2 * nfreq - 1])):
        if bool((part != 0).any()):
            fails.append(f"{what}: {name} is not exactly zero (max |v| = {float(part.abs().max()):.3g})")
    return fails


# =================================================================================================== chain
@dataclasses.dataclass(frozen=True)
class ChainCase:
    name: str
    n_fft: int
    n_mels: int
    hop: int
    L: int
    sr: int
    fmin: float
    fmax: float
    B: int = 4
    top_db: float = 80

    @property
    def frames(self):
        return 1 + self.L // self.hop

    @property
    def nfreq(self):
        return self.n_fft // 2 + 1

    @property
    def ldp(self):
        return (self.nfreq + 3) // 4 * 4

    def mel_args(self):
        return (self.n_fft, self.sr, self.n_mels, self.fmin, self.fmax, self.ldp)


# sr / fmin / fmax of the small geometries are chosen so that no filter is empty (tests/test_mel_ref.py checks it)
CHAIN_CASES = [
    ChainCase("n_fft 8, 4 mels", 8, 4, 3, 50, 1000, 0.0, 500.0),
    ChainCase("n_fft 64, 8 mels", 64, 8, 16, 400, 8000, 0.0, 4000.0),
    ChainCase("n_fft 256, 20 mels, hop 50", 256, 20, 50, 1230, 16000, 20.0, 8000.0),
    ChainCase("reference geometry", 2048, 128, 1025, 220500, 44100, 20.0, 8300.0, B=5),
]


@functools.lru_cache(maxsize=2)
def chain_input(c):
    """(B, L) fp32 windows of differing level: a seeded tone plus noise, an integer-valued ramp, an impulse at sample 0
    and another at the last sample (the reflected edges), a silent window, and (B = 5) a second, quieter tone"""
    g = np.random.default_rng(c.n_fft + c.n_mels)
    t = np.arange(c.L) / c.sr
    f0 = c.fmin + 0.37 * (c.fmax - c.fmin)
    x = np.zeros((c.B, c.L))
    x[0] = 300.0 * np.sin(2 * np.pi * f0 * t + 0.3) + 20.0 * g.standard_normal(c.L)
    x[1] = (np.arange(c.L) * 7) % 61 - 30.0
    x[2, 0], x[2, -1] = 1000.0, -700.0
    if c.B > 4:
        x[4] = 40.0 * np.sin(2 * np.pi * 0.61 * f0 * t) + 3.0 * g.standard_normal(c.L)
    return torch.from_numpy(x.astype(np.float32))


def gemm_f32_bound(a, b, split_k):
    """gemm_ref's continuous fp32 bound of a @ b: (K + split_k + 2) 2^-23 sum|a||b|"""
    return (a.shape[1] + split_k + 2) * 2.0 ** -23 * (a.abs() @ b.abs())


def chain_expected(c, frames_m, dft, mel_m, split_dft, split_mel):
    """frames_m (B frames, n_fft), dft (n_fft, 2 nfreq), mel_m (ldp, n_mels): the fp32 tensors the device holds;
    split_*: split_k of the library's plan for the two GEMMs.
    -> dict(spec=(ref, E), power=(ref, E), mel=(ref, E), db=dict(out, E)), float64"""
    F, D, M = _d(frames_m), _d(dft), _d(mel_m)
    nfreq = c.nfreq
    spec = F @ D
    E_spec = gemm_f32_bound(F, D, split_dft)
    re, im, E_re, E_im = spec[:, :nfreq], spec[:, nfreq:], E_spec[:, :nfreq], E_spec[:, nfreq:]
    p = torch.zeros(F.shape[0], c.ldp, dtype=torch.float64)
    E_p = torch.zeros_like(p)
    p[:, :nfreq] = re * re + im * im
    prop = 2 * re.abs() * E_re + E_re ** 2 + 2 * im.abs() * E_im + E_im ** 2
    E_p[:, :nfreq] = prop + 3 * U * (p[:, :nfreq] + prop) + 3 * 2.0 ** -150
    mel = p @ M
    E_mel = gemm_f32_bound(p + E_p, M, split_mel) + E_p @ M.abs()
    db = db_expected(mel, c.B, c.frames, c.n_mels, c.top_db, E_in=E_mel)
    return dict(spec=(spec, E_spec), power=(p, E_p), mel=(mel, E_mel), db=db)
