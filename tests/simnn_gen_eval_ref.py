"""float64 references for model 1's eval-mode generator forward (csrc/simnn_gen.hip gen_eval_kernel behind
gdm_simnn_gen_eval, functional.simnn_gen_forward_eval, SIMNN.sample_matrices).

A plain module next to simnn_gen_ref.py, which it imports and leaves untouched: tests/test_simnn_gen_eval_gpu.py (GPU)
and tests/test_simnn_gen_eval_ref.py (CPU) import it.

Per layer.  The kernel's taps are the raw pre-BatchNorm accumulators in the training chain's layouts (y1 (B*16, 128),
y2 (B*64, 64), y3 (B*256, 32)) and its three invstd vectors, so every layer is checked on the kernel's own inputs with
the references and bounds simnn_gen_ref already derives from operation counts:
    tap_y1  against first_ref                                        |err| <= RTOL_L1 M
    invstd  against 1 / sqrt(running_var + eps) in float64           |err| <= 4 u invstd  (the add, the square root and
            the division, one rounding each, with one to spare: the rounding term of stats_ref's E_invstd)
    tap_y2, tap_y3 against convt_ref(previous tap, running_mean, tap_invstd, ...)   |err| <= RTOL M + conv(|da|, |w|)
    out     against last_ref(tap_y3, running_mean, tap_invstd, ...)  |err| <= 0.25 E_pre + o (1 - o) u |x| + 8 u o
No new constant: eval mode only replaces the batch statistics by the running ones, the arithmetic after them and its
operation counts are those of the training chain (K = 128, 512, 256 MFMA products per output, 4 fmaf chains of <= 200
taps plus 2 adds in layer 4).

Whole chain (chain_eval_ref): the float64 generator in eval mode with the same rounding points (bf16 noise, bf16
weights of layers 1..3, bf16 staged operands of layers 2 and 3, float64 elsewhere), compared by rel-L2 against
simnn_gen_ref.CHAIN_RELL2 = 1e-4 -- the constant the training chain uses for the same rounding points, where the error
of the batch statistics comes on top.  Measured on MI355X (tests/test_simnn_gen_eval_gpu.py, B = 1 .. 512): see
MEASURED_CHAIN_RELL2 below.

Parameters (calibrated_params).  The committed checkpoint's eval output lies within 2.3e-3 of 0.5 and weights_init
draws BatchNorm weights from N(0, 0.02), so a comparison relative to the output's scale would pass for a kernel that
returns 0.5 everywhere.  The float64 comparisons therefore use conv weights ~ N(0, 0.02) as the constructor draws them,
gamma in 1 +- 0.25, beta in +-0.25, and running statistics CALIBRATED: set, layer by layer, to the float64 train-mode
statistics (mean, biased variance) of a 64-sample calibration batch, so that every layer's normalised activations are
of order one and the output moves (MOVES: ref.min() <= 0.35 and ref.max() >= 0.65, asserted before anything is
compared).  The checkpoint fixture is compared on its deviation from 0.5 (check_deviation).
"""
import torch
import torch.nn.functional as F

import simnn_gen_ref as R
from simnn_gen_ref import CheckError, U, EPS, _d, bf16r  # noqa: F401

BATCHES = [1, 2, 3, 5, 8, 9, 16, 31, 129, 256, 257, 512]
NOISE_DIMS = [1, 37, 100, 128]
CALIBRATION_BATCH = 64
MOVES = (0.35, 0.65)
DEVIATION_RTOL = 2e-2           # the project's bf16 module-output tolerance, on |want - 0.5|
# worst rel-L2 of the kernel's output against chain_eval_ref over the cases of test_whole_chain_against_float64,
# measured on MI355X: 1.55e-5 (B = 512, noise_dim = 1; 1.07e-5 at B = 16 and 257, 5.1e-8 at B = 1); the bound
# CHAIN_RELL2 = 1e-4 is 6.5 times it.
MEASURED_CHAIN_RELL2 = 1.55e-5


# ------------------------------------------------------------------------------------------------ parameters
def calibrated_params(seed, family="base", noise_dim=100, zero_channel=7):
    """(ws, bns): 4 ConvTranspose2d weights and 3 x (gamma, beta, running_mean, running_var, nbt), fp32.
    Families as in tests/test_simnn_gen_batch_gpu.py: "base"; "zero" (conv2's output channel zero_channel zeroed: a
    constant channel, running_var 0, invstd = 1 / sqrt(eps)); "saturate" (conv4 x 40: the sigmoid saturates)."""
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(noise_dim, 128, 4, 4, generator=g) * 0.02, torch.randn(128, 64, 4, 4, generator=g) * 0.02,
          torch.randn(64, 32, 4, 4, generator=g) * 0.02, torch.randn(32, 1, 5, 5, generator=g) * 0.02]
    if family == "zero":
        ws[1][:, zero_channel] = 0.0
    if family == "saturate":
        ws[3] *= 40.0
    gb = [(1 + 0.25 * (2 * torch.rand(c, generator=g) - 1), 0.25 * (2 * torch.rand(c, generator=g) - 1))
          for c in (128, 64, 32)]
    x = torch.randn(CALIBRATION_BATCH, noise_dim, 1, 1, generator=g).double()
    bns = []
    y = F.conv_transpose2d(x, ws[0].double())
    for li in range(3):
        gamma, beta = gb[li]
        mean = y.mean((0, 2, 3))
        var = y.var((0, 2, 3), unbiased=False)
        bns.append((gamma, beta, mean.float(), var.float(), torch.tensor(CALIBRATION_BATCH + li)))
        a = F.batch_norm(y, mean, var, gamma.double(), beta.double(), False, 0.0, EPS).clamp_min(0.0)
        if li < 2:
            y = F.conv_transpose2d(a, ws[li + 1].double(), stride=2, padding=1)
    return ws, bns


def case_noise(B, noise_dim, seed):
    """(B, noise_dim) standard-normal noise; with a single noise component the output is a function of one scalar, so
    those draws are scaled by 3 for one to three samples to span MOVES as well (checked on the float64 reference)."""
    z = torch.randn(B, noise_dim, generator=torch.Generator().manual_seed(seed))
    return 3.0 * z if noise_dim == 1 else z


def assert_moves(ref, what=""):
    lo, hi = float(ref.min()), float(ref.max())
    assert lo <= MOVES[0] and hi >= MOVES[1], f"{what}: the reference output spans only {lo:.3f} .. {hi:.3f}"


# ------------------------------------------------------------------------------------------------- per layer
def invstd_ref(bns, eps=EPS):
    """The three 1 / sqrt(running_var + eps) vectors concatenated (224,) in float64 -> (ref, E = 4 u ref)."""
    inv = torch.cat([1.0 / torch.sqrt(_d(bn[3]) + eps) for bn in bns])
    return inv, 4 * U * inv


def check_layers(noise, ws, bns, out, y1, y2, y3, invstd, *, what=""):
    """Every layer of one gdm_simnn_gen_eval call with taps against float64 on the kernel's own inputs.
    Returns {name: worst |err| / bound}; raises CheckError at the first element out of bounds."""
    B = noise.shape[0]
    worst = {}
    ref, M = R.first_ref(_d(noise).reshape(B, -1), ws[0])
    worst["y1"] = R.check_elementwise(y1, ref, M, rtol=R.RTOL_L1, out_dtype=torch.float32, where=R.where_l1(B),
                                      what=f"{what} layer 1")
    iref, iE = invstd_ref(bns)
    worst["invstd"] = R.check_abs(invstd, iref, iE, what=f"{what} invstd", where=lambda idx: f"invstd element {idx[-1]}")
    inv = torch.split(invstd.detach().cpu(), [128, 64, 32])
    taps = {1: y1, 2: y2, 3: y3}
    for layer in (2, 3):
        g, be, rm = bns[layer - 2][:3]
        ref, _, E = R.convt_ref(taps[layer - 1], rm, inv[layer - 2], g, be, ws[layer - 1], layer, B)
        worst[f"y{layer}"] = R.check_abs(taps[layer], ref, E, what=f"{what} layer {layer}",
                                         where=R.where_convt(layer, B))
    g, be, rm = bns[2][:3]
    ref, E = R.last_ref(y3, rm, inv[2], g, be, ws[3], B)
    worst["out"] = R.check_abs(out, ref, E, what=f"{what} layer 4", where=R.where_last)
    return worst


# ----------------------------------------------------------------------------------------------- whole chain
def chain_eval_ref(noise, ws, bns, *, rounding=True, eps=EPS, faults=()):
    """The float64 generator in eval mode from noise (B, noise_dim[, 1, 1]); bns = 3 x (gamma, beta, running_mean,
    running_var[, nbt]).  rounding: the kernel's rounding points (bf16 noise, bf16 weights of layers 1..3, bf16 staged
    operands of layers 2 and 3); rounding=False is torch.nn's eval-mode generator in float64.  Returns (B, 1, 20, 20).
    faults (tests/test_simnn_gen_eval_ref.py only): "no_eps" (invstd = 1 / sqrt(running_var)), "swap_mean_beta"
    (running mean and beta exchanged), "batch_stats" (the batch's own statistics instead of the running ones),
    "no_relu", "const_half" (output = 0.5 everywhere)."""
    fl = set(faults)
    r = bf16r if rounding else (lambda t: t)
    B = noise.shape[0]
    x = r(_d(noise).reshape(B, -1, 1, 1))
    y = F.conv_transpose2d(x, r(_d(ws[0])))
    for li in range(3):
        g, be, rm, rv = (_d(bns[li][k])[:, None, None] for k in range(4))
        if "swap_mean_beta" in fl:
            rm, be = be, rm
        if "batch_stats" in fl:
            rm = y.mean((0, 2, 3))[:, None, None]
            rv = y.var((0, 2, 3), unbiased=False)[:, None, None]
        inv = 1.0 / torch.sqrt(rv if "no_eps" in fl else rv + eps)
        a = (y - rm) * inv * g + be
        if "no_relu" not in fl:
            a = a.clamp_min(0.0)
        if li < 2:
            y = F.conv_transpose2d(r(a), r(_d(ws[li + 1])), stride=2, padding=1)
        else:
            y = F.conv_transpose2d(a, _d(ws[3]))
    out = torch.sigmoid(y)
    return torch.full_like(out, 0.5) if "const_half" in fl else out


def chain_ratio(out, ref):
    """rel-L2 of out against the chain reference, and that over CHAIN_RELL2"""
    ref = _d(ref)
    rl2 = float((_d(out).reshape(ref.shape) - ref).norm() / ref.norm())
    return rl2, rl2 / R.CHAIN_RELL2


def check_chain(out, ref, *, what=""):
    rl2, ratio = chain_ratio(out, ref)
    if not ratio <= 1.0:
        raise CheckError(f"{what}: whole-chain rel-L2 {rl2:.3g} > {R.CHAIN_RELL2:g}")
    return rl2


def check_deviation(out, want, *, what=""):
    """The checkpoint fixture, whose output lies within 2.3e-3 of 0.5: max |out - want| <= 2e-2 max |want - 0.5|.
    Returns err / bound."""
    want = _d(want)
    err = float((_d(out).reshape(want.shape) - want).abs().max())
    scale = float((want - 0.5).abs().max())
    if not err <= DEVIATION_RTOL * scale:
        raise CheckError(f"{what}: max |out - want| = {err:.3g} > {DEVIATION_RTOL:g} x max |want - 0.5| = "
                         f"{DEVIATION_RTOL * scale:.3g}")
    return err / (DEVIATION_RTOL * scale)


def checkpoint():
    """(state_dict, noise (3, 100, 1, 1), eval output (3, 1, 20, 20)) of tests/golden/simnn_gen_ckpt.npz"""
    from helpers import load_golden
    ck = load_golden("simnn_gen_ckpt.npz")
    sd = {k[3:]: torch.from_numpy(ck[k]) for k in ck.files if k.startswith("sd/")}
    return sd, torch.from_numpy(ck["noise"]), torch.from_numpy(ck["gen_out_eval"])


def checkpoint_params(sd):
    ws = [sd[f"conv{i}.weight"] for i in (1, 2, 3, 4)]
    bns = [tuple(sd[f"batch_norm{i}.{k}"] for k in ("weight", "bias", "running_mean", "running_var",
                                                    "num_batches_tracked")) for i in (1, 2, 3)]
    return ws, bns
