"""float64 references for model 1's fused generator forward (csrc/simnn_gen.hip, functional.simnn_gen_forward_fused):
one op at a time on the kernel's own inputs, with element bounds, locators and mirrors of the launch plan.

A plain module next to trunk_ref.py and mmgan_ref.py: tests/test_simnn_gen_batch_gpu.py (GPU) and
tests/test_simnn_gen_ref.py (CPU) import it.  The checkers are trunk_ref.check_elementwise and mmgan_ref.check_abs.

Layouts (channels-last fp32 between the kernels): y1 (B*16, 128), row b*16 + kh*4 + kw (the 1x1 input's output pixel
IS the tap); y2 (B*64, 64), row b*64 + oy*8 + ox; y3 (B*256, 32); out (B, 1, 20, 20).  Partials of layers 2 and 3:
(chunks, Cout, 3) = (n, mean, M2) of workgroup 4*group + class, class = 2*(oy & 1) + (ox & 1), group = b // S
(S = 8 samples for layer 2, 4 for layer 3): the valid pixels of min(S, B - S*group) samples of one parity class.

Rounding model.  u = 2^-24.  bf16 x bf16 products are exact in fp32; a sum with n fp32 roundings on the longest path
to the result is off by at most n u sum |terms| = n u M, M the same op on absolute values.

Layer 1 (gdm_simnn_gen_first; for B > 256 the tap-major bf16 GEMM of functional.convT_forward).  Operands are
bf16(noise) and bf16(w1), K = noise_dim zero padded to 128: |y1 - ref| <= (128 + 1) u M.  The output is the fp32
accumulator itself (no second rounding: trunk_ref.ulp is 0 for fp32).

Batch statistics of a kernel-produced y (stats_ref).  mean, invstd = 1 / sqrt(M2 / n + eps), running_mean and
running_var blended with momentum 0.1 from the caller's values, running_var from the unbiased M2 / (n - 1),
num_batches_tracked + 1.  The kernels differ in how they sum, not in what: gen_l1_kernel sums two-pass within one
workgroup (16 tiles per lane, 6 butterfly levels, 4 waves: G = 32 roundings on the longest path); convt_s2_bn_kernel
leaves exact two-pass partials (PTW = 2 or 4 values per lane, 4 butterfly levels, 4 waves: <= 16) that bn_finalize
merges with Chan's formula, wave w taking chunks w, w + 16, ... and then the 16 wave results (ceil(chunks / 16) + 16
merges on a path, each <= 8 roundings of values <= max |y - mean| + |mean|); gdm_bn_stats (B > 256) sums shifted
values (shift = a chunk's first value) over chunk_rows / 4 rows per lane.  So with G = P + 8 (ceil(chunks / 16) + 16)
+ 8 and D = max |y - mean| per channel:
    E_mean = G u max |y|,
    E_M2   = G u (M2 + [shifted] n D^2) + 4 n D E_mean   (the shifted sums carry (y - shift)^2 <= (y - mean)^2 + D^2;
             a mean error e moves a two-pass M2 by n e^2 and a Chan merge term by 2 |d| e per unit weight),
    E_invstd = 1/2 (var_lo + eps)^-3/2 E_M2 / n + 4 u invstd,
    running statistics: momentum times the error of what is blended in, plus 4 u of each value.
A constant channel (all of y equal) has D = 0 and M2 = 0: the bound is then exact, M2 must come out 0.

Partials (partials_ref): the same triple per workgroup in float64 from its own valid pixels; n exact,
E_mean = 18 u max |y|, E_M2 = 24 u M2 + n E_mean^2.

Layers 2 and 3 (convt_ref, convt_s2_bn_kernel).  The staged operand is mirrored as the gfx950 code computes it:
sc = fp32(invstd * gamma), v = fma(fp32(x - mean), sc, beta) single-rounded to fp32, a = bf16_rne(max(v, 0)).
v is evaluated in float64 and rounded to fp32; an operand whose value lies within one fp32 ulp of a bf16 rounding
midpoint may round either way on the device (and the float64 -> fp32 step is a double rounding), so
|da| = bf16(v + ulp32) - bf16(v - ulp32) is carried into the bound as conv(|da|, |w|).  The convolution itself is
F.conv_transpose2d(k4, s2, p1) in float64 on bf16(w) -- deliberately not the kernel's parity-class decomposition.
Accumulation: K = 4 Cin products per output in fp32 (MFMA), so RTOL = (K + 1) u: 3.06e-5 for layer 2 (K = 512) and
1.53e-5 for layer 3 (K = 256).
    |y - ref| <= RTOL M + conv(|da|, |w|).

Layer 4 (last_ref, convt_k5_bn_sigmoid_kernel).  Operands stay fp32: the staged value is the same FMA expression
(within one fp32 ulp, <= 2 u |a|), the sum runs as four fmaf chains of <= 200 taps plus 2 adds, so the
pre-activation is bounded by E_pre = (202 + 2) u M_pre.  The output is 1 / (1 + __expf(-x)): the argument scaled
by log2 e for v_exp_f32 (an absolute error of u |x| in the exponent, o (1 - o) u |x| in o), v_exp_f32 and v_rcp_f32
(1 ulp each, <= 2 u relative, each moving o by <= 2 u o) and the add (u): 5 u o; c = 8 leaves room for one more
rounding.
    |o - ref| <= 0.25 E_pre + o (1 - o) u |x| + 8 u o.

Whole chain (chain_ref): the float64 generator from the noise with the same rounding points (bf16 noise, weights of
layers 1..3 and staged operands of layers 2 and 3; float64 everywhere else).  rounding=False is the plain float64
generator.  Between kernel and chain reference, bf16 rounding-boundary decisions compound through three batch norms,
so the chain is compared by rel-L2: the output by ||out - ref|| <= CHAIN_RELL2 ||ref||, a running statistic by
||got - ref|| <= CHAIN_STATS_RELL2 ||ref - (1 - momentum) init|| + 4 u (||ref|| + ||ref - (1 - momentum) init||), i.e.
relative to what the batch blended in, plus the fp32 roundings of the blend (with the reference init's BatchNorm
weights ~ N(0, 0.02) the variances are ~1e-5 against a stored value ~0.9, so one ulp of the stored value is a percent
of the blended part).  Measured on MI355X (tests/test_simnn_gen_batch_gpu.py, B = 2 .. 512 and two trainer steps):
output rel-L2 at most 2.6e-5 (B = 257), so CHAIN_RELL2 = 1e-4 is 3.8 times it; the blended running statistics of
the direct chain by rel-L2 alone at most 1.4e-5 (running_mean of layer 1, B = 512), so CHAIN_STATS_RELL2 = 5e-5 is
3.6 times it; with the rounding term every running statistic stays within 0.16 of its allowance (running_var of
layer 3, trainer step at B = 16).
"""

import math

import torch
import torch.nn.functional as F

from mmgan_ref import check_abs
from trunk_ref import CheckError, check_elementwise  # noqa: F401  (re-exported)

U = 2.0 ** -24
MOMENTUM, EPS = 0.1, 1e-5
L1_K = 128                                      # simnn_gen.hip:32   layer 1's K, zero padded
L1_CH = 4                                       # simnn_gen.hip:52   channels per gen_l1_kernel workgroup
S = {2: 8, 3: 4}                                # simnn_gen.hip:398  samples per convt_s2_bn_kernel workgroup
GEOM = {1: (1, 4, 128), 2: (4, 8, 64), 3: (8, 16, 32)}      # layer -> (input side, output side, output channels)
CIN = {2: 128, 3: 64}
FINALIZE_ROUND = 16 * 8                         # pointwise.hip:196  chunks bn_finalize merges per round
RTOL = {2: (4 * 128 + 1) * U, 3: (4 * 64 + 1) * U}
RTOL_L1 = (L1_K + 1) * U
N_PRE = 202 + 2
C_SIG = 8
# the fused chain against chain_ref (set from measurement: see the module docstring)
CHAIN_RELL2 = 1e-4
CHAIN_STATS_RELL2 = 5e-5

BATCHES = [2, 3, 4, 5, 6, 8, 9, 16, 31, 128, 129, 255, 256, 257, 260, 512]
NOISE_DIMS = [1, 37, 100, 128]


# ---------------------------------------------------------------------------------------------- plan mirrors
def convt_chunks(layer, B):
    """gdm_simnn_gen_convt_chunks: 4 parity classes x ceil(B / S) sample groups"""
    return 4 * ((B + S[layer] - 1) // S[layer])


def bn_row_chunks(rows):
    """pointwise.hip row_chunks: >= 256 rows per chunk, at most 64 chunks"""
    return min(64, max(1, (rows + 255) // 256))


def finalize_rounds(chunks):
    return (chunks + FINALIZE_ROUND - 1) // FINALIZE_ROUND


def regimes(B, noise_dim=100, aligned=True):
    """What the fused chain exercises at batch B: the tail sizes of the layer-2 / layer-3 workgroups (0 = full), the
    bn_finalize rounds of layers 2 and 3, layer 1's route and its noise staging."""
    return dict(tail2=B % S[2], tail3=B % S[3], rounds2=finalize_rounds(convt_chunks(2, B)),
                rounds3=finalize_rounds(convt_chunks(3, B)), first="gen_first" if B <= 256 else "fallback",
                staging="vector" if noise_dim % 4 == 0 and aligned else "scalar")


# ------------------------------------------------------------------------------------------------- helpers
def _d(t):
    return t.detach().cpu().double()


def bf16r(v):
    """to bf16 round-to-nearest-even (the kernels' (__bf16) conversion), in float64"""
    return v.float().bfloat16().double()


def f32r(v):
    return v.float().double()


def nchw(y, B, layer_or_side, C=None):
    """channels-last (B*H*H, C) -> (B, C, H, H)"""
    h = layer_or_side if C is not None else GEOM[layer_or_side][1]
    C = C if C is not None else y.shape[1]
    return y.reshape(B, h, h, C).permute(0, 3, 1, 2)


def cl(y):
    """(B, C, H, W) -> channels-last (B*H*W, C)"""
    B, C = y.shape[:2]
    return y.permute(0, 2, 3, 1).reshape(-1, C)


def _fl(faults):
    return dict((f, None) if isinstance(f, str) else f for f in faults)


# --------------------------------------------------------------------------------------------------- layer 1
def first_ref(noise, w1):
    """y1 = bf16(noise) @ bf16(w1) in the (B*16, 128) layout.  Returns (ref, M)."""
    x = bf16r(_d(noise).reshape(noise.shape[0], -1))
    w = bf16r(_d(w1)).reshape(w1.shape[0], 128, 16)
    y = torch.einsum("bk,kcp->bpc", x, w).reshape(-1, 128)
    M = torch.einsum("bk,kcp->bpc", x.abs(), w.abs()).reshape(-1, 128)
    return y, M


def where_l1(B):
    def f(idx):
        r, c = idx
        b, pos = divmod(r, 16)
        return (f"layer 1 sample {b} pixel ({pos // 4}, {pos % 4}) channel {c}: workgroup {c // L1_CH}, "
                f"wave {pos // 4}, batch tile {b // 16}" + ("" if B <= 256 else " (B > 256: GEMM fallback)"))
    return f


# ------------------------------------------------------------------------------------------- batch statistics
def chunk_of_rows(layer, B):
    """the bn_finalize chunk (workgroup 4 * group + class) each row of y2 / y3 belongs to"""
    _, oh, _ = GEOM[layer]
    b = torch.arange(B).repeat_interleave(oh * oh)
    oy = torch.arange(oh).repeat_interleave(oh).repeat(B)
    ox = torch.arange(oh).repeat(B * oh)
    return 4 * (b // S[layer]) + 2 * (oy % 2) + ox % 2


def stats_path(layer, B):
    """(P, chunks, shifted): roundings inside a partial, partials merged, shifted sums (see the module docstring)"""
    if layer == 1 and B <= 256:
        return 32, 0, False
    if layer == 1:
        rows = 16 * B
        ch = bn_row_chunks(rows)
        return -(-rows // ch) // 4 + 8, ch, True
    return 16, convt_chunks(layer, B), False


def stats_ref(y, layer, B, running_mean, running_var, nbt, *, faults=()):
    """Training-mode batch statistics of the kernel-produced y (rows, C) of layer 1, 2 or 3 (the statistics that
    normalise it in the next kernel) -> dict of (ref, E): mean, invstd, running_mean, running_var, and the integer
    num_batches_tracked.  faults (tests/test_simnn_gen_ref.py only): "biased_var"; "drop_last" (the last sample left
    out); ("chunk_twice", k) (partial k counted twice, layers 2 and 3); "momentum_swap"; ("nbt", k) (advanced k
    times)."""
    fl = _fl(faults)
    y = _d(y)
    rows, C = y.shape
    per = rows // B
    wgt = torch.ones(rows, dtype=torch.float64)
    if "drop_last" in fl:
        wgt[-per:] = 0.0
    if "chunk_twice" in fl:
        wgt[chunk_of_rows(layer, B) == fl["chunk_twice"]] = 2.0
    n = float(wgt.sum())
    mean = (wgt[:, None] * y).sum(0) / n
    dev = y - mean
    m2 = (wgt[:, None] * dev * dev).sum(0)
    # bounds from the unfaulted data
    n0 = float(rows)
    P, chunks, shifted = stats_path(layer, B)
    G = P + 8 * (-(-chunks // 16) + 16) + 8 if chunks else P
    D = (y - y.mean(0)).abs().amax(0)
    Emean = G * U * y.abs().amax(0)
    m2_0 = ((y - y.mean(0)) ** 2).sum(0)
    Em2 = G * U * (m2_0 + (n0 * D * D if shifted else 0.0)) + 4 * n0 * D * Emean
    var_b = m2 / n
    inv = 1.0 / torch.sqrt(var_b + EPS)
    vlo = ((m2_0 - Em2) / n0).clamp_min(0.0)
    Einv = 0.5 * (vlo + EPS) ** -1.5 * (Em2 / n0) + 4 * U * inv
    var_u = m2 / (n if "biased_var" in fl else max(n - 1, 1))
    Evar_u = Em2 / max(n0 - 1, 1)
    rm0, rv0 = _d(running_mean), _d(running_var)
    a, b = (MOMENTUM, 1 - MOMENTUM) if "momentum_swap" in fl else (1 - MOMENTUM, MOMENTUM)
    rm = a * rm0 + b * mean
    rv = a * rv0 + b * var_u
    Erm = MOMENTUM * Emean + 4 * U * (rm.abs() + mean.abs())
    Erv = MOMENTUM * Evar_u + 4 * U * (rv.abs() + var_u.abs())
    return dict(mean=(mean, Emean), invstd=(inv, Einv), running_mean=(rm, Erm), running_var=(rv, Erv),
                num_batches_tracked=int(nbt) + fl.get("nbt", 1) if "nbt" in fl else int(nbt) + 1)


def where_channel(layer, what):
    return lambda idx: f"layer {layer} {what} channel {idx[-1]}"


def check_stats(got, ref, layer, *, what=""):
    """got: dict name -> tensor (mean, invstd, running_mean, running_var) and num_batches_tracked as an int.
    Returns {name: worst |err| / bound}."""
    res = {}
    for name, g in got.items():
        if name == "num_batches_tracked":
            if int(g) != ref[name]:
                raise CheckError(f"{what} layer {layer} num_batches_tracked {int(g)} != {ref[name]}")
            continue
        r, E = ref[name]
        res[name] = check_abs(g.reshape(r.shape), r, E, what=f"{what} layer {layer} {name}",
                              where=where_channel(layer, name))
    return res


# ----------------------------------------------------------------------------------------------------- partials
def partials_ref(y, layer, B, *, faults=()):
    """Per-workgroup (n, mean, M2) of convt_s2_bn_kernel from the kernel-produced y (rows, Cout), float64.  Returns
    dict n (chunks,), mean, M2 (chunks, Cout) as (ref, E).  faults: "tail_pad_n" (the tail workgroup counts its padded
    samples, as zeros, in n, mean and M2)."""
    fl = _fl(faults)
    s = S[layer]
    ih, oh, C = GEOM[layer]
    groups = -(-B // s)
    Bp = groups * s
    y = nchw(_d(y), B, layer)
    yp = torch.zeros(Bp, C, oh, oh, dtype=torch.float64)
    yp[:B] = y
    valid = torch.zeros(Bp, dtype=torch.float64)
    valid[:B] = 1.0
    if "tail_pad_n" in fl:
        valid[:] = 1.0
    ns, means, m2s, Ems, Em2s = [], [], [], [], []
    for g in range(groups):
        blk = yp[g * s:(g + 1) * s]
        v = valid[g * s:(g + 1) * s]
        for qy in (0, 1):
            for qx in (0, 1):
                x = blk[:, :, qy::2, qx::2].permute(1, 0, 2, 3).reshape(C, s, ih * ih)       # (C, S, IH*IH)
                w = v[None, :, None].expand_as(x)
                n = float(w.sum()) / C
                mean = (x * w).sum((1, 2)) / n
                m2 = (w * (x - mean[:, None, None]) ** 2).sum((1, 2))
                Em = 18 * U * (x.abs() * w).amax((1, 2))
                ns.append(n)
                means.append(mean)
                m2s.append(m2)
                Ems.append(Em)
                Em2s.append(24 * U * m2 + n * Em * Em)
    n = torch.tensor(ns, dtype=torch.float64)
    return dict(n=(n, torch.zeros_like(n)), mean=(torch.stack(means), torch.stack(Ems)),
                m2=(torch.stack(m2s), torch.stack(Em2s)))


def where_partial(layer, B, name):
    def f(idx):
        k = idx[0]
        g, c = divmod(k, 4)
        s0 = g * S[layer]
        ch = f" channel {idx[1]}" if len(idx) > 1 else ""
        return (f"layer {layer} partial {name}: chunk {k} = workgroup (group {g}, class ({c >> 1}, {c & 1})), samples "
                f"{s0}..{min(s0 + S[layer], B) - 1}, finalize round {k // FINALIZE_ROUND} wave {k % 16}"
                + ch)
    return f


def check_partials(part, ref, layer, B, *, what=""):
    """part: (chunks, Cout, 3) from the kernel.  Returns {n, mean, m2: worst |err| / bound}."""
    part = part.detach().cpu().double()
    got = dict(n=part[:, 0, 0], mean=part[..., 1], m2=part[..., 2])
    if not torch.equal(part[..., 0], part[:, :1, 0].expand_as(part[..., 0])):
        raise CheckError(f"{what} layer {layer} partial n differs between the channels of a workgroup")
    res = {}
    for name, g in got.items():
        r, E = ref[name]
        res[name] = check_abs(g, r, E, what=f"{what} layer {layer} partial {name}",
                              where=where_partial(layer, B, name))
    return res


# ------------------------------------------------------------------------------------------------ staging
def stage(x, mean, invstd, gamma, beta, *, bf16=True, faults=()):
    """The kernels' BN + ReLU on load on channels-last x (rows, C): sc = fp32(invstd * gamma),
    v = fma(fp32(x - mean), sc, beta) rounded once to fp32, max(v, 0), then bf16 (RNE) when bf16.
    Returns (a, da): da = the spread of the operand over v +- 1 fp32 ulp (see the module docstring).
    faults: "no_relu", "no_gamma"."""
    fl = _fl(faults)
    x, mean, invstd, gamma, beta = (_d(t) for t in (x, mean, invstd, gamma, beta))
    sc = f32r(invstd if "no_gamma" in fl else invstd * gamma)
    v = f32r(f32r(x - mean) * sc + beta).float()
    act = (lambda t: t) if "no_relu" in fl else (lambda t: t.clamp_min(0.0))
    rnd = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
    a = rnd(act(v))
    lo = rnd(act(torch.nextafter(v, torch.tensor(-math.inf))))
    hi = rnd(act(torch.nextafter(v, torch.tensor(math.inf))))
    return a, (hi - lo).abs()


# ---------------------------------------------------------------------------------------------- layers 2 and 3
def convt_ref(yin, mean, invstd, gamma, beta, w, layer, B, *, faults=()):
    """convt_s2_bn_kernel's output (B*OH*OH, Cout) from its input yin (B*IH*IH, Cin) and the statistics it was given.
    Returns (ref, M, E) with E = RTOL M + conv(|da|, |w|).  faults: "no_relu", "no_gamma" (staging);
    "wrong_tap" (class (0, 0) reads kh = qy + 2a instead of 1 - qy + 2a); "no_halo" (a border pixel reads the
    neighbouring sample instead of zero)."""
    fl = _fl(faults)
    ih, oh, C = GEOM[layer]
    a, da = stage(yin, mean, invstd, gamma, beta, faults=[f for f in faults if f in ("no_relu", "no_gamma")])
    a, da = nchw(a, B, ih, CIN[layer]), nchw(da, B, ih, CIN[layer])
    wb = bf16r(_d(w))
    ct = lambda t, ww: F.conv_transpose2d(t, ww, stride=2, padding=1)  # noqa: E731
    if "no_halo" in fl:                      # samples stacked along H with no zero rows between them
        tall = lambda t: t.permute(1, 0, 2, 3).reshape(1, t.shape[1], B * ih, ih)  # noqa: E731
        back = lambda t: t.reshape(t.shape[1], B, oh, oh).permute(1, 0, 2, 3)     # noqa: E731
        y = back(ct(tall(a), wb))
    else:
        y = ct(a, wb)
    if "wrong_tap" in fl:
        yw = ct(a, wb[:, :, [1, 0, 3, 2], :])
        y[:, :, 0::2, 0::2] = yw[:, :, 0::2, 0::2]
    M = ct(a.abs(), wb.abs())
    E = RTOL[layer] * M + ct(da, wb.abs())
    return cl(y), cl(M), cl(E)


def where_convt(layer, B):
    ih, oh, C = GEOM[layer]
    s = S[layer]
    ptw = s * ih * ih // 64                       # pixel tiles per wave (TPW / CT)

    def f(idx):
        r, co = idx
        b, p = divmod(r, oh * oh)
        oy, ox = divmod(p, oh)
        cls = 2 * (oy & 1) + (ox & 1)
        px = (b % s) * ih * ih + (oy // 2) * ih + ox // 2
        return (f"layer {layer} sample {b} pixel ({oy}, {ox}) channel {co}: parity class ({oy & 1}, {ox & 1}), "
                f"workgroup {4 * (b // s) + cls}, wave {px // 16 // ptw} pixel tile {px // 16} C-tile {co // 16}")
    return f


# --------------------------------------------------------------------------------------------------- layer 4
def last_ref(y3, mean, invstd, gamma, beta, w4, B, *, faults=()):
    """convt_k5_bn_sigmoid_kernel: (B, 1, 20, 20) from y3 (B*256, 32).  Returns (ref, E).
    faults: "bf16_input" (the staged operand rounded to bf16)."""
    fl = _fl(faults)
    a, _ = stage(y3, mean, invstd, gamma, beta, bf16="bf16_input" in fl)
    a = nchw(a, B, 3)
    w = _d(w4)
    pre = F.conv_transpose2d(a, w)
    Mpre = F.conv_transpose2d(a.abs(), w.abs())
    o = torch.sigmoid(pre)
    E = 0.25 * N_PRE * U * Mpre + o * (1 - o) * U * pre.abs() + C_SIG * U * o
    return o, E


def where_last(idx):
    b, _, oy, ox = idx
    o = oy * 20 + ox
    return f"layer 4 sample {b} (workgroup {b}) pixel ({oy}, {ox}): thread {o}, wave {o // 64}"


# ------------------------------------------------------------------------------------------------ whole chain
def chain_ref(noise, ws, bns, *, rounding=True):
    """The float64 generator in train mode from noise (B, noise_dim[, 1, 1]); ws = 4 ConvTranspose2d weights; bns = 3 x
    (gamma, beta, running_mean, running_var, nbt).  rounding: the fused chain's rounding points (bf16 noise and
    weights of layers 1..3, bf16 staged operands of layers 2 and 3).  Returns (out (B, 1, 20, 20), [(running_mean,
    running_var, nbt)] x 3)."""
    r = bf16r if rounding else (lambda t: t)
    B = noise.shape[0]
    x = r(_d(noise).reshape(B, -1, 1, 1))
    stats = []
    y = F.conv_transpose2d(x, r(_d(ws[0])))
    for li in range(3):
        g, be, rm, rv, nbt = (bns[li][k] for k in range(5))
        g, be, rm, rv = _d(g), _d(be), _d(rm), _d(rv)
        n = y.numel() // y.shape[1]
        mean = y.mean((0, 2, 3))
        var = ((y - mean[:, None, None]) ** 2).sum((0, 2, 3))
        a = (y - mean[:, None, None]) / torch.sqrt(var / n + EPS)[:, None, None] * g[:, None, None] + be[:, None, None]
        a = a.clamp_min(0.0)
        stats.append(((1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var / (n - 1),
                      int(nbt) + 1))
        if li < 2:
            y = F.conv_transpose2d(r(a), r(_d(ws[li + 1])), stride=2, padding=1)
        else:
            y = F.conv_transpose2d(a, _d(ws[3]))
    return torch.sigmoid(y), stats
