"""float64 references and checkers for the patch-lowering kernels (csrc/lowering.hip) and the layer-wise pointwise
kernels (csrc/pointwise.hip up to gdm_cast), written from each operation's definition and not from the kernel's index
formulas.  A plain module next to simnn_gen_ref.py: tests/test_lowering_ref.py (CPU) checks it against independent
torch float64 evaluations and planted faults; tests/test_lowering_batch_gpu.py and tests/test_pointwise_edges_gpu.py
(GPU) hold the kernels to it on the shape tables at the end of the file.  Every checker returns a list of failure
strings (empty = pass), most of them together with the worst err / bound.

Rounding model.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16).  The reference always sees the kernel's own inputs
(the exactly representable fp32 / bf16 values, widened to float64), so what is bounded is the kernel's arithmetic only.

  im2col, permute_pc, cast, maxpool2: copies and comparisons -- bit-equal (one rounding to the destination type).
  col2im: a gather of `taps` terms summed in fp32 in any order: |got - ref| <= (taps - 1) u sum|terms|; a bf16
    destination adds one rounding, ub (|ref| + E); positions no window covers have taps = 0 and must be exactly 0
    (ReLU(0) = 0, sigmoid(0) = 0.5 exactly).  The fused sigmoid 1 / (1 + expf(-s)): an error E in s moves o by
    o (1 - o) E; what expf, the add and the divide contribute is measured (no device-library document states
    expf's error): at most 0.94 ulp of the result on MI355X over every fused-sigmoid case of the tables, so
    SIGMOID_ULPS = 4 x 0.94 and the bound is SIGMOID_ULPS 2^-23 o.
  column sums: (rows - 1) u colsum|x| for any summation order.
  BatchNorm apply, given the kernel's own mean and invstd: v = (y - mean) (invstd gamma) + beta has four roundings
    (subtract, scale product, multiply, add; fewer when contracted): 3 u |y - mean| |invstd gamma| + u |v|.
  BatchNorm backward, given the kernel's own out / mean / invstd: g = dout act'(out) carries <= 3 roundings, xhat 2,
    the product 1, and the sums run over R rows in a fixed order: E_dbeta = (R + 3) u sum|g|, E_dgamma = (R + 6) u
    sum|g xhat|; dy = gamma invstd (g - dbeta / R - xhat dgamma / R) inherits E_dbeta / R and |xhat| E_dgamma / R and
    adds <= 8 roundings of its own terms.
  BatchNorm statistics and Welford partials: no closed form on ill-conditioned channels; stats_ratios / partial_ratios
    give each deviation in its natural fp32 unit; STATS_MEASURED holds the maxima measured on MI355X per input
    family over the whole table and stats_bounds() allows MARGIN = 4 times them.
  Adam: one step from the kernel's own fp32 state (adam_ref): the bound follows adam_element's rounding points.

Mirrors of the launch plans (pointwise.hip row_chunks / chunk_rows / lanes per row, grid_for's caps, gdm_permute_pc's
kernel switch) are kept here the way simnn_gen_ref.py keeps the generator's.
"""
import math

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3
MARGIN = 4                                  # measured bounds are MARGIN x the measured maximum
SIGMOID_ULPS = MARGIN * 0.94                # 1 / (1 + expf(-s)): measured 0.939 ulp of the result (record "sigmoid_ulps")
# BatchNorm statistics (gdm_bn_act_fwd x 2, gdm_bn_stats, gdm_bn_finalize over rank partials) and chunk partials
# (gdm_bn_partials), maxima over BN_PAIRS and MERGE_CASES on MI355X in stats_ratios / partial_ratios units, per family
# of tests/test_pointwise_edges_gpu.py.  "bigmean" (mean 1e3, spread 1e-1): the Chan merges round every partial mean at
# 1e3, which costs the variance ~1e-4 relative; "special": the channel with one 1e4 outlier.
STATS_MEASURED = {
    "standard": dict(mean=1.07, invstd=10.99, running_mean=0.472, running_var=2.913, pmean=2.889, pm2=5.198),
    "bigmean": dict(mean=2.609, invstd=1231.4, running_mean=0.553, running_var=9.404, pmean=5.963, pm2=814.9),
    "special": dict(mean=1.07, invstd=733.2, running_mean=0.472, running_var=234.2, pmean=2.889, pm2=5.198),
}
F32_TINY = 2.0 ** -126

# ------------------------------------------------------------------------------------------------ plan mirrors
LOWERING_GRID_CAP = 8192                    # lowering.hip grid_for
POINTWISE_GRID_CAP = 4096                   # pointwise.hip grid_for
ADAM_GRID_CAP = 8192                        # gdm_adam_step: blocks of 256 threads x 4 elements
PERMUTE_WIDE_P = 512                        # gdm_permute_pc: 128 x 32 tiles from P >= 512, 32 x 32 below
FINALIZE_ROUND = 16 * 8                     # bn_finalize: chunks merged per round


def stats_bounds(family):
    """(bounds for check_stats, bounds for check_partials): MARGIN x the measured maxima"""
    m = STATS_MEASURED[family]
    return ({k: MARGIN * m[k] for k in ("mean", "invstd", "running_mean", "running_var")},
            dict(mean=MARGIN * m["pmean"], m2=MARGIN * m["pm2"]))


def grid_trips(total, cap=LOWERING_GRID_CAP):
    """trips of a grid-stride loop, one element per thread, 256-thread blocks capped at `cap`"""
    blocks = min(cap, max(1, (total + 255) // 256))
    return (total + blocks * 256 - 1) // (blocks * 256)


def adam_trips(n):
    """gdm_adam_step / gdm_adam_step_dev: four elements per thread, blocks capped at ADAM_GRID_CAP"""
    blocks = min(ADAM_GRID_CAP, max(1, (n // 4 + 255) // 256))
    return (n + blocks * 1024 - 1) // (blocks * 1024)


def row_chunks(rows):
    return min(64, max(1, (rows + 255) // 256))


def chunk_rows(rows):
    c = row_chunks(rows)
    return (rows + c - 1) // c


def chunk_of_rows(rows):
    """chunk index of every row"""
    return torch.arange(rows) // chunk_rows(rows)


def lanes_per_row(C):
    """bn_partial_stats' CW: the power of two >= min(C, 64)"""
    cw = 64
    while cw // 2 >= C and cw > 1:
        cw //= 2
    return cw


def permute_kernel(P):
    return "wide" if P >= PERMUTE_WIDE_P else "narrow"


def bn_regimes(rows, C):
    return dict(cw=lanes_per_row(C), chunks=row_chunks(rows), chunk_rows=chunk_rows(rows),
                capped=(rows + 255) // 256 > 64, idle_lanes=C < 64 and lanes_per_row(C) != C,
                column_blocks=(C + 63) // 64)


# ------------------------------------------------------------------------------------------------- helpers
def _d(t):
    return t.detach().cpu().double()


def rnd(v, dtype):
    """float64 -> dtype, round to nearest even (through fp32: exact for values that are fp32 already)"""
    return v.float().to(dtype)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def check_bits(got, want, *, what=""):
    """bit equality (tells +0 from -0), with the first differing element named"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{what}: shape / dtype {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"]
    ne = bits(got) != bits(want)
    if not bool(ne.any()):
        return []
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return [f"{what}: {int(ne.sum())} element(s) differ; first at {list(idx)}: got {float(got[idx])!r} "
            f"want {float(want[idx])!r}"]


def check_bound(got, ref, E, *, what=""):
    """|got - ref| <= E per element; returns (failures, worst err / bound)"""
    got, ref, E = _d(got).reshape(ref.shape), ref.double(), E.double()
    err = (got - ref).abs()
    bad = ~(err <= E)                       # also catches NaN
    if not bool(bad.any()):                 # (E = 0 with err = 0 gives 0 / tiny = 0)
        return [], float((err / E.clamp_min(1e-300)).max()) if err.numel() else 0.0
    ratio = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    worst = float(torch.nan_to_num(ratio, nan=math.inf).max()) if ratio.numel() else 0.0
    if not bool(bad.any()):
        return [], worst
    flat = int(torch.nan_to_num(ratio, nan=math.inf).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return [f"{what}: {int(bad.sum())} element(s) out of bound; worst at {list(idx)}: got {float(got[idx]):.9g} ref "
            f"{float(ref[idx]):.9g} |err| {float(err[idx]):.3g} > bound {float(E[idx]):.3g}"], worst


def act_ref(v, act, slope=0.0):
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def act_grad_from_out(o, act, slope=0.0):
    if act == ACT_RELU:
        return (o > 0).double()
    if act == ACT_LEAKY:
        return torch.where(o > 0, torch.ones_like(o), torch.full_like(o, slope))
    if act == ACT_SIGMOID:
        return o * (1 - o)
    return torch.ones_like(o)


def act_bound(ref_pre, E_pre, act, slope=0.0):
    """error of act(s) when s carries E_pre: the slope of the activation times E_pre, plus the activation's own
    roundings (sigmoid: SIGMOID_ULPS of the result, measured)"""
    if act == ACT_SIGMOID:
        o = act_ref(ref_pre, act)
        return (o * (1 - o) + E_pre) * E_pre + SIGMOID_ULPS * 2.0 ** -23 * o + F32_TINY
    if act == ACT_LEAKY:
        return E_pre + U * ref_pre.abs() * abs(slope)
    return E_pre


def store_bound(ref, E, dtype):
    """+ one rounding to a bf16 destination"""
    return E + UB * (ref.abs() + E) if dtype == torch.bfloat16 else E


# -------------------------------------------------------------------------------------------------- im2col
def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _channels_last(src, planar, B, H, W, C):
    s = _d(src)
    return s.reshape(B, C, H, W).permute(0, 2, 3, 1) if planar else s.reshape(B, H, W, C)


def im2col_ref(src, *, planar, B, H, W, C, KH, KW, stride, pad, OH, OW):
    """cols[(b, oh, ow), (c, kh, kw)] = zero-padded src[b, oh s - p + kh, ow s - p + kw, c]; float64"""
    x = _channels_last(src, planar, B, H, W, C)
    hp, wp = max(H + 2 * pad, (OH - 1) * stride + KH), max(W + 2 * pad, (OW - 1) * stride + KW)
    padded = torch.zeros(B, hp, wp, C, dtype=torch.float64)
    padded[:, pad:pad + H, pad:pad + W] = x
    cols = torch.empty(B, OH, OW, C, KH, KW, dtype=torch.float64)
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(KH):
                cols[:, oh, ow, :, kh, :] = padded[:, oh * stride + kh, ow * stride:ow * stride + KW].transpose(1, 2)
    return cols.reshape(B * OH * OW, C * KH * KW)


# -------------------------------------------------------------------------------------------------- col2im
def col2im_ref(cols, *, B, H, W, C, KH, KW, stride, pad, OH, OW, tap_major=False, planar=False, act=ACT_NONE,
               faults=()):
    """Scatter form: every (oh, ow, kh, kw) adds cols[(b, oh, ow), (c, kh, kw)] into dst[b, oh s - p + kh,
    ow s - p + kw, c] when that position is inside.  Returns dict(pre, out, mag = sum|terms|, taps), each in the
    destination's layout ((B,C,H,W) if planar else (B,H,W,C)), float64.
    faults: "short_tap" = the highest tap row of every window is left out; "torch_order" = tap-major columns read in
    torch's (c, kh, kw) order."""
    c = _d(cols).reshape(B, OH, OW, C * KH * KW)
    if tap_major and "torch_order" not in faults:
        c = c.reshape(B, OH, OW, KH, KW, C)
    else:
        c = c.reshape(B, OH, OW, C, KH, KW).permute(0, 1, 2, 4, 5, 3)
    hp, wp = max(H + pad, (OH - 1) * stride + KH), max(W + pad, (OW - 1) * stride + KW)
    acc = torch.zeros(3, B, hp, wp, C, dtype=torch.float64)
    kh_end = KH - 1 if "short_tap" in faults else KH
    for oh in range(OH):
        for ow in range(OW):
            t = c[:, oh, ow, :kh_end]
            win = acc[:, :, oh * stride:oh * stride + kh_end, ow * stride:ow * stride + KW]
            win[0] += t
            win[1] += t.abs()
            win[2] += 1.0
    pre, mag, taps = (a[:, pad:pad + H, pad:pad + W] for a in acc)
    if planar:
        pre, mag, taps = (a.permute(0, 3, 1, 2) for a in (pre, mag, taps))
    pre, mag, taps = pre.contiguous(), mag.contiguous(), taps.contiguous()
    return dict(pre=pre, out=act_ref(pre, act), mag=mag, taps=taps, act=act)


def col2im_bound(ref, dst_dtype):
    E_pre = (ref["taps"] - 1).clamp_min(0) * U * ref["mag"]
    E = torch.where(ref["taps"] > 0, act_bound(ref["pre"], E_pre, ref["act"]), torch.zeros_like(E_pre))
    return store_bound(ref["out"], E, dst_dtype)


def check_col2im(got, ref, dst_dtype, *, what=""):
    """(failures, worst err / bound).  Uncovered positions (taps = 0) are held to act(0) exactly."""
    fails, worst = check_bound(got, ref["out"], col2im_bound(ref, dst_dtype), what=what)
    return fails, worst


# ---------------------------------------------------------------------------------------------- permute_pc
def permute_ref(src, B, P, C, out_dtype, *, faults=()):
    """(B, P, C) -> (B, C, P), rounded once to out_dtype.  fault "tile_edge": the square block at the high end of P
    (the last tile's edge) is written transposed within itself, p and c offsets swapped."""
    x = _d(src).reshape(B, P, C)
    out = x.permute(0, 2, 1).contiguous()
    if "tile_edge" in faults:
        n = min(32, P, C)
        p0 = P - n
        out[:, :n, p0:p0 + n] = out[:, :n, p0:p0 + n].transpose(1, 2).clone()
    return rnd(out, out_dtype)


# ------------------------------------------------------------------------------------------------ maxpool2
def maxpool2_ref(x, B, H, W, C, *, faults=()):
    """2x2 / stride 2 floor pooling of channels-last x: (values (B,OH,OW,C) float64, idx uint8 = window position
    dy*2+dx of the FIRST maximum in scan order).  fault "last_max": the last maximum instead."""
    v = _d(x).reshape(B, H, W, C)
    OH, OW = H // 2, W // 2
    win = [v[:, dy:2 * OH:2, dx:2 * OW:2] for dy in (0, 1) for dx in (0, 1)]
    m, pos = win[0].clone(), torch.zeros(B, OH, OW, C, dtype=torch.uint8)
    for k in (1, 2, 3):
        take = win[k] >= m if "last_max" in faults else win[k] > m
        m = torch.where(take, win[k], m)
        pos = torch.where(take, torch.full_like(pos, k), pos)
    return m, pos


def maxpool2_bwd_ref(dout, idx, B, H, W, C, *, faults=()):
    """dense zeros (B,H,W,C) with dout routed to the window position idx names; the odd last row / column stay 0.
    fault "odd_row": for odd H the gradient of the last pooled row lands one row lower, in the dropped row."""
    g = _d(dout).reshape(B, H // 2, W // 2, C)
    idx = idx.detach().cpu().reshape(B, H // 2, W // 2, C)
    dx = torch.zeros(B, H, W, C, dtype=torch.float64)
    OH, OW = H // 2, W // 2
    for k in range(4):
        dy, dxx = k // 2, k % 2
        dx[:, dy:2 * OH:2, dxx:2 * OW:2] = torch.where(idx == k, g, torch.zeros_like(g))
    if "odd_row" in faults and H % 2 == 1:
        dx[:, H - 1] = dx[:, H - 2]
        dx[:, H - 2] = 0
    return dx


def pool_input(B, H, W, C, dtype):
    """values with planted ties: per window class (cycled over the windows) two equal maxima at each pair of positions,
    all four equal, and +0.0 against -0.0 in both orders"""
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C))
    OH, OW = H // 2, W // 2
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                k = (b * OH * OW + oh * OW + ow) % 10
                win = x[b, 2 * oh:2 * oh + 2, 2 * ow:2 * ow + 2]        # (2, 2, C) view
                if k < 6:
                    a, c = pairs[k]
                    win[a // 2, a % 2] = win[c // 2, c % 2] = win.reshape(4, C).max(0).values + 1.0
                elif k == 6:
                    win[:] = win[0, 0]
                elif k == 7:
                    win[:] = torch.tensor([[-0.0, 0.0], [-1.0, 0.0]]).reshape(2, 2, 1)
                elif k == 8:
                    win[:] = torch.tensor([[0.0, -0.0], [-0.0, -2.0]]).reshape(2, 2, 1)
    return x.to(dtype)


# ----------------------------------------------------------------------------------------------- batch norm
def bn_stats_ref(y, running_mean, running_var, nbt, *, calls=1, momentum=0.1, eps=1e-5, faults=()):
    """two-pass float64 mean / biased variance of y (rows, C), invstd, and the running statistics after `calls`
    training-mode calls on the same y (unbiased variance blended in).  fault "biased_running": the biased one."""
    y = _d(y)
    R = y.shape[0]
    mean = y.mean(0)
    m2 = ((y - mean) ** 2).sum(0)
    var = m2 / R
    var_u = var if "biased_running" in faults else m2 / max(R - 1, 1)
    rm, rv = _d(running_mean).clone(), _d(running_var).clone()
    for _ in range(calls):
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var_u
    return dict(mean=mean, var=var, m2=m2, invstd=1.0 / torch.sqrt(var + eps), running_mean=rm, running_var=rv,
                num_batches_tracked=int(nbt) + calls, absmax=y.abs().max(0).values,
                dev=(y - mean).abs().max(0).values)


def stats_ratios(got, ref):
    """The measured quantities of the statistics check, each |got - ref| over its natural fp32 scale:
      mean, running_mean: u max|y|;  invstd: u invstd (a relative error in units of u);
      running_var: u (|running_var| + var).
    A zero scale (constant zero channel) demands exact agreement (ratio 0 or inf)."""
    out = {}
    scales = dict(mean=U * ref["absmax"], running_mean=U * (ref["absmax"] + ref["running_mean"].abs()),
                  invstd=U * ref["invstd"], running_var=U * (ref["running_var"].abs() + ref["var"]))
    for k, s in scales.items():
        if k in got and got[k] is not None:
            err = (_d(got[k]) - ref[k]).abs()
            r = torch.where(s > 0, err / s.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
            out[k] = float(torch.nan_to_num(r, nan=math.inf).max())
    return out


def check_stats(got, ref, bounds, *, what=""):
    """got: dict of tensors (mean, invstd, running_mean, running_var) + num_batches_tracked; bounds: name -> allowed
    ratio (stats_ratios' units).  Returns (failures, ratios)."""
    ratios = stats_ratios(got, ref)
    fails = [f"{what}: {k} off by {v:.3g} units, allowed {bounds[k]:.3g}" for k, v in ratios.items()
             if not v <= bounds[k]]
    if "num_batches_tracked" in got and int(got["num_batches_tracked"]) != ref["num_batches_tracked"]:
        fails.append(f"{what}: num_batches_tracked {int(got['num_batches_tracked'])} != {ref['num_batches_tracked']}")
    return fails, ratios


def bn_apply_ref(y, gamma, beta, mean, invstd, act, out_dtype):
    """act((y - mean) invstd gamma + beta) from GIVEN statistics (the kernel's own): (ref, bound)"""
    y, gamma, beta, mean, invstd = (_d(t) for t in (y, gamma, beta, mean, invstd))
    alpha = invstd * gamma
    pre = (y - mean) * alpha + beta
    E_pre = 3 * U * (y - mean).abs() * alpha.abs() + U * pre.abs()
    ref = act_ref(pre, act)
    return ref, store_bound(ref, act_bound(pre, E_pre, act), out_dtype)


def bn_bwd_ref(dout, out, y, gamma, mean, invstd, act):
    """gdm.h's backward from the kernel's own out / mean / invstd: dict name -> (ref, bound)"""
    dout, out, y, gamma, mean, invstd = (_d(t) for t in (dout, out, y, gamma, mean, invstd))
    R = y.shape[0]
    g = dout * act_grad_from_out(out, act)
    xhat = (y - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    E_db = (R + 3) * U * g.abs().sum(0)
    E_dg = (R + 6) * U * (g * xhat).abs().sum(0)
    k = (gamma * invstd).abs()
    dy = gamma * invstd * (g - dbeta / R - xhat * dgamma / R)
    E_dy = k * ((E_db + xhat.abs() * E_dg) / R + 8 * U * (g.abs() + dbeta.abs() / R + (xhat * dgamma).abs() / R))
    return dict(dy=(dy, E_dy), dgamma=(dgamma, E_dg), dbeta=(dbeta, E_db))


def partials_ref(y):
    """(n, mean, M2) per (row chunk, channel) in float64, plus each chunk's max|y| and max|y - mean|"""
    y = _d(y)
    rows, C = y.shape
    k, cr = row_chunks(rows), chunk_rows(rows)
    res = {name: torch.zeros(k, C, dtype=torch.float64) for name in ("n", "mean", "m2", "absmax", "dev")}
    for j in range(k):
        part = y[j * cr:min(rows, (j + 1) * cr)]
        if part.shape[0] == 0:
            continue
        mu = part.mean(0)
        res["n"][j], res["mean"][j], res["m2"][j] = part.shape[0], mu, ((part - mu) ** 2).sum(0)
        res["absmax"][j], res["dev"][j] = part.abs().max(0).values, (part - mu).abs().max(0).values
    return res


def partial_ratios(part, ref):
    """n must be exact; mean over u max|y|, M2 over u (M2 + n dev^2) of its chunk (zero scale = exact)"""
    p = _d(part)
    out = {"n_exact": bool(torch.equal(p[..., 0], ref["n"]))}
    for name, i, s in (("mean", 1, U * ref["absmax"]), ("m2", 2, U * (ref["m2"] + ref["n"] * ref["dev"] ** 2))):
        err = (p[..., i] - ref[name]).abs()
        r = torch.where(s > 0, err / s.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
        out[name] = float(torch.nan_to_num(r, nan=math.inf).max())
    return out


def check_partials(part, ref, bounds, *, what=""):
    r = partial_ratios(part, ref)
    fails = [] if r["n_exact"] else [f"{what}: a chunk's row count differs from the chunk map"]
    fails += [f"{what}: partial {k} off by {r[k]:.3g} units, allowed {bounds[k]:.3g}" for k in ("mean", "m2")
              if not r[k] <= bounds[k]]
    return fails, r


def merge_partials_ref(part, rows, running_mean, running_var, nbt, *, momentum=0.1, eps=1e-5, faults=()):
    """Chan's merge of (chunks, C, 3) triples in float64, chunk by chunk: what gdm_bn_finalize makes of them, in the
    form of bn_stats_ref's result.  faults: ("twice", k) counts chunk k twice."""
    p = _d(part)
    order = list(range(p.shape[0]))
    for f in faults:
        if isinstance(f, tuple) and f[0] == "twice":
            order.insert(f[1], f[1])
    n = torch.zeros(p.shape[1], dtype=torch.float64)
    mean, m2 = n.clone(), n.clone()
    for j in order:
        bn, bm, b2 = p[j, :, 0], p[j, :, 1], p[j, :, 2]
        tot = (n + bn).clamp_min(1e-300)
        d = bm - mean
        mean = mean + d * bn / tot
        m2 = m2 + b2 + d * d * n * bn / tot
        n = n + bn
    var = m2 / rows
    rm = (1 - momentum) * _d(running_mean) + momentum * mean
    rv = (1 - momentum) * _d(running_var) + momentum * m2 / max(rows - 1, 1)
    return dict(mean=mean, invstd=1.0 / torch.sqrt(var + eps), running_mean=rm, running_var=rv,
                num_batches_tracked=int(nbt) + 1)


# --------------------------------------------------------------------------------------------------- colsum
def colsum_ref(x):
    x = _d(x)
    return x.sum(0), (x.shape[0] - 1) * U * x.abs().sum(0)


# ----------------------------------------------------------------------------------------------------- Adam
def adam_corrections(step, lr, beta1, beta2):
    """torch's host-side doubles: (step_size, sqrt(bias_correction2))"""
    return lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)


def adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0, *, faults=()):
    """ONE step of torch.optim.Adam's single-tensor algorithm (no amsgrad, no weight decay) in float64 on the given
    state, gradient scaled by grad_scale first.  The hyper-parameters are the values the C ABI receives (floats).
    Returns dict name -> (ref, bound) for p, m, v.  The bound follows adam_element (gdm_common.h):
      gj = fl(g gs)                              E_g = u |gj|
      mj = fl(w1 fl(gj - m) + m)   (or its mirrored form for w1 >= 0.5)
                                                 E_m = w1 E_g + max(w1, 1 - w1) u |gj - m| + u |mj|
      vj = fl(fl(omb2 gj) gj + fl(v beta2))      E_v = 2 omb2 |gj| E_g + u (omb2 gj^2 + beta2 v + vj)
      den = fl(fl(sqrtf(vj)) / bc2s) + eps       E_d = E_v / (2 sqrt(vj) bc2s) + 3 u sqrt(vj) / bc2s + u den
                                                 (sqrt, the fp32 bc2s, the divide; the add)
      p' = fl(p - ss fl(mj / den))               E_p = ss (E_m / den + |mj| E_d / den^2 + 2 u |mj / den|) + ulp(p')
    (the fp32 step size and the divide give the 2 u; ulp(p') is the final rounding, "1 ulp of p").  1 - beta in fp32 is
    exact for beta in [0.5, 1] (Sterbenz).  First-order terms carry a factor 1.01.
    fault ("tail", n): the last n % 4 elements are left as they were."""
    p, g, m, v = (_d(t) for t in (p, g, m, v))
    ss, bc2s = adam_corrections(step, lr, beta1, beta2)
    w1, omb2 = 1.0 - beta1, 1.0 - beta2
    gj = g * grad_scale
    E_g = U * gj.abs()
    mj = m + w1 * (gj - m)
    E_m = w1 * E_g + max(w1, 1 - w1) * U * (gj - m).abs() + U * mj.abs()
    vj = beta2 * v + omb2 * gj * gj
    E_v = 2 * omb2 * gj.abs() * E_g + U * (omb2 * gj * gj + beta2 * v + vj)
    sq = vj.sqrt()
    den = sq / bc2s + eps
    E_d = E_v / (2 * sq * bc2s).clamp_min(1e-300) + 3 * U * sq / bc2s + U * den
    E_d = torch.minimum(E_d, E_v.sqrt() / bc2s + 3 * U * sq / bc2s + U * den)      # sqrt is 1/2-Hoelder at 0
    q = mj / den
    pn = p - ss * q
    ulp_p = torch.ldexp(torch.ones_like(pn), (torch.frexp(pn.abs())[1] - 24).to(torch.int32)) * (pn != 0)
    E_p = 1.01 * ss * (E_m / den + mj.abs() * E_d / den ** 2 + 2 * U * q.abs()) + ulp_p + 2.0 ** -149
    res = dict(p=(pn, E_p), m=(mj, 1.01 * E_m + 2.0 ** -149), v=(vj, 1.01 * E_v + 2.0 ** -149))
    for f in faults:
        if isinstance(f, tuple) and f[0] == "tail" and f[1] % 4:
            t = f[1] % 4
            for name, old in (("p", p), ("m", m), ("v", v)):
                res[name][0][-t:] = old[-t:]
    return res


def check_adam(got, ref, *, what=""):
    """got: dict p, m, v.  Returns (failures, worst ratios)"""
    fails, worst = [], {}
    for k in ("p", "m", "v"):
        f, w = check_bound(got[k], ref[k][0], ref[k][1], what=f"{what} {k}")
        fails += f
        worst[k] = w
    return fails, worst


# ------------------------------------------------------------------------------------------- BCE, criterion, head
def bce_terms(x, y):
    """per-element terms of oracle.steps.bce_with_logits, float64"""
    x = _d(x)
    return torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def sum_bound(terms, n_round=4):
    """a fixed-order fp32 sum of n terms, each carrying n_round roundings of its own: (n - 1 + n_round) u sum|terms|"""
    t = terms.abs()
    return (t.numel() - 1 + n_round) * U * float(t.sum())


# ------------------------------------------------------------------------------------------------ shape tables
def geom(name, planar, B, H, W, C, KH, KW, stride, pad, **kw):
    """One lowering geometry.  (H, W) is the image side: im2col's source, col2im's destination; (OH, OW) the column
    grid.  For a transposed convolution the image is the layer's OUTPUT, which gives the same relation."""
    return dict(name=name, planar=planar, B=B, H=H, W=W, C=C, KH=KH, KW=KW, stride=stride, pad=pad,
                OH=out_size(H, KH, stride, pad), OW=out_size(W, KW, stride, pad), **kw)


EDGE_GEOMS = [
    geom("edge k3x2", False, 3, 9, 8, 4, 3, 2, 1, 1),
    geom("edge k2x5", False, 3, 7, 11, 3, 2, 5, 1, 1),
    geom("edge stride 3", False, 3, 11, 13, 5, 4, 4, 3, 1),
    geom("edge pad 0", False, 3, 9, 10, 4, 3, 3, 1, 0),
    geom("edge k5 s1 p2", False, 3, 7, 9, 3, 5, 5, 1, 2),
    geom("edge uncovered rows", False, 3, 10, 10, 4, 3, 3, 2, 0),          # OH = 4: row / column 9 is in no window
    geom("edge one window", False, 3, 4, 4, 6, 4, 4, 1, 0),
    geom("edge C=1", False, 3, 9, 7, 1, 3, 3, 2, 1),
    geom("edge C=33 planar", True, 3, 9, 7, 33, 3, 3, 2, 1),
]
IM2COL_GEOMS = [
    geom("dcnn conv1 T=50", True, 3, 128, 50, 2, 4, 4, 2, 1),
    geom("dcnn conv1 T=37", True, 3, 128, 37, 2, 4, 4, 2, 1),
    geom("dcnn conv1 B=1", True, 1, 128, 50, 2, 4, 4, 2, 1),
    geom("dcnn conv2", False, 3, 64, 25, 16, 4, 4, 2, 1),
    geom("simnn conv1 22x30", True, 3, 22, 30, 1, 3, 3, 1, 1),
    geom("simnn conv2 11x15", False, 3, 11, 15, 16, 3, 3, 1, 1),
    geom("gen bwd dy 20x20", False, 3, 20, 20, 1, 5, 5, 1, 0),
    geom("gen bwd dy 16x16", False, 3, 16, 16, 32, 4, 4, 2, 1),
    geom("gen bwd dy 8x8", False, 3, 8, 8, 64, 4, 4, 2, 1),
    geom("gen bwd dy 4x4", False, 3, 4, 4, 128, 4, 4, 1, 0),
] + EDGE_GEOMS + [geom("two trips", False, 3, 32, 32, 96, 3, 3, 1, 1)]
COL2IM_GEOMS = [
    geom("dcnn dX conv2", False, 3, 64, 25, 16, 4, 4, 2, 1),
    geom("dcnn dX conv1 T=50", True, 3, 128, 50, 2, 4, 4, 2, 1),
    geom("dcnn dX conv1 T=37", True, 3, 128, 37, 2, 4, 4, 2, 1),
    geom("simnn dX conv2 11x15", False, 3, 11, 15, 16, 3, 3, 1, 1),
    geom("simnn dX conv1 22x30", True, 3, 22, 30, 1, 3, 3, 1, 1),
    geom("gen fwd 4->8", False, 3, 8, 8, 64, 4, 4, 2, 1, tap_major=True, act=ACT_RELU),
    geom("gen fwd 8->16", False, 3, 16, 16, 32, 4, 4, 2, 1, tap_major=True),
    geom("gen fwd 8->16 B=1", False, 1, 16, 16, 32, 4, 4, 2, 1, tap_major=True),
    geom("gen fwd 16->20 sigmoid", True, 3, 20, 20, 1, 5, 5, 1, 0, act=ACT_SIGMOID),
] + EDGE_GEOMS + [geom("edge uncovered rows sigmoid", False, 3, 10, 10, 4, 3, 3, 2, 0, act=ACT_SIGMOID),
                  geom("edge tap-major k2x5 planar", True, 3, 7, 11, 3, 2, 5, 1, 1, tap_major=True),
                  geom("two trips", False, 3, 64, 64, 180, 4, 4, 2, 1)]


def im2col_elements(g):
    return g["B"] * g["OH"] * g["OW"] * g["C"] * g["KH"] * g["KW"]


def col2im_elements(g):
    return g["B"] * g["H"] * g["W"] * g["C"]


PERMUTE_SHAPES = [(2, 400, 1), (3, 384, 32), (2, 511, 33), (2, 512, 33), (2, 641, 70), (128, 16, 64), (2, 2048, 32)]
POOL_SHAPES = [(3, 22, 30, 16), (3, 11, 15, 16), (3, 2, 2, 16), (3, 22, 30, 5), (3, 11, 15, 5), (1, 2, 2, 5)]
BN_ROWS = [2, 255, 256, 257, 513, 16384, 16385, 65536]
BN_CHANNELS = [1, 2, 3, 5, 17, 32, 33, 64, 65, 100]
# (257, 9) is not in the channel list above: it is there for the one lanes-per-row value (16) the list does not reach
BN_PAIRS = [(257, 9), (2, 33), (2, 100), (255, 1), (255, 65), (256, 2), (256, 64), (257, 3), (257, 100), (513, 5), (513, 17),
            (16384, 32), (16384, 2), (16385, 3), (16385, 33), (65536, 32), (65536, 100)]
COLSUM_ROWS = [1, 3, 255, 257, 16385]
COLSUM_COLS = [1, 63, 65, 300]
BIAS_ACT_SHAPES = [(1, 1), (300, 77), (4100, 257)]          # n = 1, a tail, and a second trip of pointwise.hip's loop
ADAM_N = [1, 3, 4, 5, 1023, 1027, 8388608 + 1027]
LOSS_N = [1, 1023, 1025, 65536]
HEAD_N = [(1, 1), (9, 5), (65536, 30001)]
MERGE_CASES = [((600,), 8), ((300, 300), 8), ((200, 200, 200), 8), ((75,) * 8, 8), ((5, 300), 8),
               ((16384, 16384, 16384), 8)]       # (rows of each shard, channels)
