"""float64 references for model 2's bf16 kernels: the fused discriminator (csrc/mmgan_dcnn.hip) with the kernel's own
roundings and mirrors of its launch plan, and the generator blocks Linear + BatchNorm1d + activation
(csrc/linear_bn.hip) with element bounds.

A plain module next to trunk_ref.py: tests/test_mmgan_batch_gpu.py (GPU) and tests/test_mmgan_ref.py (CPU) import it.
The checker is trunk_ref.check_elementwise; ulp and CheckError come from there too.

The fused DCNN: mirrors of its launch plan -- n_blocks (workgroups for B samples on `cap` = 7/8 of the CUs) and the
sample -> (workgroup, round) assignment b = blockIdx.x + k * gridDim.x -- so that a test can prove which regime each
case runs (one sample per workgroup, several rounds, an uneven last round, a workgroup that holds both labels).

Rounding model.  u = 2^-24.  bf16 x bf16 products are exact in fp32; a sum of n terms with fp32 roundings, in any
order, is off by at most n * u * sum |terms| where n is the number of roundings on the longest path to the result.

Fused DCNN (dcnn_ref).  The reference mirrors every rounding the kernel makes: the input planes to bf16 (RNE) as
x_store does (mmgan_dcnn.hip:191); W1, W2, Wfc to bf16 as the pack does (:98), biases fp32; h1 = bf16(leaky(z1))
(:255) and h2 = bf16(leaky(z2)) (:303) with the fp32 constant 0.2f; dl = (sigmoid(z) - y) / cnt with (y, cnt) chosen
per sample by b < bsplit (:330-332); gy2 = dl * wfc * (h2 > 0 ? 1 : 0.2) summed unrounded into db2 and rounded to
bf16 for conv2's backward (:352-354); dy1 = conv2^T(bf16(gy2), W2) * (h1 > 0 ? 1 : 0.2) summed unrounded into db1
and rounded to bf16 for dW1 (:436-438); dWfc = sum dl h2 (:351); loss = sum (max(z,0) - z y + log1p(exp(-|z|))) / cnt.
What is left between kernel and reference is fp32 accumulation and the rare element whose fp32 value rounds to the
other bf16 neighbour (or falls on the other side of 0 for a LeakyReLU').  A worst-case per-element bound that grants
every possibly-affected element its one-ulp slack does not bind: at T = 50 about 30 % of h2 lie within the worst-case
accumulation bound (257 u M) of a bf16 rounding boundary.  So the outputs are checked per tensor, relative to the
magnitude M (the same computation on absolute values; unlike ||ref|| it does not shrink when a sum cancels):
    ||got - ref||_2 / ||M||_2 <= RL_BF16 = 5e-5.
The fp32 accumulation contributes about sqrt(n) u (n <= 1.2e3 roundings on the longest path at B = 512: ~2e-6);
a neighbour rounding moves one term by 2^-8 of itself, and those are a small fraction of the terms, with random signs.
What the bound must see: one sample dropped from (or added twice to) the gradients moves a weight-gradient tensor by
~1/B of M when the sample's dl is typical, less when it is small; at B = 512 (tests/test_mmgan_ref.py) the smallest
such fault, a first-segment sample counted twice, moves dWfc by 2.6e-4 of ||M||, and an unrounded input moves the
logits by 5.7e-5: RL_BF16 = 5e-5 lies below 1/B = 2.0e-3 and below every injected fault.
The exact-fp32 parity path (functional.dcnn_forward / dcnn_backward, dcnn_ref(bf16=False)) has no roundings to mirror
and is held to RL_F32 = 1e-5.
Measured on MI355X over the table of tests/test_mmgan_batch_gpu.py (worst ||err|| / ||M|| over the bound): fused bf16
logits 0.033, loss 0.15, dW1 0.42, db1 0.006, dW2 0.17, db2 0.062, dWfc 0.26, dbfc 0.22; fp32 parity path at b = 256
<= 0.02 (dWfc), the rest <= 0.006.

Linear + BatchNorm1d + activation.  The kernel splits both operands: x = xh + xl (+ ex), w = wh + wl (+ ew), all bf16,
|x - xh| <= 2^-8 |x|, |ex| <= 2^-8 |x - xh| <= 2^-16 |x|, and accumulates xh wh + xh wl + xl wh (linear_bn.hip:
128-158).  The three products are exact; x w minus that sum is ex w' + x' ew + xl wl (x' = xh + xl), at most
3.05 * 2^-16 |x||w|.  The fp32 accumulation: 3 K products (+ zero padding) and the bias, n = 3 K + 2 roundings.
So |y - y64| <= E_y = (3.05 * 2^-16 + (3K + 2) u) * sum_k |x_k w_k| + |b| u.  Everything after y is carried as an
interval bound: mean = sum y / M (4 waves of sums, n <= M + 6), m2 = sum (y - mean)^2 computed from the kernel's own
mean (error 2 |y - mean| (E_y + E_mean) + (M + 8) u per term), invstd = 1 / sqrt(m2 / M + eps) (derivative bound
plus 4 u), out = act((y - mean) * invstd * gamma + beta) with act' <= 1 (NONE, RELU) or 1/4 (SIGMOID) plus 20 u of
the sigmoid's own arithmetic.  Running statistics: rm <- (1 - m) rm + m mean, rv <- (1 - m) rv + m m2 / (M - 1) (the
unbiased variance), applied groups x stat_repeats times in group order (:217-226), 4 u per update.
Measured on MI355X over the table of tests/test_mmgan_batch_gpu.py (worst |err| / bound): y 0.18, out 0.18,
save_mean 0.067, save_invstd 0.37, running_mean 0.066, running_var 0.032.  A dropped xh wl term exceeds the y bound
7-27x (tests/test_mmgan_ref.py).
"""

import torch

from trunk_ref import CheckError, check_elementwise, ulp  # noqa: F401  (re-exported for the mmgan tests)

U = 2.0 ** -24
T_VALUES = (50, 48, 34, 32, 18, 16)


def dcnn_batches(cap):
    """the batch sizes of tests/test_mmgan_batch_gpu.py's fused-DCNN table (T = 50)"""
    return [1, 2, 12, cap, cap + 1, 512, 2 * cap + 1]


def dcnn_splits(B):
    """its label splits: one segment, either way round, halves, and an odd split inside the workgroups' rounds"""
    return sorted({0, B, B // 2, min(B, 2 * (B // 3) + 1)})


# ------------------------------------------------------------------------------------------ schedule mirrors
def n_blocks(B, cap):
    """mmgan_dcnn.hip:690-703: the fewest workgroups that finish in the same number of sample rounds."""
    rounds = (B + cap - 1) // cap
    return (B + rounds - 1) // rounds


def cap_for(cus):
    return max(cus * 7 // 8, 1)


def assignment(B, nb):
    """sample b -> (workgroup, round): the kernel's loop b = blockIdx.x + k * gridDim.x (mmgan_dcnn.hip:208)."""
    return [(b % nb, b // nb) for b in range(B)]


def workgroup_samples(B, nb):
    return [list(range(w, B, nb)) for w in range(nb)]


def regimes(B, bsplit, cap):
    """What a (B, bsplit) case exercises on `cap` workgroups: rounds, uneven last round, a workgroup holding both labels,
    a workgroup with fewer samples than another."""
    nb = n_blocks(B, cap)
    per = [len(s) for s in workgroup_samples(B, nb)]
    mixed = any(s and s[0] < bsplit <= s[-1] for s in workgroup_samples(B, nb))
    return dict(nb=nb, rounds=max(per), uneven=min(per) != max(per), mixed=mixed)


def dims(T):
    OW1 = T // 2
    OW2 = (OW1 - 2) // 2 + 1
    return dict(OW1=OW1, OW2=OW2, KFC=32 * 32 * OW2)


def slab_width(T):
    """floats per workgroup slab with gradients (mmgan_dcnn.hip:37, 704): S_DWFC + KFC"""
    return 8756 + dims(T)["KFC"]


def where_sample(B, nb, bsplit):
    def f(idx):
        b = idx[0]
        return (f"sample {b} ({'first' if b < bsplit else 'second'} segment), workgroup {b % nb} round {b // nb} "
                f"of {(B + nb - 1) // nb} on {nb} workgroups")
    return f


def _d(t):
    return t.detach().cpu().double()


# ---------------------------------------------------------------------------------------------- fused DCNN
SLOPE = 0.20000000298023224            # the kernel's 0.2f
GRAD_NAMES = ("dw1", "db1", "dw2", "db2", "dwfc", "dbfc")
OUT_NAMES = ("logits", "loss") + GRAD_NAMES
# ||got - ref||_2 / ||M||_2 bounds (see the module docstring): bf16 fused kernel against the same-rounding reference,
# and the exact-fp32 parity path against the unrounded one
RL_BF16 = 5e-5
RL_F32 = 1e-5


def bf16r(v):
    """fp32 -> bf16 round-to-nearest-even (the kernel's (__bf16) conversion), in float64"""
    return v.float().bfloat16().double()


def _leaky(v):
    return torch.where(v > 0, v, SLOPE * v)


def dcnn_ref(x, bsplit, ya, yb, params, *, bf16=True, faults=(), loss_init=0.0):
    """The pass of gdm_dcnn_fused (bf16=True: every rounding of the kernel mirrored) or of functional.dcnn_forward /
    dcnn_backward in fp32 (bf16=False: no rounding) on x (B, 2, 128, T) fp32: samples [0, bsplit) carry label ya,
    the rest yb.  params: (w1, b1, w2, b2, wfc, bfc) fp32.  Returns {name: (ref, M)} for logits (B,), loss (1,) and
    the six gradients in torch layout; M is the same computation on absolute values.
    faults (tests/test_mmgan_ref.py only): ("drop", k) / ("twice", k): sample k enters the gradients 0 / 2 times;
    "swap_label": sample bsplit takes ya; "cnt_B": loss and dl normalised by B; "conv2_shift": conv2 reads its input
    one column to the left; "slope0": conv1's LeakyReLU' uses 0 for 0.2; "no_input_round": the input is not rounded."""
    fl = dict((f, None) if isinstance(f, str) else f for f in faults)
    x = _d(x)
    B, T = x.shape[0], x.shape[3]
    w1, b1, w2, b2, wfc, bfc = (_d(q) for q in params)
    r = bf16r if bf16 else (lambda v: v)
    if bf16 and "no_input_round" not in fl:
        x = bf16r(x)                                                   # x_store (mmgan_dcnn.hip:191)
    w1, w2, wfc = r(w1), r(w2), r(wfc)                                 # the pack (:98); biases stay fp32
    conv = lambda a, w, b_=None: torch.nn.functional.conv2d(a, w, b_, stride=2, padding=1)  # noqa: E731
    z1 = conv(x, w1, b1)
    Mz1 = conv(x.abs(), w1.abs(), b1.abs())
    h1 = r(_leaky(z1))                                                 # :255
    h1_in = torch.nn.functional.pad(h1, (0, 1))[..., 1:] if "conv2_shift" in fl else h1
    z2 = conv(h1_in, w2, b2)
    Mz2 = conv(h1.abs(), w2.abs(), b2.abs())
    h2 = r(_leaky(z2))                                                 # :303
    hf = h2.flatten(1)                                                 # channel-major, as fc's weight
    z = hf @ wfc[0] + bfc[0]
    Mz = hf.abs() @ wfc[0].abs() + bfc.abs()[0]
    first = torch.arange(B) < bsplit
    y = torch.where(first, float(ya), float(yb)).double()
    cnt = torch.where(first, float(max(bsplit, 1)), float(max(B - bsplit, 1))).double()   # :331
    if "swap_label" in fl and bsplit < B:
        y[bsplit] = float(ya)
    if "cnt_B" in fl:
        cnt = torch.full_like(cnt, float(B))
    sig = torch.sigmoid(z)
    dl = (sig - y) / cnt                                               # :332
    lt = torch.nn.functional.softplus(-z.abs()) + z.clamp_min(0) - z * y
    loss = (lt / cnt).sum() + loss_init                                # :335
    Mloss = ((torch.nn.functional.softplus(-z.abs()) + z.clamp_min(0) + (z * y).abs()) / cnt).sum() + abs(loss_init)
    wgt = torch.ones(B, dtype=torch.float64)
    if "drop" in fl:
        wgt[fl["drop"]] = 0.0
    if "twice" in fl:
        wgt[fl["twice"]] = 2.0
    dlg = dl * wgt
    dwfc, Mdwfc = (dlg @ hf)[None], (dlg.abs() @ hf.abs())[None]      # :351
    dbfc, Mdbfc = dlg.sum()[None], dlg.abs().sum()[None]
    W = wfc[0].view(1, 32, 32, -1)
    gy2 = dlg[:, None, None, None] * W * torch.where(h2 > 0, 1.0, SLOPE)     # :352
    db2, Mdb2 = gy2.sum((0, 2, 3)), gy2.abs().sum((0, 2, 3))          # :353 (unrounded)
    g2 = r(gy2)                                                        # :354
    cw = lambda a, shape, g: torch.nn.grad.conv2d_weight(a, shape, g, stride=2, padding=1)  # noqa: E731
    dw2, Mdw2 = cw(h1, w2.shape, g2), cw(h1.abs(), w2.shape, g2.abs())
    ci = lambda w, g: torch.nn.grad.conv2d_input(h1.shape, w, g, stride=2, padding=1)  # noqa: E731
    dh1, Mdh1 = ci(w2, g2), ci(w2.abs(), g2.abs())
    sl1 = torch.where(h1 > 0, 1.0, 0.0 if "slope0" in fl else SLOPE)
    dy1 = dh1 * sl1                                                    # :436
    db1, Mdb1 = dy1.sum((0, 2, 3)), (Mdh1 * sl1).sum((0, 2, 3))       # :437 (unrounded)
    g1 = r(dy1)                                                        # :438
    dw1, Mdw1 = cw(x, w1.shape, g1), cw(x.abs(), w1.shape, g1.abs())
    return dict(logits=(z, Mz), loss=(loss[None], Mloss[None]), dw1=(dw1, Mdw1), db1=(db1, Mdb1), dw2=(dw2, Mdw2),
                db2=(db2, Mdb2), dwfc=(dwfc, Mdwfc), dbfc=(dbfc, Mdbfc))


def rel_to_m(got, ref, M):
    got = got.detach().cpu().double().reshape(ref.shape)
    return float((got - ref).norm() / M.norm().clamp_min(1e-300))


def check_dcnn(got, ref, *, bound, what=""):
    """||got - ref|| / ||M|| <= bound for every output in `got` (name -> tensor).  Returns {name: measured / bound}."""
    res = {}
    for name, g in got.items():
        q = rel_to_m(g, *ref[name])
        if not q <= bound:
            raise CheckError(f"{what} {name}: ||err|| / ||M|| = {q:.3g} > {bound:.3g}")
        res[name] = q / bound
    return res


# ------------------------------------------------------------------------------ Linear + BatchNorm1d + activation
SPLIT_REL = 3.05 * 2.0 ** -16
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 3


def split_parts(v):
    """fp32 v -> (hi, lo) bf16 parts as the kernel stages them (linear_bn.hip:130, 137), in float64."""
    v = v.detach().cpu().float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi.double(), lo.double()


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def linear_bn_ref(x, w, bias, gamma, beta, running_mean, running_var, nbt, *, act, training=True, momentum=0.1,
                  eps=1e-5, groups=1, stat_repeats=1, faults=()):
    """gdm_linear_bn_act_fwd on x (groups * M, K).  Returns dict of (ref, E) pairs -- the bound is absolute --:
    y, out (groups * M, N); save_mean, save_invstd (groups, N); running_mean, running_var (N,); and the integer
    num_batches_tracked.  faults (tests/test_mmgan_ref.py only): "drop_xh_wl", "biased_var", "reverse_groups"."""
    x, w = _d(x), _d(w)
    N, K = w.shape
    M = x.shape[0] // groups
    b = _d(bias) if bias is not None else torch.zeros(N, dtype=torch.float64)
    gm, bt = _d(gamma), _d(beta)
    rm = _d(running_mean) if running_mean is not None else None
    rv = _d(running_var) if running_var is not None else None
    y = x @ w.T + b
    if "drop_xh_wl" in faults:
        xh, _ = split_parts(x)
        _, wl = split_parts(w)
        y = y - xh @ wl.T
    Ey = (SPLIT_REL + (3 * K + 2) * U) * (x.abs() @ w.abs().T) + U * b.abs()
    ig = 0.25 if act == ACT_SIGMOID else 1.0
    outs, Eouts, means, Emeans, invs, Einvs, stats = [], [], [], [], [], [], []
    for g in range(groups):
        yg, Eg = y[g * M:(g + 1) * M], Ey[g * M:(g + 1) * M]
        if training:
            mean = yg.mean(0)
            Emean = Eg.mean(0) + (M + 6) * U * yg.abs().mean(0)
            d = yg - mean
            m2 = (d * d).sum(0)
            Em2 = (2 * d.abs() * (Eg + Emean) + (Eg + Emean) ** 2).sum(0) + (M + 8) * U * m2
            var = m2 / M
            inv = 1.0 / torch.sqrt(var + eps)
            vlo = ((m2 - Em2) / M).clamp_min(0.0)
            Einv = 0.5 * (vlo + eps) ** -1.5 * (Em2 / M) + 4 * U * inv
            stats.append((mean, Emean, m2 / max(M - 1, 1), Em2 / max(M - 1, 1)))
        else:
            mean, Emean = rm, torch.zeros_like(rm)
            inv = 1.0 / torch.sqrt(rv + eps)
            Einv = 4 * U * inv
        d = yg - mean
        pre = d * inv * gm + bt
        Epre = ((Eg + Emean) * inv + (d.abs() + Eg + Emean) * Einv) * gm.abs() + 4 * U * (pre.abs() + bt.abs())
        o = _act(pre, act)
        Eo = ig * Epre + (20 * U * o.abs() if act == ACT_SIGMOID else 0.0)
        outs.append(o)
        Eouts.append(Eo)
        means.append(mean)
        Emeans.append(Emean)
        invs.append(inv)
        Einvs.append(Einv)
    res = dict(y=(y, Ey), out=(torch.cat(outs), torch.cat(Eouts)))
    shape = (N,) if groups == 1 else (groups, N)
    res["save_mean"] = (torch.stack(means).reshape(shape), torch.stack(Emeans).reshape(shape))
    res["save_invstd"] = (torch.stack(invs).reshape(shape), torch.stack(Einvs).reshape(shape))
    n0 = int(nbt) if nbt is not None else 0
    if training and rm is not None:
        Erm, Erv = torch.zeros_like(rm), torch.zeros_like(rv)
        order = list(reversed(stats)) if "reverse_groups" in faults else stats
        for mean, Emean, uvar, Euvar in order:
            if "biased_var" in faults:
                uvar = uvar * (M - 1) / M
            for _ in range(stat_repeats):
                rm = (1 - momentum) * rm + momentum * mean
                rv = (1 - momentum) * rv + momentum * uvar
                Erm = (1 - momentum) * Erm + momentum * Emean + 4 * U * (rm.abs() + mean.abs())
                Erv = (1 - momentum) * Erv + momentum * Euvar + 4 * U * (rv.abs() + uvar.abs())
        res["running_mean"], res["running_var"] = (rm, Erm), (rv, Erv)
        res["num_batches_tracked"] = n0 + groups * stat_repeats
    else:
        if rm is not None:
            res["running_mean"], res["running_var"] = (rm, torch.zeros_like(rm)), (rv, torch.zeros_like(rv))
        res["num_batches_tracked"] = n0
    return res


def check_abs(got, ref, E, *, what="", where=None):
    """|got - ref| <= E per element (check_elementwise with rtol 1 and M = E).  Returns the worst ratio."""
    where = where or (lambda idx: f"{what}{list(idx)}")
    return check_elementwise(got, ref, E, rtol=1.0, out_dtype=torch.float32, where=where, what=what)


def where_lb(M):
    def f(idx):
        r = idx[0]
        rest = f", column {idx[1]}" if len(idx) > 1 else ""
        return f"row {r} (group {r // M}, wave {(r % M) // 64}, tile {((r % M) % 64) // 16}){rest}"
    return f


def check_linear_bn(got, ref, *, M, what=""):
    """got: dict name -> tensor for the outputs present.  Returns {name: worst |err| / bound}."""
    res = {}
    for name, g in got.items():
        r, E = ref[name]
        wh = where_lb(M) if name in ("y", "out") else None
        res[name] = check_abs(g.reshape(r.shape), r, E, what=f"{what} {name}", where=wh)
    return res
