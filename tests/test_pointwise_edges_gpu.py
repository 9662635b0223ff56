"""GPU: the layer-wise pointwise kernels of csrc/pointwise.hip (BatchNorm forward / backward / statistics / partials
and their merge, column sums, bias + activation and its backward, casts, Adam, BCE and the criteria) against the
float64 references of tests/lowering_ref.py at their edges: both sides of every row_chunks boundary, every
lanes-per-row value, bf16 outputs, ill-conditioned channels, grid-stride second trips, misaligned pointers.

Derived bounds (lowering_ref's docstring): BatchNorm apply and backward (from the kernel's own statistics / output),
column sums, bias + activation, Adam (one step from the kernel's own fp32 state), the criteria.  expf and log1pf enter
as lowering_ref.SIGMOID_ULPS of the sigmoid (measured, tests/test_lowering_batch_gpu.py) and 8 u of the log1p term.

Measured bounds: the BatchNorm statistics and partials, in the units of lowering_ref.stats_ratios / partial_ratios
(u max|y| for means, u invstd for invstd, u (|running_var| + var) for running_var, u (M2 + n dev^2) for a chunk's
M2).  Measured maxima on MI355X over BN_PAIRS and MERGE_CASES, written by helpers.record as "bn_stats" /
"bn_partials" / "bn_merge" and kept in lowering_ref.STATS_MEASURED; the bounds are 4 x measured:
    family     mean   invstd  running_mean  running_var  partial mean  partial M2
    standard   1.07    10.99         0.472        2.913         2.889       5.198
    bigmean    2.609  1231.4         0.553        9.404         5.963       814.9
    special    1.07    733.2         0.472        234.2         2.889       5.198
(bigmean: Chan's merges round every partial mean at 1e3, which costs the variance ~1e-4 relative; special: the
outlier channel.)  The derived bounds are nearly attained: worst err / bound 0.996 for the BatchNorm output (a bf16
store at half an ulp), 0.98 for Adam's v, 0.80 for the column sums.
Families: "standard" (N(0.5, 2)), "bigmean" (every channel mean 1e3, spread 1e-1: the case the shifted sums exist
for), "special" (standard, with channel 0 exactly constant -- variance exactly 0, M2 exactly 0, invstd = 1/sqrt(eps),
finite output -- and the last channel carrying one outlier of 1e4 in the first row of its last chunk).

NaN is left out of the cast test: the library is built with -fno-honor-nans.  The 64-bit-index variant
bn_apply<int64_t> needs more than 2^31 elements and stays untested.

gdm_simnn_head: prob against float64 with the dot product's (128 + 1) u sum|h w| through the sigmoid; everything behind
it (loss, dh1, dw2, db2, db1) from the kernel's own prob, each sum with n u sum|terms| on top of its terms' bounds.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402
from gan_des_midi_music_gen_amd.ops import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F32  # noqa: E402

import lowering_ref as R  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
DT = {torch.float32: F32, torch.bfloat16: BF16}
TYPES = (torch.float32, torch.bfloat16)
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))      # what the C ABI receives
FAMILIES = ("standard", "bigmean", "special")
@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


_bounds = R.stats_bounds


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bn_input(rows, C, family, seed=0):
    g = _gen(rows * 131 + C + seed)
    if family == "bigmean":
        return 1e3 + 0.1 * torch.randn(rows, C, generator=g)
    y = torch.randn(rows, C, generator=g) * 2 + 0.5
    if family == "special":
        y[:, 0] = 0.75
        if C >= 2:
            y[(R.row_chunks(rows) - 1) * R.chunk_rows(rows), C - 1] = 1e4
    return y


def _bn_params(C, seed):
    g = _gen(seed)
    return (1 + 0.5 * (2 * torch.rand(C, generator=g) - 1), 0.5 * (2 * torch.rand(C, generator=g) - 1),
            torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5)


ACT_TYPE = [(a, t) for a in (ACT_RELU, ACT_SIGMOID, ACT_NONE) for t in TYPES]


@pytest.mark.parametrize("rows,C", R.BN_PAIRS)
def test_batchnorm_statistics_forward_backward(rows, C):
    fails = []
    gamma, beta, rm0, rv0 = _bn_params(C, rows + C)
    case = R.BN_PAIRS.index((rows, C))
    for fi, family in enumerate(FAMILIES):
        y = bn_input(rows, C, family)
        yd = y.to(DEV)
        sb, pb = _bounds(family)
        what = f"({rows},{C}) {family}"
        # ---- statistics: two training calls on the same input; gdm_bn_stats launches the same two kernels
        act, ot = ACT_TYPE[(case + 2 * fi) % 6]
        rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor(3, device=DEV)
        out, mean, inv = ops.bn_act_fwd(yd, gamma.to(DEV), beta.to(DEV), rm, rv, nbt, act=act, out_dtype=DT[ot])
        rm_s, rv_s, nbt_s = rm0.to(DEV), rv0.to(DEV), torch.tensor(3, device=DEV)
        mean_s, inv_s = ops.bn_stats(yd, rm_s, rv_s, nbt_s)
        for a, b, n in ((mean_s, mean, "mean"), (inv_s, inv, "invstd"), (rm_s, rm, "running_mean"),
                        (rv_s, rv, "running_var")):
            fails += R.check_bits(a, b, what=f"{what} gdm_bn_stats vs gdm_bn_act_fwd {n}")
        ops.bn_act_fwd(yd, gamma.to(DEV), beta.to(DEV), rm, rv, nbt, act=act, out_dtype=DT[ot])
        ref = R.bn_stats_ref(y, rm0, rv0, 3, calls=2, momentum=MOM, eps=EPS)
        f, ratios = R.check_stats(dict(mean=mean, invstd=inv, running_mean=rm, running_var=rv,
                                       num_batches_tracked=int(nbt.item())), ref, sb, what=what)
        record("bn_stats", case=what, **{k: round(v, 3) for k, v in ratios.items()})
        fails += f
        # ---- the Welford partials, chunk by chunk
        part = ops.bn_partials(yd)
        f, pr = R.check_partials(part, R.partials_ref(y), pb, what=what)
        record("bn_partials", case=what, mean=round(pr["mean"], 3), m2=round(pr["m2"], 3))
        fails += f
        if family == "special":
            c = float(y[0, 0])
            assert float(part[:, 0, 2].abs().max()) == 0.0 and bool((part[:, 0, 1] == c).all()), "constant channel"
            assert float(mean[0]) == c
            inv0 = 1.0 / math.sqrt(EPS)
            assert abs(float(inv[0]) - inv0) <= 4 * 2.0 ** -23 * inv0, "variance of a constant channel must be exactly 0"
            assert bool(torch.isfinite(out.float()).all())
        if rows * C > 1 << 20 and fi != case % 3:        # the large cases: apply / backward on one family each
            continue
        # ---- apply and backward from the kernel's own statistics / output
        o_ref, E = R.bn_apply_ref(y, gamma, beta, mean, inv, act, ot)
        f, w_out = R.check_bound(out, o_ref, E, what=f"{what} out act {act} {ot}")
        fails += f
        d = torch.randn(rows, C, generator=_gen(rows + fi)).to(ot)
        dy, dgamma, dbeta = ops.bn_act_bwd(d.to(DEV), out, yd, gamma.to(DEV), mean, inv, act=act)
        bw = R.bn_bwd_ref(d, out, y, gamma, mean, inv, act)
        worst = {"out": w_out}
        for name, got in (("dy", dy), ("dgamma", dgamma), ("dbeta", dbeta)):
            f, worst[name] = R.check_bound(got, bw[name][0], bw[name][1], what=f"{what} {name} act {act} {ot}")
            fails += f
        record("bn_fwd_bwd", case=what, act=act, dtype=str(ot), **{k: round(v, 4) for k, v in worst.items()})
    # ---- eval mode: the running statistics are used and left alone
    y = bn_input(rows, C, "standard", seed=1)
    act, ot = ACT_TYPE[(case + 1) % 6]
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor(3, device=DEV)
    out, mean, inv = ops.bn_act_fwd(y.to(DEV), gamma.to(DEV), beta.to(DEV), rm, rv, nbt, act=act, out_dtype=DT[ot],
                                    training=False)
    fails += R.check_bits(rm, rm0, what="eval running_mean") + R.check_bits(rv, rv0, what="eval running_var")
    fails += R.check_bits(mean, rm0, what="eval save_mean")
    assert int(nbt.item()) == 3
    inv_ref = 1.0 / torch.sqrt(rv0.double() + EPS)
    fails += R.check_bound(inv, inv_ref, 4 * R.U * inv_ref, what="eval invstd")[0]
    o_ref, E = R.bn_apply_ref(y, gamma, beta, mean, inv, act, ot)
    fails += R.check_bound(out, o_ref, E, what=f"({rows},{C}) eval out act {act} {ot}")[0]
    assert not fails, fails


@pytest.mark.parametrize("shards,C", R.MERGE_CASES, ids=str)
@pytest.mark.parametrize("family", ["standard", "bigmean"])
def test_rank_merge_of_partials_in_one_process(shards, C, family):
    rows = sum(shards)
    y = bn_input(rows, C, family)
    gamma, beta, rm0, rv0 = _bn_params(C, rows)
    parts, r0 = [], 0
    for r in shards:
        parts.append(ops.bn_partials(y[r0:r0 + r].contiguous().to(DEV)))
        r0 += r
    part = torch.cat(parts).contiguous()
    assert part.shape[0] == sum(R.row_chunks(r) for r in shards)
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor(0, device=DEV)
    mean, inv = ops.bn_finalize(part, part.shape[0], rows, C, rm, rv, nbt)
    ref = R.bn_stats_ref(y, rm0, rv0, 0, momentum=MOM, eps=EPS)
    fails, ratios = R.check_stats(dict(mean=mean, invstd=inv, running_mean=rm, running_var=rv,
                                       num_batches_tracked=int(nbt.item())), ref, _bounds(family)[0],
                                  what=f"{shards} {family}")
    record("bn_merge", case=f"{shards} {family}", **{k: round(v, 3) for k, v in ratios.items()})
    for act, ot in ((ACT_RELU, torch.bfloat16), (ACT_NONE, torch.float32)):
        out = ops.bn_apply(y.to(DEV), gamma.to(DEV), beta.to(DEV), mean, inv, act=act, out_dtype=DT[ot])
        o_ref, E = R.bn_apply_ref(y, gamma, beta, mean, inv, act, ot)
        fails += R.check_bound(out, o_ref, E, what=f"{shards} {family} bn_apply act {act}")[0]
    assert not fails, fails


def test_colsum():
    fails, worst = [], 0.0
    for rows in R.COLSUM_ROWS:
        for cols in R.COLSUM_COLS:
            x32 = torch.randn(rows, cols, generator=_gen(rows + cols)) + 0.25
            for t in TYPES:
                x = x32.to(t)
                ref, E = R.colsum_ref(x)
                got = ops.colsum(x.to(DEV))
                if rows == 1:
                    fails += R.check_bits(got, x.float().reshape(-1), what=f"colsum (1,{cols}) {t}")
                f, w = R.check_bound(got, ref, E, what=f"colsum ({rows},{cols}) {t}")
                fails += f
                worst = max(worst, w)
    record("colsum", worst=round(worst, 4))
    assert not fails, fails


@pytest.mark.parametrize("rows,cols", R.BIAS_ACT_SHAPES)
def test_bias_act_forward_and_backward(rows, cols):
    fails = []
    x = torch.randn(rows, cols, generator=_gen(rows)) * 3
    bias = torch.randn(cols, generator=_gen(cols))
    slope = 0.2
    sl = float(np.float32(slope))
    for act in (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID):
        for t in TYPES:
            for b in (bias, None):
                pre = x.double() + (b.double() if b is not None else 0.0)
                E_pre = R.U * pre.abs() if b is not None else torch.zeros_like(pre)
                ref = R.act_ref(pre, act, sl)
                E = R.store_bound(ref, R.act_bound(pre, E_pre, act, sl), t)
                out = ops.bias_act_fwd(x.to(DEV), None if b is None else b.to(DEV), act=act, slope=slope,
                                       out_dtype=DT[t])
                fails += R.check_bound(out, ref, E, what=f"bias_act ({rows},{cols}) act {act} {t} bias {b is not None}")[0]
            d = torch.randn(rows, cols, generator=_gen(act + 5)).to(t)
            dx = ops.act_bwd(d.to(DEV), out, act=act, slope=slope)
            assert dx.dtype == t
            g = d.double() * R.act_grad_from_out(out.cpu().double(), act, sl)
            fails += R.check_bound(dx, g, R.store_bound(g, 3 * R.U * g.abs(), t),
                                   what=f"act_bwd ({rows},{cols}) act {act} {t}")[0]
    assert not fails, fails


def test_cast_round_trips_and_rounds_to_nearest_even():
    """NaN patterns are left out: the library is built with -fno-honor-nans."""
    pat = torch.arange(65536, dtype=torch.int32)
    keep = ~(((pat & 0x7F80) == 0x7F80) & ((pat & 0x7F) != 0))
    b = pat[keep].to(torch.int16).view(torch.bfloat16)
    assert b.numel() == 65536 - 2 * 127
    up = ops.cast(b.to(DEV), F32)
    fails = R.check_bits(up, b.float(), what="bf16 -> fp32")
    fails += R.check_bits(ops.cast(up, BF16), b, what="bf16 -> fp32 -> bf16")
    words = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,          # exact ties, even and odd kept bit
             0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,          # one fp32 ulp either side of a tie
             0x3FFFFFFF, 0x3FFF8000, 0xBFFFFFFF, 0x007FFFFF,          # round up into the next binade
             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,          # the largest finite values (to Inf, or not)
             0x00000001, 0x00008000, 0x00018000, 0x0000FFFF, 0x80000001, 0x80018000, 0x00400000,   # subnormals
             0x00000000, 0x80000000, 0x7F800000, 0xFF800000]          # +-0, +-Inf
    f = torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())
    f = torch.cat([f, torch.randn(5000, generator=_gen(1)) * 1e3])
    fails += R.check_bits(ops.cast(f.to(DEV), BF16), f.bfloat16(), what="fp32 -> bf16")
    fails += R.check_bits(ops.cast(f.to(DEV), F32), f, what="fp32 -> fp32")
    assert not fails, fails


def _adam_run(n, gs, betas, lr, offset):
    """five steps; every step of gdm_adam_step is checked against ONE float64 step from the kernel's own previous
    state, and gdm_adam_step_dev (its own trajectory) must equal it bit for bit.  Returns (failures, worst, state)."""
    b1, b2 = (float(np.float32(b)) for b in betas)
    lr32, eps32 = float(np.float32(lr)), float(np.float32(1e-8))
    g = _gen(n % 100000 + int(gs * 8))

    def buf(src=None):
        t = torch.zeros(n + offset, device=DEV)[offset:]
        if src is not None:
            t.copy_(src)
        assert t.data_ptr() % 16 == (4 * offset) % 16
        return t

    p0 = torch.randn(n, generator=g)
    p, m, v = buf(p0), buf(), buf()
    pd, md, vd = buf(p0), buf(), buf()
    hyper = ops.adam_hyper(torch.device(DEV), lr, betas[0], betas[1], 1e-8, gs)
    fails, worst = [], {}
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * 10.0 ** -step
        gd = buf(grad)
        before = [t.cpu() for t in (p, m, v)]
        ops.adam_step(p, gd, m, v, step, lr, betas[0], betas[1], 1e-8, gs)
        ops.adam_step_dev(pd, gd, md, vd, hyper)
        ref = R.adam_ref(before[0], grad, before[1], before[2], step, lr32, b1, b2, eps32, gs)
        f, w = R.check_adam(dict(p=p, m=m, v=v), ref, what=f"adam n={n} gs={gs} betas={betas} step {step}")
        fails += f
        worst = {k: max(worst.get(k, 0.0), x) for k, x in w.items()}
        for a, b, name in ((pd, p, "p"), (md, m, "m"), (vd, v, "v")):
            fails += R.check_bits(a, b, what=f"adam_step_dev vs adam_step {name} n={n} step {step}")
    return fails, worst, (p.cpu(), m.cpu(), v.cpu())


@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_steps_against_float64(n):
    big = n > 1 << 20
    combos = [(0.125, (0.5, 0.999), 2e-5)] if big else [(gs, betas, lr) for gs in (1.0, 0.125)
                                                        for betas, lr in (((0.5, 0.999), 2e-5), ((0.9, 0.99), 1e-2))]
    fails = []
    for gs, betas, lr in combos:
        f, worst, state = _adam_run(n, gs, betas, lr, 0)
        fails += f
        record("adam", n=n, gs=gs, betas=list(betas), **{k: round(x, 4) for k, x in worst.items()})
        if not big:                      # the scalar variant: views one float into their buffers
            f, _, state_u = _adam_run(n, gs, betas, lr, 1)
            fails += f
            for a, b, name in zip(state_u, state, "pmv"):
                fails += R.check_bits(a, b, what=f"misaligned vs aligned {name} n={n}")
    assert not fails, fails


def _logits(n, seed):
    x = torch.randn(n, generator=_gen(seed)) * 3
    edge = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0])
    x[:min(n, 5)] = edge[:min(n, 5)]
    return x


def _loss_bound(terms_abs, log_terms, n, loss):
    """fixed-order sum of n terms (any order: n - 1 roundings), <= 4 roundings inside a term, log1pf(expf()) within
    8 u of its value, the division by n and the accumulate add"""
    return ((n + 3) * R.U * float(terms_abs.sum()) + 8 * R.U * float(log_terms.sum())) / n + 2 * R.U * abs(loss) \
        + R.F32_TINY


@pytest.mark.parametrize("n", R.LOSS_N)
def test_bce_and_criteria_against_float64(n):
    fails = []
    for target, gs in ((0.9, 1.0), (0.0, 0.5), (1.0, 1.0)):
        y = float(np.float32(target))
        for fuse in (False, True):
            x = torch.sigmoid(_logits(n, n)) if fuse else _logits(n, n + 1)
            xd = x.double()
            log_t = torch.log1p(torch.exp(-xd.abs()))
            t_abs = torch.clamp(xd, min=0) + (xd * y).abs() + log_t
            loss_ref = float(R.bce_terms(x, y).mean())
            o = torch.sigmoid(xd)
            chain = xd * (1 - xd) if fuse else torch.ones_like(xd)
            dx_ref = (o - y) * gs / n * chain
            E_dx = (R.SIGMOID_ULPS * 2.0 ** -23 * o + 8 * R.U * (o - y).abs()) * gs / n * chain.abs() + 2.0 ** -149
            for acc in (False, True):
                for want in (True, False):
                    lo = torch.full((1,), 1.5, device=DEV)
                    _, dx = ops.bce_with_logits(x.to(DEV), target, grad_scale=gs, want_grad=want,
                                                fuse_sigmoid_backward=fuse, loss_out=lo, accumulate_loss=acc)
                    want_loss = loss_ref + (1.5 if acc else 0.0)
                    E = _loss_bound(t_abs, log_t, n, want_loss)
                    if not abs(lo.item() - want_loss) <= E:
                        fails.append(f"bce n={n} y={y} fuse={fuse} acc={acc}: loss {lo.item()!r} vs {want_loss!r} "
                                     f"(bound {E:.3g})")
                    assert (dx is None) == (not want)
                    if want:
                        fails += R.check_bound(dx, dx_ref, E_dx, what=f"bce dx n={n} y={y} fuse={fuse}")[0]
            if not fuse:                     # the criterion entry point: BCE bit-identical, MSE and L1 against float64
                la, lb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
                _, da = ops.bce_with_logits(x.to(DEV), target, grad_scale=gs, loss_out=la)
                _, db = ops.criterion_loss(x.to(DEV), target, "bce", loss_out=lb, grad_scale=gs)
                fails += R.check_bits(lb, la, what="criterion bce loss") + R.check_bits(db, da, what="criterion bce dx")
                r = xd - y
                for crit, terms, dref in (("mse", r * r, 2 * r * gs / n), ("l1", r.abs(), torch.sign(r) * gs / n)):
                    for acc in (False, True):
                        lo = torch.full((1,), 1.5, device=DEV)
                        _, dx = ops.criterion_loss(x.to(DEV), target, crit, loss_out=lo, accumulate_loss=acc,
                                                   grad_scale=gs)
                        want_loss = float(terms.mean()) + (1.5 if acc else 0.0)
                        E = _loss_bound(terms, torch.zeros(1), n, want_loss)
                        if not abs(lo.item() - want_loss) <= E:
                            fails.append(f"{crit} n={n} y={y} acc={acc}: loss {lo.item()!r} vs {want_loss!r}")
                        fails += R.check_bound(dx, dref, 4 * R.U * dref.abs() + 2.0 ** -149, what=f"{crit} dx n={n}")[0]
                    _, none = ops.criterion_loss(x.to(DEV), target, crit, loss_out=lo, want_grad=False)
                    assert none is None
    assert not fails, fails


@pytest.mark.parametrize("n,n0", R.HEAD_N)
@pytest.mark.parametrize("dh", TYPES, ids=str)
def test_simnn_head_against_float64(n, n0, dh):
    assert n0 % 8 or n == 1
    g = _gen(n)
    h1 = torch.relu(torch.randn(n, 128, generator=g))
    w2, b2 = torch.randn(1, 128, generator=g) * 0.2, torch.randn(1, generator=g)
    y0, y1 = float(np.float32(0.9)), float(np.float32(0.1))
    lo = torch.full((1,), 1.5, device=DEV)
    prob, dh1, (dw2, db2, db1) = ops.simnn_head(h1.to(DEV), w2.to(DEV), b2.to(DEV), n0, 0.9, 0.1, loss_out=lo,
                                                accumulate_loss=True, dh_dtype=DT[dh])
    hd, wd = h1.double(), w2.double().reshape(-1)
    z = hd @ wd + b2.double()
    E_z = 129 * R.U * (hd.abs() @ wd.abs() + b2.double().abs())
    fails = R.check_bound(prob, R.act_ref(z, ACT_SIGMOID), R.act_bound(z, E_z, ACT_SIGMOID), what=f"head prob n={n}")[0]
    p = prob.cpu().double()                                   # everything below: from the kernel's own prob
    first = torch.arange(n) < n0
    y = torch.where(first, torch.tensor(y0, dtype=torch.float64), torch.tensor(y1, dtype=torch.float64))
    cnt = torch.where(first, float(n0), float(max(n - n0, 1)))
    log_t = torch.log1p(torch.exp(-p.abs()))
    lt_abs = (p + (p * y).abs() + log_t) / cnt
    loss_ref = float(((p - p * y + log_t) / cnt).sum()) + 1.5
    E_loss = (n + 12) * R.U * float(lt_abs.sum()) + 4 * R.U * abs(loss_ref)
    if not abs(lo.item() - loss_ref) <= E_loss:
        fails.append(f"head loss n={n}: {lo.item()!r} vs {loss_ref!r} (bound {E_loss:.3g})")
    sp = torch.sigmoid(p)
    chain = p * (1 - p) / cnt
    dz = (sp - y) * chain
    E_dz = (R.SIGMOID_ULPS * 2.0 ** -23 * sp + 8 * R.U * (sp - y).abs()) * chain + 2.0 ** -149
    live = hd > 0
    dh_ref = torch.where(live, dz[:, None] * wd[None, :], torch.zeros_like(hd))
    E_dh = torch.where(live, E_dz[:, None] * wd.abs()[None, :] + R.U * dh_ref.abs(), torch.zeros_like(hd))
    fails += R.check_bound(dh1, dh_ref, R.store_bound(dh_ref, E_dh, dh), what=f"head dh1 n={n} {dh}")[0]
    dzh = dz[:, None] * hd
    fails += R.check_bound(dw2.reshape(-1), dzh.sum(0), (E_dz[:, None] * hd).sum(0) + (n + 1) * R.U * dzh.abs().sum(0),
                           what=f"head dw2 n={n}")[0]
    fails += R.check_bound(db2, dz.sum().reshape(1), (E_dz.sum() + n * R.U * dz.abs().sum()).reshape(1),
                           what=f"head db2 n={n}")[0]
    fails += R.check_bound(db1, dh_ref.sum(0), E_dh.sum(0) + n * R.U * dh_ref.abs().sum(0), what=f"head db1 n={n}")[0]
    lo2 = torch.full((1,), 7.0, device=DEV)
    prob2, none, grads = ops.simnn_head(h1.to(DEV), w2.to(DEV), b2.to(DEV), n0, 0.9, 0.1, loss_out=lo2, want_grad=False)
    assert none is None and grads is None
    fails += R.check_bits(prob2, prob, what="prob without gradients")
    if not abs(lo2.item() - (loss_ref - 1.5)) <= E_loss:
        fails.append(f"head loss without gradients n={n}: {lo2.item()!r} vs {loss_ref - 1.5!r}")
    assert not fails, fails
