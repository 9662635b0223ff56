"""Call recorder, per-call float64 checks, float64 mirrors and case tables for the autograd composites of
gan_des_midi_music_gen_amd/functional.py that sit behind the public nn.Module classes:

  simnn_gen        simnn_gen_forward(need_backward=True) / simnn_gen_backward     SIMNN.Generator
  mlp_bn_sigmoid   mlp_bn_sigmoid_forward(need_backward=True) / _backward         network_tests.Generator, BeatGenerator
  mlp_leaky        mlp_leaky_forward / mlp_leaky_backward                         network_tests.Discriminator
  simnn_net        simnn_net_forward / simnn_net_backward                         SIMNN.SimNN

A plain module next to lowering_ref.py and gemm_ref.py: tests/test_autograd_ref.py (CPU) proves the mirrors against
torch autograd in float64, that every planted fault is rejected and that the tables reach the regimes they name;
tests/test_autograd_modules_gpu.py (GPU) holds the modules to it.

Recorder.  recording(ops) replaces the entry points in RECORDED on the ops module (the composites call ops.<name>
through the module attribute) with wrappers that call the original and log every tensor argument (shape, strides,
dtype, address, a copy of the values), the keyword arguments and copies of the results.

Per-call check (check_call).  Every logged call is held to the bound the project already derives for that kernel, on
the call's own recorded operands -- transposed views, K = B * 256, bf16-stored inputs:
  gemm               gemm_ref's continuous bound (K + split_k + 2) 2^-23 Mag + activation + store; split_k from
                     ops.gemm_plan_raw on the recorded description; bf16 compute sees the operands rounded to bf16
  col2im             lowering_ref.check_col2im
  im2col, permute_pc, maxpool2_fwd / _bwd     bit equality
  bn_act_fwd         lowering_ref.check_stats with stats_bounds("standard"), bn_apply_ref from the kernel's statistics
  bn_act_bwd, colsum, act_bwd                 lowering_ref.bn_bwd_ref, colsum_ref, the 3 u |g| of test_pointwise_edges
  linear_bn_act_fwd  mmgan_ref.linear_bn_ref / check_linear_bn
No tolerance is introduced here and no element is left out.

Mirrors.  gen_mirror, mlp_bn_mirror, mlp_leaky_mirror, net_mirror: explicit forward and backward formulas (no
autograd) in the arithmetic type of `dtype` (float64, or float32 for the baseline), with the roundings of bf16 mode
when bf16=True: both operands of every bf16-compute gemm rounded to bf16 (to nearest even), a result rounded where
the composite passes out_dtype=dt, and model 2's fused block as xh wh + xh wl + xl wh (csrc/linear_bn.hip).  Backward
takes the ReLU / leaky-ReLU / pooling selections from `sel` when given (the device's recorded out / idx), else from
its own forward.  faults= plants the wiring mistakes of FAULTS.

End-to-end check.  Per output, gradient and running statistic: max|got - ref| / max|ref| over every element, ref the
float64 mirror with the mode's roundings (on the GPU: with the device's selections).  The bound is measured on the
reference alone: MARGIN (lowering_ref's 4) times the largest ratio the same mirror evaluated in float32 on the CPU
makes against the float64 mirror over the cases of its family (composite, mode, kind), kind in weight / bias /
input / output.  family_bounds() computes the bounds when a test needs them, once per process and on one thread;
nothing reads the table below, which only shows their size.  A Linear bias in front of train-mode BatchNorm has an
exactly zero gradient: it is compared absolutely, against the scale of that layer's weight gradient.  Model 2's
generators at two rows, where BatchNorm's backward is a cancellation to ~1e-5, are a family whose gradients are
compared absolutely too, against the same backward pass on absolute values (family_of says why and how).
tests/test_autograd_ref.py asserts that every fp32 bound is below 2^-10 (half a bf16 ulp is 2^-9: a stray bf16
rounding cannot pass) and that every planted fault exceeds the bound on every case in both modes, but for the
(fault, case) pairs of BF16_BELOW_BASELINE: bf16-mode pairs where the float32 baseline itself holds an error of the
fault's size (a value crossing a bf16 rounding boundary), each held below LISTED_BELOW times the bound instead.

In bf16 mode model 2's weight gradients are held end to end only to 16% of their scale (0.16 below: the family's
maximum, from BeatGenerator's first layer, where one crossed dy meets beat times up to 27); a dropped row or an
unbiased variance is of that size from 256 rows on.  The per-call checks carry those gradients.

Bounds, and beside them in brackets the maxima measured on MI355X over tests/test_autograd_modules_gpu.py
(helpers.record "autograd_e2e"); last column: the largest measured ratio / bound of any tensor of the family:
  family                   mode  weight             bias               input              output
  simnn_gen                fp32  1.4e-05 (8.2e-07)  3.1e-06 (7.2e-07)  2.2e-06 (1.1e-06)  9.7e-07 (3.2e-07)  0.48
  simnn_gen                bf16  0.0086 (0.0025)    0.0032 (0.00052)   0.0076 (0.0015)    0.0034 (0.00051)   0.29
  mlp_bn_sigmoid           fp32  0.00013 (1.3e-05)  1.9e-05 (5.2e-06)  7.7e-06 (1.7e-06)  8.5e-06 (2e-06)    0.27
  mlp_bn_sigmoid           bf16  0.16 (0.038)       0.033 (0.0082)     0.018 (0.0041)     0.024 (0.006)      0.29
  mlp_bn_sigmoid[rows=2]   fp32  4.7e-06 (1.2e-06)  1.4e-05 (5.4e-06)  2.4e-07 (2.3e-13)  8.2e-06 (5.7e-06)  0.47
  mlp_bn_sigmoid[rows=2]   bf16  2.1e-05 (5.3e-06)  2.9e-05 (3.2e-06)  2.4e-07 (5.2e-15)  2e-05 (4.9e-06)    0.50
  mlp_leaky                fp32  3.1e-06 (8.2e-07)  1.5e-06 (4.1e-07)  8.2e-07 (2.1e-07)  2.9e-06 (3.5e-07)  0.27
  mlp_leaky                bf16  4.8e-07 (1.2e-07)  7.1e-07 (1.8e-07)  2.8e-07 (5.4e-08)  3.3e-07 (8.2e-08)  0.25
  simnn_net                fp32  2.6e-06 (7.3e-07)  2.8e-06 (5.3e-07)  1.4e-06 (3.3e-07)  1.4e-06 (5.4e-07)  0.24
  simnn_net                bf16  0.0078 (0.00058)   0.00059 (0.00015)  0.0014 (0.00022)   0.0016 (9.8e-05)   0.25
The bf16 bounds are what one value crossing a bf16 rounding boundary costs at these reduction lengths: 2^-8 of one
product of a sum over K = rows terms.  Per-call checks, worst err / bound over all 62 cases (helpers.record
"autograd_calls", fp32 / bf16 mode): gemm 0.22 / 0.99 (bf16: the half ulp of a bf16 result), col2im 1.0 / 1.0,
bn_act_fwd 0.995 / 0.95, bn_act_bwd 0.53 / 0.49, act_bwd 0.78 / 0.79, colsum 0.995 / 0.997 (two rows: one add
against (rows - 1) u sum|x|), linear_bn_act_fwd - / 0.31; im2col, permute_pc and maxpool2 are bit-equal.
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

import gemm_ref as G
import lowering_ref as L
import mmgan_ref as M

F32, BF16 = 0, 1
MARGIN = L.MARGIN
EPS, MOM = 1e-5, 0.1
SLOPE = 0.20000000298023224          # float(slope) as the C ABI receives it: 0.2f
RECORDED = ("gemm", "im2col", "col2im", "permute_pc", "bn_act_fwd", "bn_act_bwd", "act_bwd", "colsum",
            "linear_bn_act_fwd", "maxpool2_fwd", "maxpool2_bwd")
_GDT = {torch.float32: F32, torch.bfloat16: BF16}
_TDT = {F32: torch.float32, BF16: torch.bfloat16}
G_GEOM = ((1, 0), (2, 1), (2, 1), (1, 0))      # (stride, padding) of the generator's four transposed convolutions


# ====================================================================================================== recorder
class Rec:
    """one tensor as a call saw it"""
    __slots__ = ("shape", "strides", "dtype", "ptr", "value")

    def __init__(self, t):
        self.shape, self.strides, self.dtype, self.ptr = tuple(t.shape), tuple(t.stride()), t.dtype, t.data_ptr()
        self.value = t.detach().to("cpu", copy=True).contiguous()       # the logical values


def _rec(v):
    if isinstance(v, torch.Tensor):
        return Rec(v)
    if isinstance(v, (tuple, list)):
        return tuple(_rec(x) for x in v)
    return v


@contextlib.contextmanager
def recording(ops):
    """log = list of dict(name, args, kwargs, results, after): args / kwargs before the call, results after it, and
    `after` = the tensor arguments once more after the call (the running statistics are updated in place)"""
    log, saved = [], {n: getattr(ops, n) for n in RECORDED}

    def wrap(name, fn):
        def inner(*args, **kwargs):
            entry = dict(name=name, args=_rec(args), kwargs={k: _rec(v) for k, v in kwargs.items()})
            res = fn(*args, **kwargs)
            entry["results"] = _rec(res if isinstance(res, (tuple, list)) else (res,))
            entry["after"] = _rec(args) if name in ("bn_act_fwd", "linear_bn_act_fwd") else None
            log.append(entry)
            return res
        return inner
    for n, fn in saved.items():
        setattr(ops, n, wrap(n, fn))
    try:
        yield log
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)


# ============================================================================================== per-call checks
def gemm_plan_of_call(call, ops):
    a, b = call["args"][:2]
    kw = call["kwargs"]
    m, k = a.shape
    n = b.shape[1]
    comp = kw.get("compute", F32)
    split = kw.get("split_k")
    split = ops.default_split_k(m, n, k, comp) if split is None else split
    out = kw.get("out")
    if out is None:
        tc = kw.get("out_dtype")
        c = (1 << 12, F32 if tc is None else tc, n, 1)
    else:
        c = (out.ptr, _GDT[out.dtype], out.strides[0], out.strides[1])
    bias = kw.get("bias_n")
    return ops.gemm_plan_raw(a.ptr, _GDT[a.dtype], a.strides[0], a.strides[1], b.ptr, _GDT[b.dtype], b.strides[0],
                             b.strides[1], *c, m, n, k, bias.ptr if bias is not None else None, comp, split)


def _check_gemm(call, ops):
    a, b = call["args"][:2]
    kw = call["kwargs"]
    comp = kw.get("compute", F32)
    plan = gemm_plan_of_call(call, ops)

    def seen(t):
        v = t.value.float()
        return (v.bfloat16().float() if comp == BF16 else v).double()
    A, Bm = seen(a), seen(b)
    pre, mag = A @ Bm, A.abs() @ Bm.abs()
    if kw.get("bias_n") is not None:
        bn = kw["bias_n"].value.double()
        pre, mag = pre + bn, mag + bn.abs()
    if kw.get("bias_m") is not None:
        bm = kw["bias_m"].value.double()[:, None]
        pre, mag = pre + bm, mag + bm.abs()
    act = kw.get("act", L.ACT_NONE)
    slope = float(torch.tensor(kw.get("slope", 0.0), dtype=torch.float32))
    e_pre = (a.shape[1] + plan["split_k"] + 2) * 2.0 ** -23 * mag
    ref = L.act_ref(pre, act, slope)
    got = call["results"][0]
    E = L.store_bound(ref, L.act_bound(pre, e_pre, act, slope), got.dtype)
    return L.check_bound(got.value, ref, E, what=f"gemm {a.shape}x{b.shape} {plan['kernel']} split {plan['split_k']}")


def _bits(got, want, what):
    return L.check_bits(got.value.reshape(want.shape), want, what=what), None


def check_call(call, ops):
    """-> (failures, worst err / bound, or None for a bit-equality check) of one logged call"""
    name, a, kw, res = call["name"], call["args"], call["kwargs"], call["results"]
    if name == "gemm":
        return _check_gemm(call, ops)
    if name == "im2col":
        g = dict(B=kw["b"], H=kw["h"], W=kw["w"], C=kw["c"], KH=kw["kh"], KW=kw["kw"], stride=kw["stride"],
                 pad=kw["pad"])
        oh, ow = L.out_size(g["H"], g["KH"], g["stride"], g["pad"]), L.out_size(g["W"], g["KW"], g["stride"], g["pad"])
        fails = [] if (res[1], res[2]) == (oh, ow) else [f"im2col grid {(res[1], res[2])} != {(oh, ow)}"]
        want = L.rnd(L.im2col_ref(a[0].value, planar=kw["planar"], OH=oh, OW=ow, **g), _TDT[kw["out_dtype"]])
        return fails + _bits(res[0], want, f"im2col {g}")[0], None
    if name == "col2im":
        ref = L.col2im_ref(a[0].value, B=kw["b"], H=kw["h"], W=kw["w"], C=kw["c"], KH=kw["kh"], KW=kw["kw"],
                           stride=kw["stride"], pad=kw["pad"], OH=kw["oh"], OW=kw["ow"],
                           tap_major=kw.get("tap_major", False), planar=kw.get("planar", False),
                           act=kw.get("act", L.ACT_NONE))
        return L.check_col2im(res[0].value, ref, _TDT[kw["out_dtype"]], what=f"col2im {kw}")
    if name == "permute_pc":
        b, p, c = a[1:4]
        return _bits(res[0], L.permute_ref(a[0].value, b, p, c, res[0].dtype), f"permute_pc {(b, p, c)}")
    if name == "maxpool2_fwd":
        b, h, w, c = a[1:5]
        m, pos = L.maxpool2_ref(a[0].value, b, h, w, c)
        fails = _bits(res[0], L.rnd(m, a[0].dtype), f"maxpool2_fwd {(b, h, w, c)}")[0]
        return fails + _bits(res[1], pos, f"maxpool2_fwd idx {(b, h, w, c)}")[0], None
    if name == "maxpool2_bwd":
        b, h, w, c = a[2:6]
        want = L.rnd(L.maxpool2_bwd_ref(a[0].value, a[1].value, b, h, w, c), a[0].dtype)
        return _bits(res[0], want, f"maxpool2_bwd {(b, h, w, c)}")
    if name == "bn_act_fwd":
        y, gamma, beta, rm, rv, nbt = a[:6]
        assert kw.get("training", True), "the composites under test run in train mode"
        act, ot = kw["act"], _TDT[kw.get("out_dtype", F32)]
        ref = L.bn_stats_ref(y.value, rm.value, rv.value, int(nbt.value), momentum=kw.get("momentum", MOM),
                             eps=kw.get("eps", EPS))
        post = call["after"]
        got = dict(mean=res[1].value, invstd=res[2].value, running_mean=post[3].value, running_var=post[4].value,
                   num_batches_tracked=int(post[5].value))
        what = f"bn_act_fwd {y.shape}"
        fails, ratios = L.check_stats(got, ref, L.stats_bounds("standard")[0], what=what)
        worst = max(ratios[k] / L.stats_bounds("standard")[0][k] for k in ratios)
        o_ref, E = L.bn_apply_ref(y.value, gamma.value, beta.value, res[1].value, res[2].value, act, ot)
        f, w = L.check_bound(res[0].value, o_ref, E, what=what + " out")
        return fails + f, max(worst, w)
    if name == "bn_act_bwd":
        ref = L.bn_bwd_ref(*[t.value for t in a[:6]], kw["act"])
        fails, worst = [], 0.0
        for key, got in zip(("dy", "dgamma", "dbeta"), res):
            f, w = L.check_bound(got.value, ref[key][0], ref[key][1], what=f"bn_act_bwd {a[2].shape} {key}")
            fails, worst = fails + f, max(worst, w)
        return fails, worst
    if name == "colsum":
        ref, E = L.colsum_ref(a[0].value)
        return L.check_bound(res[0].value, ref, E, what=f"colsum {a[0].shape}")
    if name == "act_bwd":
        slope = float(torch.tensor(kw.get("slope", 0.0), dtype=torch.float32))
        g = a[0].value.double() * L.act_grad_from_out(a[1].value.double(), kw["act"], slope)
        return L.check_bound(res[0].value, g, L.store_bound(g, 3 * L.U * g.abs(), a[0].dtype),
                             what=f"act_bwd {a[0].shape} act {kw['act']}")
    if name == "linear_bn_act_fwd":
        x, w, bias, gamma, beta, rm, rv, nbt = a[:8]
        ref = M.linear_bn_ref(x.value, w.value, bias.value, gamma.value, beta.value, rm.value, rv.value,
                              int(nbt.value), act=kw["act"], training=kw.get("training", True),
                              groups=kw.get("groups", 1), stat_repeats=kw.get("stat_repeats", 1))
        post = call["after"]
        got = dict(out=res[0].value, save_mean=res[2].value, save_invstd=res[3].value, running_mean=post[5].value,
                   running_var=post[6].value)
        if res[1] is not None:
            got["y"] = res[1].value
        what = f"linear_bn_act_fwd {x.shape}x{w.shape}"
        try:
            worst = M.check_linear_bn(got, ref, M=x.shape[0] // kw.get("groups", 1), what=what)
        except M.CheckError as e:
            return [str(e)], float("inf")
        fails = [] if int(post[7].value) == ref["num_batches_tracked"] else [f"{what}: num_batches_tracked"]
        return fails, max(worst.values())
    raise KeyError(name)


def check_calls(log, ops):
    """-> (failures, {name: worst err / bound}) over every logged call"""
    fails, worst = [], {}
    for i, call in enumerate(log):
        f, w = check_call(call, ops)
        fails += [f"call {i} {x}" for x in f]
        if w is not None:
            worst[call["name"]] = max(worst.get(call["name"], 0.0), w)
    return fails, worst


# ====================================================================================================== mirrors
class Arith:
    """arithmetic type and rounding switches of a mirror.  op(): a gemm operand (rounded to bf16 in bf16 mode);
    st(): a result stored with out_dtype=dt; site(name, v): an operand at a named site, where the faults
    "round_in_fp32" / "unrounded_in_bf16" invert the rounding."""

    def __init__(self, dtype, bf16, faults):
        self.dtype, self.bf16, self.faults = dtype, bf16, set(faults)
        self.flip_site = None

    def t(self, x):
        return x.detach().cpu().to(self.dtype)

    def r(self, v):
        return v.float().bfloat16().to(self.dtype)

    def op(self, v):
        return self.r(v) if self.bf16 else v

    st = op

    def site(self, v):
        """the operand the rounding faults act on (one per mirror)"""
        if self.bf16:
            return v if "unrounded_in_bf16" in self.faults else self.r(v)
        return self.r(v) if "round_in_fp32" in self.faults else v


def _sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def _fit(v, n):
    """v cropped / repeated to length n (a gradient returned in the slot of a parameter of another width)"""
    return v.repeat((n + v.numel() - 1) // v.numel())[:n].clone()


def _bn_forward(y, gamma, beta, rm, rv, dims):
    """train-mode batch norm over `dims`: (xhat, invstd, mean, var, pre, new running mean, new running var)"""
    n = 1
    for d in dims:
        n *= y.shape[d]
    shape = [1] * y.dim()
    shape[1] = -1
    mean = y.mean(dims)
    var = ((y - mean.view(shape)) ** 2).sum(dims) / n
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (y - mean.view(shape)) * invstd.view(shape)
    pre = xhat * gamma.view(shape) + beta.view(shape)
    rm2 = (1 - MOM) * rm + MOM * mean
    rv2 = (1 - MOM) * rv + MOM * var * (n / max(n - 1, 1))
    return xhat, invstd, mean, var, pre, rm2, rv2, n


def _bn_backward(g, y, out, xhat, invstd, mean, var, rm_new, gamma, dims, n, faults):
    """(dy, dgamma, dbeta) of train-mode batch norm from g = dL/d(pre)"""
    shape = [1] * y.dim()
    shape[1] = -1
    if "unbiased_var" in faults:
        invstd = 1.0 / torch.sqrt(var * (n / max(n - 1, 1)) + EPS)
        xhat = (y - mean.view(shape)) * invstd.view(shape)
    if "running_mean_in_bwd" in faults:
        xhat = (y - rm_new.view(shape)) * invstd.view(shape)
    dbeta = g.sum(dims)
    dgamma = (g * (out if "dgamma_from_out" in faults else xhat)).sum(dims)
    dy = (gamma * invstd).view(shape) * (g - dbeta.view(shape) / n - xhat * dgamma.view(shape) / n)
    return dy, dgamma, dbeta


# ------------------------------------------------------------------------------------------- model 1 generator
def gen_mirror(inp, *, dtype=torch.float64, bf16=False, faults=(), sel=None):
    """SIMNN.Generator in train mode, forward and backward of loss = (out * R).sum().
    inp: dict(sd = state dict, x = noise (B, nd, 1, 1), R).  sel: three (B, C, H, W) masks `out > 0` of the ReLUs.
    -> dict(out, grads {parameter name: gradient}, dx, running {buffer name: value}, sel)"""
    A = Arith(dtype, bf16, faults)
    sd = {k: A.t(v) for k, v in inp["sd"].items()}
    x, R = A.t(inp["x"]), A.t(inp["R"])
    B = x.shape[0]
    ws = [sd[f"conv{i}.weight"] for i in (1, 2, 3, 4)]
    c_out = ws[3].shape[1]
    saved, running, own_sel = [], {}, []
    h = x
    for li in range(4):
        stride, pad = G_GEOM[li]
        hin = A.site(h) if li == 2 else A.op(h)
        y = F.conv_transpose2d(hin, A.op(ws[li]), None, stride=stride, padding=pad)
        if li < 3:
            bn = f"batch_norm{li + 1}"
            xhat, invstd, mean, var, pre, rm2, rv2, n = _bn_forward(y, sd[bn + ".weight"], sd[bn + ".bias"],
                                                                   sd[bn + ".running_mean"], sd[bn + ".running_var"],
                                                                   (0, 2, 3))
            running[bn + ".running_mean"], running[bn + ".running_var"] = rm2, rv2
            running[bn + ".num_batches_tracked"] = int(inp["sd"][bn + ".num_batches_tracked"]) + 1
            out = torch.where(pre > 0, pre, torch.zeros_like(pre))
            own_sel.append(out > 0)
            saved.append((h, y, out, xhat, invstd, mean, var, rm2, n))
        else:
            out = _sigmoid(y)
            saved.append((h, y, out))
        h = out
    img = out
    if "permute_swapped" in faults and c_out > 1:       # permute_pc(out, b, c_out, pixels): counts exchanged
        cl = out.permute(0, 2, 3, 1).contiguous()
        img = cl.view(B, c_out, -1).permute(0, 2, 1).contiguous().view(out.shape)
    use = own_sel if sel is None else sel
    grads = {}
    d = R
    if "permute_swapped_bwd" in faults and c_out > 1:
        hw = R.shape[2] * R.shape[3]
        d = R.contiguous().view(B, hw, c_out).permute(0, 2, 1).contiguous().view(B, R.shape[2], R.shape[3], c_out)
        d = d.permute(0, 3, 1, 2)
    for li in (3, 2, 1, 0):
        stride, pad = G_GEOM[li]
        w = ws[li]
        if li == 3:
            hprev, y, out = saved[li]
            dy = d if "no_sigmoid_grad" in faults else d * out * (1 - out)
        else:
            hprev, y, out, xhat, invstd, mean, var, rm2, n = saved[li]
            bn = f"batch_norm{li + 1}"
            g = d * use[li].to(dtype)
            dy, dgamma, dbeta = _bn_backward(g, y, out, xhat, invstd, mean, var, rm2, sd[bn + ".weight"], (0, 2, 3), n,
                                             faults if li == 1 else ())
            grads[bn + ".weight"], grads[bn + ".bias"] = dgamma, dbeta
        xs, dys = A.op(hprev), A.op(dy)
        if "drop_last_row" in faults and li == 3:
            xs, dys = xs[:-1], dys[:-1]
        if "im2col_geom" in faults and li == 2:     # layer 3's (stride, pad) = (1, 0) on layer 2's grids
            cin, cout, kh, kw = w.shape
            ih, oh = hprev.shape[2], dy.shape[2]
            dcols = L.im2col_ref(A.op(dy).permute(0, 2, 3, 1).contiguous(), planar=False, B=B, H=oh, W=oh, C=cout,
                                 KH=kh, KW=kw, stride=G_GEOM[3][0], pad=G_GEOM[3][1], OH=ih, OW=ih).to(dtype)
            x2d = A.op(hprev).permute(0, 2, 3, 1).reshape(-1, cin)
            dw = (x2d.t() @ dcols).view(w.shape)
            d = (dcols @ A.op(w).reshape(cin, -1).t()).view(B, ih, ih, cin).permute(0, 3, 1, 2)
        else:
            # y = convT(x, w) is the adjoint of conv2d(., w): dw is conv2d's weight gradient with the roles exchanged
            dw = torch.nn.grad.conv2d_weight(dys, w.shape, xs, stride=stride, padding=pad)
            d = F.conv2d(A.op(dy), A.op(w), None, stride=stride, padding=pad)
        if "dw_tap_major" in faults and li == 2:
            dw = dw.permute(0, 2, 3, 1).contiguous().view(w.shape)
        grads[f"conv{li + 1}.weight"] = dw
    if "swap_grads" in faults:
        grads["batch_norm2.weight"], grads["batch_norm2.bias"] = grads["batch_norm2.bias"], grads["batch_norm2.weight"]
    if "dbeta_other_layer" in faults:
        grads["batch_norm1.bias"] = _fit(grads["batch_norm2.bias"], grads["batch_norm1.bias"].numel())
    return dict(out=img, grads=grads, dx=d, running=running, sel=own_sel)


def gen_sel_from_log(log, B):
    """the device's ReLU selections: `out > 0` of the three recorded bn_act_fwd results, (B*H*W, C) -> (B, C, H, W)"""
    sel = []
    for call in log:
        if call["name"] == "bn_act_fwd":
            o = call["results"][0].value
            hw = int(round((o.shape[0] // B) ** 0.5))
            sel.append((o > 0).view(B, hw, hw, o.shape[1]).permute(0, 3, 1, 2))
    return sel


# ------------------------------------------------------------------------------------------ model 2 generators
def mlp_bn_mirror(inp, *, dtype=torch.float64, bf16=False, faults=(), sel=None, max_rows=256):
    """network_tests.Generator / BeatGenerator in train mode: 4 x [Linear, BatchNorm1d, Sigmoid] on x = cat(noise,
    input).  inp: dict(sd, x (rows, K), R).  bf16 mode with rows <= max_rows: the fused block's split product.
    The BatchNorm faults are planted at the last layer, where no later BatchNorm attenuates them.  At two rows the
    result carries `scale`: the backward pass on absolute values, the scale e2e_ratios divides by (family_of)."""
    A = Arith(dtype, bf16, faults)
    sd = {k: A.t(v) for k, v in inp["sd"].items()}
    x, R = A.t(inp["x"]), A.t(inp["R"])
    rows = x.shape[0]
    fused = bf16 and rows <= max_rows
    n_layers = 4
    saved, running, grads = [], {}, {}
    h = x
    for li in range(n_layers):
        w, b = sd[f"gen.{li}.0.weight"], sd[f"gen.{li}.0.bias"]
        bn = f"gen.{li}.1"
        if fused:
            hh = A.r(h)
            hl = A.r(h - hh)
            wh = A.r(w)
            wl = A.r(w - wh)
            y = hh @ wh.t() + hh @ wl.t() + hl @ wh.t() + b
        else:
            y = (A.site(h) if li == n_layers - 1 else A.op(h)) @ A.op(w).t() + b
        xhat, invstd, mean, var, pre, rm2, rv2, n = _bn_forward(y, sd[bn + ".weight"], sd[bn + ".bias"],
                                                               sd[bn + ".running_mean"], sd[bn + ".running_var"], (0,))
        running[bn + ".running_mean"], running[bn + ".running_var"] = rm2, rv2
        running[bn + ".num_batches_tracked"] = int(inp["sd"][bn + ".num_batches_tracked"]) + 1
        out = _sigmoid(pre)
        saved.append((h, y, out, xhat, invstd, mean, var, rm2, n))
        h = out
    d = R.reshape(rows, -1)
    dm, mags = d.abs(), {}          # the same backward on absolute values: what each difference is a difference OF
    for li in range(n_layers - 1, -1, -1):
        hprev, y, out, xhat, invstd, mean, var, rm2, n = saved[li]
        w = sd[f"gen.{li}.0.weight"]
        g = d * out * (1 - out)
        gm = dm * out * (1 - out)
        k = (sd[f"gen.{li}.1.weight"] * invstd).abs()
        dym = k * (gm + gm.sum(0) / n + xhat.abs() * (gm * xhat.abs()).sum(0) / n)
        mags[f"gen.{li}.0.weight"], mags[f"gen.{li}.0.bias"] = dym.t() @ hprev.abs(), dym.sum(0)
        mags[f"gen.{li}.1.weight"], mags[f"gen.{li}.1.bias"] = (gm * xhat.abs()).sum(0), gm.sum(0)
        dm = dym @ w.abs()
        dy, dgamma, dbeta = _bn_backward(g, y, out, xhat, invstd, mean, var, rm2, sd[f"gen.{li}.1.weight"], (0,), n,
                                         faults if li == n_layers - 1 else ())
        dys = A.op(dy)
        xs = A.site(hprev) if li == n_layers - 1 else A.op(hprev)
        if "drop_last_row" in faults and li == n_layers - 1:
            dys, xs = dys[:-1], xs[:-1]
        grads[f"gen.{li}.0.weight"] = dys.t() @ xs
        grads[f"gen.{li}.0.bias"] = dy.sum(0)
        grads[f"gen.{li}.1.weight"], grads[f"gen.{li}.1.bias"] = dgamma, dbeta
        d = A.op(dy) @ A.op(w)
    if "swap_grads" in faults:
        grads["gen.2.1.weight"], grads["gen.2.1.bias"] = grads["gen.2.1.bias"], grads["gen.2.1.weight"]
    if "dbeta_other_layer" in faults:
        grads["gen.3.1.bias"] = _fit(grads["gen.2.1.bias"], grads["gen.3.1.bias"].numel())
    mags["dx"] = dm
    return dict(out=h.view(inp["R"].shape), grads=grads, dx=d, running=running, sel=[],
                scale=mags if rows == 2 else {})


# ---------------------------------------------------------------------------------------- MLP discriminator
def mlp_leaky_mirror(inp, *, dtype=torch.float64, bf16=False, faults=(), sel=None, slope=SLOPE):
    """network_tests.Discriminator: 3 x [Linear, LeakyReLU(0.2)].  sel: the three masks `out > 0`.  slope: the
    kernels' 0.2f by default (torch's LeakyReLU holds the double 0.2: the autograd comparison passes that)."""
    A = Arith(dtype, bf16, faults)
    sd = {k: A.t(v) for k, v in inp["sd"].items()}
    h, R = A.t(inp["x"]), A.t(inp["R"])
    saved, own_sel, grads = [], [], {}
    for li in range(3):
        w, b = sd[f"disc.{li}.0.weight"], sd[f"disc.{li}.0.bias"]
        pre = A.op(h) @ A.op(w).t() + b
        out = torch.where(pre > 0, pre, pre * slope)
        own_sel.append(out > 0)
        saved.append((h, out))
        h = out
    use = own_sel if sel is None else sel
    d = R
    for li in (2, 1, 0):
        hprev, out = saved[li]
        w = sd[f"disc.{li}.0.weight"]
        dy = d * torch.where(use[li], torch.ones_like(d), torch.full_like(d, 1.0 if "no_slope" in faults else slope))
        dys = A.op(dy)
        xs = A.site(hprev) if li == 0 else A.op(hprev)
        if "drop_last_row" in faults and li == 0:
            dys, xs = dys[:-1], xs[:-1]
        grads[f"disc.{li}.0.weight"] = dys.t() @ xs
        grads[f"disc.{li}.0.bias"] = dy.sum(0)
        d = A.op(dy) @ A.op(w)
    if "swap_grads" in faults:          # the widths differ (16, 32): each lands cropped / tiled in the other's slot
        b0, b1 = grads["disc.0.0.bias"], grads["disc.1.0.bias"]
        grads["disc.0.0.bias"], grads["disc.1.0.bias"] = _fit(b1, b0.numel()), _fit(b0, b1.numel())
    if "bias_other_layer" in faults:
        grads["disc.0.0.bias"] = _fit(grads["disc.1.0.bias"], grads["disc.0.0.bias"].numel())
    return dict(out=h, grads=grads, dx=d, running={}, sel=own_sel)


def leaky_sel_from_log(log):
    return [c["results"][0].value > 0 for c in log if c["name"] == "gemm" and c["kwargs"].get("act") == L.ACT_LEAKY]


# ---------------------------------------------------------------------------------------------------- SimNN
def _pool(v):
    """2x2 / stride 2 floor pooling of (B, C, H, W): (values, idx = window position dy*2+dx of the first maximum)"""
    H, W = v.shape[2], v.shape[3]
    OH, OW = H // 2, W // 2
    win = [v[:, :, dy:2 * OH:2, dx:2 * OW:2] for dy in (0, 1) for dx in (0, 1)]
    m, pos = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        take = win[k] > m
        m = torch.where(take, win[k], m)
        pos = torch.where(take, torch.full_like(pos, k), pos)
    return m, pos


def _unpool(g, idx, H, W):
    dx = torch.zeros(g.shape[0], g.shape[1], H, W, dtype=g.dtype)
    OH, OW = H // 2, W // 2
    for k in range(4):
        dx[:, :, k // 2:2 * OH:2, k % 2:2 * OW:2] = torch.where(idx == k, g, torch.zeros_like(g))
    return dx


def net_mirror(inp, *, dtype=torch.float64, bf16=False, faults=(), sel=None):
    """SIMNN.SimNN: Conv(1->32,k3,p1) ReLU pool, Conv(32->64,k3,p1) ReLU pool, channel-major flatten, Linear ReLU,
    Linear.  sel: dict(a1, a2 = masks (B, C, H, W), hid = mask (B, 512), i1, i2 = pooling indices (B, C, OH, OW))."""
    A = Arith(dtype, bf16, faults)
    sd = {k: A.t(v) for k, v in inp["sd"].items()}
    x, R = A.t(inp["x"]), A.t(inp["R"])
    B, _, H, W = x.shape
    w1, w2, wf1, wf2 = sd["conv1.weight"], sd["conv2.weight"], sd["fc1.weight"], sd["fc2.weight"]
    relu = lambda v: torch.where(v > 0, v, torch.zeros_like(v))      # noqa: E731
    xr = A.st(x)                                                     # im2col(out_dtype=dt)
    a1 = A.st(relu(F.conv2d(xr, A.op(w1), sd["conv1.bias"], padding=1)))
    q1, i1 = _pool(a1)
    a2 = A.st(relu(F.conv2d(q1, A.op(w2), sd["conv2.bias"], padding=1)))
    q2, i2 = _pool(a2)
    flat = q2.permute(0, 2, 3, 1).reshape(B, -1) if "flatten_channels_last" in faults else q2.reshape(B, -1)
    hid = relu(A.op(flat) @ A.op(wf1).t() + sd["fc1.bias"])
    out = A.site(hid) @ A.op(wf2).t() + sd["fc2.bias"]
    own = dict(a1=a1 > 0, a2=a2 > 0, hid=hid > 0, i1=i1, i2=i2)
    s = own if sel is None else sel
    g = {}
    d = R
    g["fc2.weight"], g["fc2.bias"] = A.op(d).t() @ A.op(hid), d.sum(0)
    dhid = (A.op(d) @ A.op(wf2)) * s["hid"].to(dtype)
    dh, fl = A.op(dhid), A.op(flat)
    if "drop_last_row" in faults:
        dh, fl = dh[:-1], fl[:-1]
    g["fc1.weight"], g["fc1.bias"] = dh.t() @ fl, dhid.sum(0)
    dflat = A.st(A.op(dhid) @ A.op(wf1))
    dq2 = dflat.view(q2.shape)
    if "flatten_channels_last" in faults:
        dq2 = dflat.view(B, q2.shape[2], q2.shape[3], q2.shape[1]).permute(0, 3, 1, 2)
    da2 = _unpool(dq2, s["i2"], a2.shape[2], a2.shape[3]) * s["a2"].to(dtype)
    g["conv2.weight"] = torch.nn.grad.conv2d_weight(A.op(q1), w2.shape, A.op(da2), padding=1)
    g["conv2.bias"] = da2.sum((0, 2, 3))
    dq1 = A.st(torch.nn.grad.conv2d_input(q1.shape, A.op(w2), A.op(da2), padding=1))
    da1 = _unpool(dq1, s["i1"], H, W) * s["a1"].to(dtype)
    g["conv1.weight"] = torch.nn.grad.conv2d_weight(xr, w1.shape, A.op(da1), padding=1)
    g["conv1.bias"] = da1.sum((0, 2, 3))
    dx = torch.nn.grad.conv2d_input(x.shape, A.op(w1), A.op(da1), padding=1)
    if "swap_grads" in faults:          # conv1.bias (32) and conv2.bias (64) exchanged, cropped / tiled to fit
        b1, b2 = g["conv1.bias"], g["conv2.bias"]
        g["conv1.bias"], g["conv2.bias"] = _fit(b2, b1.numel()), _fit(b1, b2.numel())
    if "bias_other_layer" in faults:
        g["fc1.bias"] = _fit(g["fc2.bias"], g["fc1.bias"].numel())
    return dict(out=out, grads=g, dx=dx, running={}, sel=own)


def net_sel_from_log(log, B, H, W):
    """a1, a2, hid and the pooling indices as the device made them, in the mirror's (B, C, H, W) layout"""
    relus = [c["results"][0].value for c in log if c["name"] == "gemm" and c["kwargs"].get("act") == L.ACT_RELU]
    idx = [c["results"][1].value for c in log if c["name"] == "maxpool2_fwd"]
    h1, w1 = H // 2, W // 2

    def nchw(t, h, w):
        return t.view(B, h, w, t.shape[1]).permute(0, 3, 1, 2)
    return dict(a1=nchw(relus[0].float() > 0, H, W), a2=nchw(relus[1].float() > 0, h1, w1), hid=relus[2] > 0,
                i1=nchw(idx[0], h1, w1), i2=nchw(idx[1], h1 // 2, w1 // 2))


MIRRORS = dict(simnn_gen=gen_mirror, mlp_bn_sigmoid=mlp_bn_mirror, mlp_leaky=mlp_leaky_mirror, simnn_net=net_mirror)
FAULTS = dict(
    simnn_gen=("permute_swapped", "permute_swapped_bwd", "dw_tap_major", "im2col_geom", "no_sigmoid_grad",
               "dgamma_from_out", "unbiased_var", "swap_grads", "dbeta_other_layer", "round_in_fp32",
               "unrounded_in_bf16", "drop_last_row"),
    mlp_bn_sigmoid=("dgamma_from_out", "unbiased_var", "running_mean_in_bwd", "swap_grads", "dbeta_other_layer",
                    "round_in_fp32", "unrounded_in_bf16", "drop_last_row"),
    mlp_leaky=("no_slope", "swap_grads", "bias_other_layer", "round_in_fp32", "unrounded_in_bf16", "drop_last_row"),
    simnn_net=("flatten_channels_last", "swap_grads", "bias_other_layer", "round_in_fp32", "unrounded_in_bf16",
               "drop_last_row"),
)


# Every planted fault must exceed the end-to-end bound on every case where it changes anything, in both modes, except
# the (fault, case) pairs below, all in bf16 mode.  There the float32 baseline itself holds an error of the fault's
# size: one value crossing a bf16 rounding boundary moves a product by a full bf16 ulp (2^-8 of itself), which at the
# short reductions of these composites (K = rows of a batch) is 2^-8 / sqrt(K) of a weight gradient.
#   unrounded_in_bf16 moves every product by at most half an ulp: in the max norm about one crossing.  It stays
#     required on the model 1 generator, the MLP discriminator (no crossing in its baseline) and two of the two-row
#     cases; on the listed cases the per-call gemm check is what sees it
#     (tests/test_autograd_ref.py::test_per_call_check_rejects_an_unrounded_operand).
#   unbiased_var moves invstd by 1 / (2 N) of itself: listed from N = 256 rows on, and on the generator cases where
#     layer 2's BatchNorm has N = B * 64 >= 192 rows and the measured ratio is within 20% of the bound.
#   drop_last_row moves a weight gradient by ~1 / sqrt(N): listed where N >= 256 and model 2's bf16 weight bound (0.16,
#     from BeatGenerator's first layer: beat times up to 27 against one crossed dy) is at least 1 / 1.2 of that.
# A pair is listed when the fault's worst ratio / bound is below 1.2 here; the CPU test requires every other pair to be
# rejected and every listed pair to stay below 2, so that a listed pair that comes to exceed the bound is noticed.
BF16_BELOW_BASELINE = {
    "unrounded_in_bf16": tuple(f"{m}-rows{r}" for m in ("g1", "g1_64", "g2") for r in (16, 17, 256, 257, 300))
    + ("g2-rows2", "simnn-3x22x30-nodx", "simnn-3x22x30-dx", "simnn-2x37x41-nodx", "simnn-2x37x41-dx"),
    "unbiased_var": ("gen-ref-B5", "gen-ref-B33", "gen-ref-B65", "gen-c3-n37-g8-B3")
    + tuple(f"{m}-rows{r}" for m in ("g1", "g1_64", "g2") for r in (256, 257, 300)),
    "drop_last_row": ("g1-rows300", "g1_64-rows256", "g1_64-rows300", "g2-rows256", "g2-rows257", "g2-rows300"),
}
LISTED_BELOW = 2.0      # a listed pair's worst ratio / bound stays below this


def fault_present(fault, case, bf16):
    """whether the fault changes anything on this case in this mode"""
    if fault in ("round_in_fp32", "unrounded_in_bf16"):
        return bf16 == (fault == "unrounded_in_bf16")
    if fault in ("permute_swapped", "permute_swapped_bwd"):
        return case["channels"] > 1
    return True


def fault_applies(fault, case, bf16):
    """whether the end-to-end check must reject the fault on this case in this mode"""
    if not fault_present(fault, case, bf16):
        return False
    return not (bf16 and case["name"] in BF16_BELOW_BASELINE.get(fault, ()))


# ================================================================================================== case tables
def _case(composite, name, **kw):
    return dict(composite=composite, name=name, **kw)


GEN_CASES = [_case("simnn_gen", f"gen-ref-B{b}", B=b, channels=1, noise_dim=100, gen_dim=32) for b in (2, 5, 33, 65)]
GEN_CASES.append(_case("simnn_gen", "gen-c3-n37-g8-B3", B=3, channels=3, noise_dim=37, gen_dim=8))
MLP_ROWS = (2, 16, 17, 256, 257, 300)
# MultiModalGAN()'s defaults: z_dim 100, hidden 64, adj (28, 28), input_dim 50, output_dim 16
MLP_BN_MODELS = dict(
    g1=dict(cls="Generator", z_dim=100, input_dim=100, hidden=64, adj=(28, 28), out=784, beats=False),
    g1_64=dict(cls="Generator", z_dim=100, input_dim=100, hidden=64, adj=(64, 64), out=4096, beats=False),
    g2=dict(cls="BeatGenerator", z_dim=100, input_dim=50, hidden=64, adj=None, out=16, beats=True),
)
MLP_BN_CASES = [_case("mlp_bn_sigmoid", f"{m}-rows{r}", model=m, B=r, **MLP_BN_MODELS[m])
                for m in MLP_BN_MODELS for r in MLP_ROWS]
LEAKY_CASES = [_case("mlp_leaky", f"mlpd-B{b}-{'dx' if dx else 'nodx'}", B=b, roll=(2, 128, 16), want_dx=dx)
               for b in (2, 33) for dx in (False, True)]
NET_CASES = [_case("simnn_net", f"simnn-{b}x{h}x{w}-{'dx' if dx else 'nodx'}", B=b, H=h, W=w, n=6, want_dx=dx)
             for (b, h, w) in ((3, 22, 30), (2, 37, 41)) for dx in (False, True)]
CASES = GEN_CASES + MLP_BN_CASES + LEAKY_CASES + NET_CASES
CASE = {c["name"]: c for c in CASES}


def _bn_state(sd, prefix, C, g, gamma_mean=1.0):
    sd[prefix + ".weight"] = gamma_mean + 0.2 * torch.randn(C, generator=g)
    sd[prefix + ".bias"] = 0.2 * torch.randn(C, generator=g)
    sd[prefix + ".running_mean"] = 0.1 * torch.randn(C, generator=g)
    sd[prefix + ".running_var"] = 0.5 + torch.rand(C, generator=g)
    sd[prefix + ".num_batches_tracked"] = torch.tensor(3, dtype=torch.long)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the seeded state dict (module key names), input x and upstream gradient R of a case; fp32, never modified"""
    c = CASE[name]
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31 - 1))
    sd, B = {}, c["B"]
    if c["composite"] == "simnn_gen":
        gd, nd, ch = c["gen_dim"], c["noise_dim"], c["channels"]
        shapes = [(nd, 4 * gd, 4, 4), (4 * gd, 2 * gd, 4, 4), (2 * gd, gd, 4, 4), (gd, ch, 5, 5)]
        for i, s in enumerate(shapes):
            sd[f"conv{i + 1}.weight"] = 0.02 * torch.randn(s, generator=g)
        for i, C in enumerate((4 * gd, 2 * gd, gd)):
            _bn_state(sd, f"batch_norm{i + 1}", C, g)
        x = torch.randn(B, nd, 1, 1, generator=g)
        R = torch.randn(B, ch, 20, 20, generator=g)
    elif c["composite"] == "mlp_bn_sigmoid":
        K = c["z_dim"] + c["input_dim"]
        dims = [K, c["hidden"] * 4, c["hidden"] * 2, c["hidden"], c["out"]]
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            sd[f"gen.{i}.0.weight"] = torch.randn(fo, fi, generator=g) * (2.0 / (fi + fo)) ** 0.5      # xavier normal
            sd[f"gen.{i}.0.bias"] = 0.1 * torch.randn(fo, generator=g)
            _bn_state(sd, f"gen.{i}.1", fo, g)
        x = torch.randn(B, K, generator=g)
        if c["beats"]:          # un-normalised cumulative beat times, as tests/test_mmgan_batch_gpu.py::_block
            x[:, c["z_dim"]:] = torch.cumsum(torch.rand(B, c["input_dim"], generator=g) * 0.5 + 0.3, dim=1)
        R = torch.randn((B, 1) + c["adj"] if c["adj"] else (B, c["out"]), generator=g)
    elif c["composite"] == "mlp_leaky":
        dims = [c["roll"][0] * c["roll"][1] * c["roll"][2], 16, 32, 1]
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            sd[f"disc.{i}.0.weight"] = (2 * torch.rand(fo, fi, generator=g) - 1) / fi ** 0.5
            sd[f"disc.{i}.0.bias"] = (2 * torch.rand(fo, generator=g) - 1) / fi ** 0.5
        x = torch.randn(B, dims[0], generator=g)
        R = torch.randn(B, 1, generator=g)
    else:
        n, feat = c["n"], 64 * (c["H"] // 4) * (c["W"] // 4)
        for key, shape, fan in (("conv1", (32, 1, 3, 3), 9), ("conv2", (64, 32, 3, 3), 288),
                                ("fc2", (n * n + 4 * n, 512), 512)):
            sd[key + ".weight"] = (2 * torch.rand(shape, generator=g) - 1) / fan ** 0.5
            sd[key + ".bias"] = (2 * torch.rand(shape[0], generator=g) - 1) / fan ** 0.5
        with torch.random.fork_rng():       # fc1 is re-created by every forward from torch's CPU generator
            torch.manual_seed(net_seed(name))
            fc1 = torch.nn.Linear(feat, 512)
        sd["fc1.weight"], sd["fc1.bias"] = fc1.weight.detach().clone(), fc1.bias.detach().clone()
        x = torch.randn(B, 1, c["H"], c["W"], generator=g)
        R = torch.randn(B, n * n + 4 * n, generator=g)
    return dict(sd=sd, x=x, R=R)


def net_seed(name):
    """the seed set right before a SimNN forward, so that the module draws the case's fc1"""
    return 1000 + CASES.index(CASE[name])


def mirror(name, **kw):
    return MIRRORS[CASE[name]["composite"]](inputs(name), **kw)


# =========================================================================================== end-to-end check
def kind_of(key):
    if key in ("out", "dx"):
        return {"out": "output", "dx": "input"}[key]
    return "weight" if key.endswith(".weight") and (".0." in key or key.startswith(("conv", "fc"))) else "bias"


def _zero_bias_scale(composite, key):
    """a Linear bias in front of train-mode BatchNorm: its gradient is exactly zero -> the weight gradient's scale"""
    return key[:-4] + "weight" if composite == "mlp_bn_sigmoid" and key.endswith(".0.bias") else None


def tensors_of(res):
    """every compared tensor of a mirror's (or the device's) result: out, dx, the gradients, the running statistics"""
    out = {"out": res["out"]}
    if res.get("dx") is not None:
        out["dx"] = res["dx"]
    out.update(res["grads"])
    out.update({k: v for k, v in res["running"].items() if not k.endswith("num_batches_tracked")})
    return out


def e2e_ratios(composite, got, ref):
    """{key: max|got - ref| / max|ref|} over every tensor of `ref` that `got` has (every element)"""
    tg, tr = tensors_of(got), tensors_of(ref)
    res = {}
    for key, r in tr.items():
        if key not in tg or tg[key] is None:
            continue
        r = r.double()
        gq = tg[key].detach().cpu().double().reshape(r.shape)
        zb = _zero_bias_scale(composite, key)
        scale = (tr[zb].double() if zb else r).abs().max().clamp_min(1e-300)
        if key in ref.get("scale", {}):          # the two-row family: the cancellation-free magnitude (family_of)
            scale = ref["scale"][key].double().abs().max().clamp_min(1e-300)
        res[key] = float((gq - r).abs().max() / scale)
    return res


@functools.lru_cache(maxsize=None)
def baseline(name, bf16):
    """ratios of the float32 CPU mirror against the float64 mirror (given the float32 mirror's selections); on one
    thread, so that the float32 summation order does not depend on the number of cores"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        sub = mirror(name, dtype=torch.float32, bf16=bf16)
        ref = mirror(name, dtype=torch.float64, bf16=bf16, sel=sub["sel"] or None)
    finally:
        torch.set_num_threads(threads)
    return e2e_ratios(CASE[name]["composite"], sub, ref)


def family_of(name):
    """The family of a case: its composite -- except model 2's generators at two rows, a family with a scale of its own.
    With two rows BatchNorm's backward is dy = gamma invstd (g0 - g1) / 2 * eps / (d^2 + eps) (d = half the difference
    of the two pre-activations): a difference of terms that agree to eps / (d^2 + eps) ~ 1e-5 of themselves, so any
    fp32 evaluation is off by ~1e-3 of the result, and a bound relative to max|ref| cannot stay below 2^-10.  These
    cases are therefore compared absolutely, as the zero-gradient Linear bias is: every gradient against the same
    backward pass evaluated on absolute values (mlp_bn_mirror's `scale`: |gamma invstd| (|g| + mean|g| + |xhat|
    mean|g xhat|) per layer, carried to dW, db, dgamma, dbeta and dx), i.e. against what the differences are
    differences of.  Gradients below the last layer are attenuated by eps / (d^2 + eps) per BatchNorm, so for them
    this scale says little beyond "no term of the cancellation is wrong"; the last layer's and the per-call checks
    carry the rest: there the float32 baseline falls to 1e-13 of the scale and is pure noise, so no baseline of this
    family counts for less than u = 2^-24, one fp32 rounding of the scale.  Outputs and running statistics keep the
    ordinary scale."""
    c = CASE[name]
    return "mlp_bn_sigmoid[rows=2]" if c["composite"] == "mlp_bn_sigmoid" and c["B"] == 2 else c["composite"]


FAMILIES = ("simnn_gen", "mlp_bn_sigmoid", "mlp_bn_sigmoid[rows=2]", "mlp_leaky", "simnn_net")


@functools.lru_cache(maxsize=None)
def family_bounds(family, bf16):
    """{kind: MARGIN x the largest baseline ratio over the cases of the family in this mode}"""
    worst = {}
    for c in CASES:
        if family_of(c["name"]) == family:
            for key, v in baseline(c["name"], bf16).items():
                worst[kind_of(key)] = max(worst.get(kind_of(key), 0.0), v)
    if family.endswith("[rows=2]"):     # no bound below one fp32 rounding of the scale itself (family_of)
        worst = {k: max(v, L.U) for k, v in worst.items()}
    return {k: MARGIN * v for k, v in worst.items()}


def check_e2e(name, bf16, got, ref, *, what=""):
    """-> (failures, {key: ratio}, {key: ratio / bound})"""
    comp = CASE[name]["composite"]
    bounds = family_bounds(family_of(name), bf16)
    ratios = e2e_ratios(comp, got, ref)
    fails = [f"{what} {key}: max|err| / max|ref| = {v:.3g} > {bounds[kind_of(key)]:.3g}" for key, v in ratios.items()
             if not v <= bounds[kind_of(key)]]
    for key, v in ref["running"].items():
        if key.endswith("num_batches_tracked") and key in got["running"] and int(got["running"][key]) != v:
            fails.append(f"{what} {key}: {int(got['running'][key])} != {v}")
    return fails, ratios, {k: v / bounds[kind_of(k)] for k, v in ratios.items()}


# ===================================================================================== call sites from shapes
def _site(site, m, n, k, ta=F32, la="k", tb=F32, lb="r", comp=F32, tc=F32, bias=False):
    la, lb = ("k" if m == 1 else la), ("k" if n == 1 else lb)       # one row / column: both strides are 1
    return dict(site=site, m=m, n=n, k=k, ta=ta, la=la, tb=tb, lb=lb, comp=comp, tc=tc, bias=bias)


def gemm_sites(name, bf16, max_rows=256):
    """the gemm calls of a case's forward + backward in the order functional.py issues them, from the shapes alone"""
    c = CASE[name]
    dt = BF16 if bf16 else F32
    B, s = c["B"], []
    if c["composite"] == "simnn_gen":
        gd = c["gen_dim"]
        chans = (c["noise_dim"], 4 * gd, 2 * gd, gd, c["channels"])
        grid, ks = (1, 4, 8, 16, 20), (4, 4, 4, 5)
        for li in range(4):
            s.append(_site(f"fwd{li}", B * grid[li] ** 2, chans[li + 1] * ks[li] ** 2, chans[li], comp=dt))
        for li in (3, 2, 1, 0):
            rows, cin, ncol = B * grid[li] ** 2, chans[li], chans[li + 1] * ks[li] ** 2
            s.append(_site(f"dw{li}", cin, ncol, rows, la="r", comp=dt))
            s.append(_site(f"dx{li}", rows, cin, ncol, lb="k", comp=dt))
    elif c["composite"] in ("mlp_bn_sigmoid", "mlp_leaky"):
        if c["composite"] == "mlp_bn_sigmoid":
            dims = [c["z_dim"] + c["input_dim"], c["hidden"] * 4, c["hidden"] * 2, c["hidden"], c["out"]]
            fwd, need_dx = not (bf16 and B <= max_rows), True
        else:
            dims = [c["roll"][0] * c["roll"][1] * c["roll"][2], 16, 32, 1]
            fwd, need_dx = True, c["want_dx"]
        nl = len(dims) - 1
        if fwd:
            for li in range(nl):
                s.append(_site(f"fwd{li}", B, dims[li + 1], dims[li], lb="k", comp=dt, bias=True))
        for li in range(nl - 1, -1, -1):
            s.append(_site(f"dw{li}", dims[li + 1], dims[li], B, la="r", comp=dt))
            if li > 0 or need_dx:
                s.append(_site(f"dx{li}", B, dims[li], dims[li + 1], comp=dt))
    else:
        H, W, n = c["H"], c["W"], c["n"]
        r0, r1 = B * H * W, B * (H // 2) * (W // 2)
        feat, no = 64 * (H // 4) * (W // 4), n * n + 4 * n
        s += [_site("conv1", r0, 32, 9, ta=dt, lb="k", comp=dt, tc=dt, bias=True),
              _site("conv2", r1, 64, 288, ta=dt, lb="k", comp=dt, tc=dt, bias=True),
              _site("fc1", B, 512, feat, ta=dt, lb="k", comp=dt, bias=True),
              _site("fc2", B, no, 512, lb="k", comp=dt, bias=True),
              _site("dwf2", no, 512, B, la="r", comp=dt), _site("dhid", B, 512, no, comp=dt),
              _site("dwf1", 512, feat, B, la="r", tb=dt, comp=dt), _site("dflat", B, feat, 512, comp=dt, tc=dt),
              _site("dw2", 64, 288, r1, ta=dt, la="r", tb=dt, comp=dt), _site("dcols2", r1, 288, 64, ta=dt, comp=dt),
              _site("dw1", 32, 9, r0, ta=dt, la="r", tb=dt, comp=dt)]
        if c["want_dx"]:
            s.append(_site("dcols1", r0, 9, 32, ta=dt, comp=dt))
    return s


def site_plan(site, ops):
    """the library's plan for a call site (fresh 16-byte aligned operands; no launch)"""
    t = {F32: "f32", BF16: "bf16"}
    c = G.Case(site["site"], site["m"], site["n"], site["k"], t[site["ta"]], site["la"], t[site["tb"]], site["lb"],
               site["comp"], ops.default_split_k(site["m"], site["n"], site["k"], site["comp"]), bias_n=site["bias"],
               tc=t[site["tc"]])
    L_ = G.layout(c)
    base = 1 << 20
    return ops.gemm_plan_raw(base, site["ta"], L_["sam"], L_["sak"], 2 * base, site["tb"], L_["sbk"], L_["sbn"],
                             3 * base, site["tc"], site["n"], 1, c.m, c.n, c.k, 4 * base if c.bias_n else None,
                             c.comp, c.split)


def site_of_call(call):
    """a recorded gemm in gemm_sites' terms (without the site's name)"""
    a, b = call["args"][:2]
    kw = call["kwargs"]
    tc = kw.get("out_dtype")
    return dict(m=a.shape[0], n=b.shape[1], k=a.shape[1], ta=_GDT[a.dtype], la="k" if a.strides[1] == 1 else "r",
                tb=_GDT[b.dtype], lb="k" if b.strides[0] == 1 else "r", comp=kw.get("compute", F32),
                tc=F32 if tc is None else tc, bias=kw.get("bias_n") is not None)


def col2im_sites(name):
    """(tap_major, stride) of the generator's forward col2im calls"""
    c = CASE[name]
    if c["composite"] != "simnn_gen":
        return []
    gd = c["gen_dim"]
    return [dict(layer=li, tap_major=co >= 16, stride=G_GEOM[li][0])
            for li, co in ((1, 2 * gd), (2, gd), (3, c["channels"]))]


def bn_sites(name):
    """(rows, C) of the unfused batch norms of a case"""
    c = CASE[name]
    if c["composite"] == "simnn_gen":
        gd = c["gen_dim"]
        return [(c["B"] * 16, 4 * gd), (c["B"] * 64, 2 * gd), (c["B"] * 256, gd)]
    if c["composite"] == "mlp_bn_sigmoid":
        return [(c["B"], n) for n in (c["hidden"] * 4, c["hidden"] * 2, c["hidden"], c["out"])]
    return []
