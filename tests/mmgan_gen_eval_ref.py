"""float64 reference, bounds and a torch-CPU emulation for the one-launch eval-mode generators of model 2
(csrc/mmgan_gen_eval.hip).  A plain module next to mmgan_ref.py: tests/test_mmgan_gen_eval_ref.py (CPU) and
tests/test_mmgan_gen_eval_gpu.py (GPU) import it.

The chain is four blocks Linear -> BatchNorm1d (running statistics) -> Sigmoid on x = cat(noise, input).  Every block is
mmgan_ref.linear_bn_ref(training=False); its bound E covers the kernel's rounding points (split bf16 operands, three
exact products, fp32 accumulation of 3 K + 2 terms, the affine map and the sigmoid in fp32).

Per layer (the taps): the kernel's y_l and a_l are held to linear_bn_ref's (y, E_y) and (out, E_out) computed ON THE
KERNEL'S OWN previous tap a_{l-1} (layer 1: on the inputs), so a layer is judged on what it was given.

Whole chain (the final outputs): the float64 chain runs on its own activations, and the bound is propagated, nothing is
measured.  If the kernel's input of layer l + 1 is off by at most E_out(l) per element, then its exact product is off
by at most E_out(l) @ |W|^T, and its own rounding error is bounded by linear_bn_ref's E_y evaluated on an input of
magnitude |x| + E_out(l):
    E_y(l + 1) = E_y^own(|x| + E_in) + E_in @ |W|^T,        E_in = E_out(l),
and E_out follows from E_y through the same interval step as in linear_bn_ref's eval branch (mean exact, invstd to
4 u, sigmoid' <= 1/4, 20 u of the sigmoid's own arithmetic): `out_bound` below, asserted equal to linear_bn_ref's on
E_in = 0 by the CPU tests.

`emulate` is the kernel's arithmetic in torch fp32 on the CPU: split operands, three products, fp32 sums (in torch's
order, not the MFMA's: both are inside the bound), with the faults the checker has to catch.
"""
import functools

import torch

import mmgan_ref as R

U = R.U
EPS = 1e-5
HIDDEN = (256, 128, 64)
ROW_TILE = 16                                   # GE_R of the kernel
BATCHES = (1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE + 1, 257, 300)
# name -> (z, in, N4): K1 = z + in
GEOMETRIES = {
    "g1_checkpoint": (50, 50, 4096),            # Generator(z_dim=50, adj_size=(64, 64))
    "g2_checkpoint": (50, 50, 20),              # BeatGenerator(z_dim=50, input_dim=50, output_dim=20)
    "g1_default": (100, 100, 784),              # MultiModalGAN(): Generator(100, adj_size=(28, 28))
    "g2_default": (100, 50, 16),                # BeatGenerator(100, input_dim=50, output_dim=16)
    "edge": (3, 4, 17),                         # K below one k tile, ragged N
}
PAIRS = (("g1_checkpoint", "g2_checkpoint"), ("g1_default", "g2_default"))
FAULTS = ("drop_xh_wl_l4", "no_sigmoid_l3", "batch_stats", "broadcast_noise", "drop_last_tile", "ignore_k_tail")
VEC_NAMES = ("bias", "gamma", "beta", "running_mean", "running_var")


def make_inputs(B, z, n_in, seed, broadcast=False):
    """noise (B, z) ~ N(0, 1) and the second half: un-normalised cumulative beat times (up to ~27), the case behind the
    split operands (mmgan_ref / linear_bn.hip); (1, in) when broadcast."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, z, generator=g)
    rows = 1 if broadcast else B
    inp = torch.cumsum(torch.rand(rows, n_in, generator=g) * 0.5 + 0.3, dim=1)
    return noise, inp


@functools.lru_cache(maxsize=None)
def make_params(name, seed=0):
    """Four layers of (w, bias, gamma, beta, running_mean, running_var), calibrated on a 64-row batch of make_inputs so
    that every layer's normalised values are O(1): running_mean is the layer's column mean plus noise, running_var its
    column variance times a factor in [0.5, 1.5] (never 1), so the final outputs span more than 0.2 ... 0.8 and a
    constant 0.5, an identity BatchNorm or the batch statistics cannot pass."""
    z, n_in, n4 = GEOMETRIES[name]
    g = torch.Generator().manual_seed(1000 + seed + 17 * n4 + z)
    noise, inp = make_inputs(64, z, n_in, 555 + seed)
    x = torch.cat((noise, inp), 1).double()
    layers = []
    dims = (z + n_in, *HIDDEN, n4)
    for K, N in zip(dims[:-1], dims[1:]):
        w = torch.randn(N, K, generator=g) * (2.0 / K ** 0.5)
        bias = torch.randn(N, generator=g) * 0.1
        y = x @ w.double().T + bias.double()
        rm = (y.mean(0) + 0.2 * y.std(0) * torch.randn(N, generator=g).double()).float()
        rv = (y.var(0) * (torch.rand(N, generator=g).double() + 0.5) + 1e-3).float()
        gamma = torch.rand(N, generator=g) + 0.75
        beta = torch.randn(N, generator=g) * 0.5
        layers.append(dict(w=w, bias=bias, gamma=gamma, beta=beta, running_mean=rm, running_var=rv))
        x = torch.sigmoid((y - rm.double()) / torch.sqrt(rv.double() + EPS) * gamma.double() + beta.double())
    return tuple(layers)


def cat_input(noise, inp):
    return torch.cat((noise, inp.expand(noise.shape[0], -1)), 1)


def layer_ref(x, p):
    """One block on x (B, K): {'y': (ref, E), 'out': (ref, E)} of mmgan_ref.linear_bn_ref in eval mode."""
    res = R.linear_bn_ref(x, p["w"], p["bias"], p["gamma"], p["beta"], p["running_mean"], p["running_var"], 0,
                          act=R.ACT_SIGMOID, training=False, eps=EPS)
    return dict(y=res["y"], out=res["out"])


def y_bound(x, E_in, p):
    """E_y of a layer whose input is x (float64 reference) known to E_in per element (module docstring)."""
    w, b = p["w"].double(), p["bias"].double()
    K = w.shape[1]
    own = (R.SPLIT_REL + (3 * K + 2) * U) * ((x.abs() + E_in) @ w.abs().T) + U * b.abs()
    return own + E_in @ w.abs().T


def out_bound(y, Ey, p):
    """E_out from E_y: the eval branch of mmgan_ref.linear_bn_ref (:277-285), with any E_y."""
    gm, bt = p["gamma"].double(), p["beta"].double()
    inv = 1.0 / torch.sqrt(p["running_var"].double() + EPS)
    Einv = 4 * U * inv
    d = y - p["running_mean"].double()
    pre = d * inv * gm + bt
    Epre = (Ey * inv + (d.abs() + Ey) * Einv) * gm.abs() + 4 * U * (pre.abs() + bt.abs())
    o = torch.sigmoid(pre)
    return 0.25 * Epre + 20 * U * o.abs()


def chain_ref(noise, inp, params):
    """The float64 chain on its own activations with the propagated bound: [(y, E_y, out, E_out)] per layer."""
    x = cat_input(noise, inp).double()
    E_in = torch.zeros_like(x)
    res = []
    for p in params:
        lr = layer_ref(x, p)
        y, out = lr["y"][0], lr["out"][0]
        Ey = y_bound(x, E_in, p)
        Eo = out_bound(y, Ey, p)
        res.append((y, Ey, out, Eo))
        x, E_in = out, Eo
    return res


def _split(v):
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def emulate(noise, inp, params, faults=()):
    """The kernel's arithmetic in torch fp32 on the CPU.  Returns dict(ys=[y1..y4], acts=[a1..a3], out=(B, N4)).
    faults: see FAULTS -- xh wl dropped in layer 4; layer 3's sigmoid skipped; batch statistics in place of the
    running ones; the broadcast (row-0) read also applied to the noise half; the last column tile of N4 not written
    (left 0); layer 1's K tail past the last whole 32-column tile ignored."""
    noise, inp = noise.float(), inp.float()
    B = noise.shape[0]
    if "broadcast_noise" in faults:
        noise = noise[:1].expand(B, -1)
    x = cat_input(noise, inp)
    ys, acts = [], []
    for li, p in enumerate(params):
        w = p["w"].float()
        if li == 0 and "ignore_k_tail" in faults:
            keep = x.shape[1] // 32 * 32
            x, w = x[:, :keep], w[:, :keep]
        xh, xl = _split(x)
        wh, wl = _split(w)
        y = xl @ wh.T
        if not (li == 3 and "drop_xh_wl_l4" in faults):
            y = y + xh @ wl.T
        y = y + xh @ wh.T + p["bias"].float()
        mean, var = p["running_mean"].float(), p["running_var"].float()
        if "batch_stats" in faults:
            mean, var = y.mean(0), y.var(0, unbiased=False)
        alpha = (1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))) * p["gamma"].float()
        pre = (y - mean) * alpha + p["beta"].float()
        a = pre if (li == 2 and "no_sigmoid_l3" in faults) else 1.0 / (1.0 + torch.exp(-pre))
        ys.append(y)
        if li < 3:
            acts.append(a)
            x = a
    out = a.clone()
    if "drop_last_tile" in faults:
        n4 = out.shape[1]
        out[:, (n4 - 1) // 16 * 16:] = 0.0
        ys[3] = ys[3].clone()
        ys[3][:, (n4 - 1) // 16 * 16:] = 0.0
    return dict(ys=ys, acts=acts, out=out)


def where_row(name):
    def f(idx):
        return f"{name} row {idx[0]} (row tile {idx[0] // ROW_TILE}, row {idx[0] % ROW_TILE} of it), column {idx[1]}"
    return f


def check_run(got, noise, inp, params, *, chain=None, what=""):
    """got: dict(ys, acts, out) of the kernel (or the emulation) on (noise, inp).  Every tap against its layer's bound
    from the run's own previous tap, the final outputs against the propagated chain bound.  Returns {name: worst
    |err| / bound}; raises mmgan_ref.CheckError."""
    res = {}
    x = cat_input(noise, inp)
    for li, p in enumerate(params):
        lr = layer_ref(x, p)
        res[f"y{li + 1}"] = R.check_abs(got["ys"][li], *lr["y"], what=f"{what} y{li + 1}", where=where_row(f"y{li + 1}"))
        a = got["acts"][li] if li < 3 else got["out"]
        name = f"a{li + 1}" if li < 3 else "out_layer"
        res[name] = R.check_abs(a, *lr["out"], what=f"{what} {name}", where=where_row(name))
        x = a.detach().cpu().float()
    chain = chain if chain is not None else chain_ref(noise, inp, params)
    _y, _Ey, out, Eo = chain[3]
    res["out_chain"] = R.check_abs(got["out"], out, Eo, what=f"{what} out (chain)", where=where_row("out"))
    return res
