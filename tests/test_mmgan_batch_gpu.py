"""GPU: model 2's generator blocks (csrc/linear_bn.hip) per element against the float64 reference of
tests/mmgan_ref.py, and the fused discriminator's (csrc/mmgan_dcnn.hip) launch plan and cross-sample invariants at the
batch sizes the trainer runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import _lib, ops, synthetic  # noqa: E402

import mmgan_ref as R  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
LAYERS = [(100, 256), (256, 128), (128, 64), (64, 4096), (64, 20)]       # every generator block (K, N)
ROWS = [2, 16, 17, 31, 32, 33, 64, 65, 100, 129, 255, 256]


def _cap():
    return R.cap_for(torch.cuda.get_device_properties(0).multi_processor_count)


def _block(K, N, M, seed, groups=1, beats=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(groups * M, K, generator=g)
    if beats:                       # un-normalised cumulative beat times (up to ~27), the case behind the split operands
        x[:, K // 2:] = torch.cumsum(torch.rand(groups * M, K - K // 2, generator=g) * 0.5 + 0.3, dim=1)
    return dict(x=x, w=torch.randn(N, K, generator=g) / K ** 0.5, bias=torch.randn(N, generator=g) * 0.1,
                gamma=torch.rand(N, generator=g) + 0.5, beta=torch.randn(N, generator=g),
                running_mean=torch.randn(N, generator=g) * 0.1, running_var=torch.rand(N, generator=g) + 0.5)


def _run(c, *, act, training, save_y, groups=1, stat_repeats=1, x_dev=None):
    d = {k: v.to(DEV) for k, v in c.items()}
    nbt = torch.full((), 3, dtype=torch.long, device=DEV)
    out, y, mean, invstd = ops.linear_bn_act_fwd(d["x"] if x_dev is None else x_dev, d["w"], d["bias"], d["gamma"],
                                                 d["beta"], d["running_mean"], d["running_var"], nbt, act=act,
                                                 training=training, save_y=save_y, groups=groups,
                                                 stat_repeats=stat_repeats)
    got = dict(out=out, save_mean=mean, save_invstd=invstd, running_mean=d["running_mean"],
               running_var=d["running_var"])
    if save_y:
        got["y"] = y
    return got, int(nbt.item())


def _check(c, got, nbt, *, act, training, groups=1, stat_repeats=1, what=""):
    ref = R.linear_bn_ref(*[c[k] for k in ("x", "w", "bias", "gamma", "beta", "running_mean", "running_var")], 3,
                          act=act, training=training, groups=groups, stat_repeats=stat_repeats)
    M = c["x"].shape[0] // groups
    worst = R.check_linear_bn(got, ref, M=M, what=what)
    assert nbt == ref["num_batches_tracked"], (what, nbt)
    record("linear_bn_vs_float64", case=what, **{k: round(v, 4) for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("K,N", LAYERS)
def test_linear_bn_every_layer_and_row_count(K, N):
    """Every generator layer at every row count of the table (row passes of 32, tiles of 16, waves of 64 skipped or
    partial), training, sigmoid; M = 256 with save_y=False is the production branch (no per-row test)."""
    for i, M in enumerate(ROWS):
        c = _block(K, N, M, 100 + i)
        for save_y in ((False, True) if M == 256 else (i % 2 == 0,)):
            got, nbt = _run(c, act=R.ACT_SIGMOID, training=True, save_y=save_y)
            _check(c, got, nbt, act=R.ACT_SIGMOID, training=True, what=f"K={K} N={N} M={M} save_y={save_y}")


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID])
@pytest.mark.parametrize("training", [True, False])
def test_linear_bn_activations_modes_and_tails(act, training):
    """Activations x train/eval on the production row count and on odd ones, plus K / N tails (K % 4 != 0 takes the
    scalar staging path) and an input view at a 4-byte storage offset (misaligned: scalar path too)."""
    for K, N, M in ((100, 256, 256), (64, 20, 65), (8, 33, 31), (37, 1, 100), (37, 33, 256)):
        c = _block(K, N, M, 7 * K + N + M)
        for save_y in (False, True):
            got, nbt = _run(c, act=act, training=training, save_y=save_y)
            _check(c, got, nbt, act=act, training=training, what=f"act={act} training={training} K={K} N={N} M={M}")
    c = _block(64, 128, 100, 9)
    buf = torch.empty(c["x"].numel() + 1, device=DEV)
    xv = buf[1:].view(100, 64)
    xv.copy_(c["x"].to(DEV))
    assert xv.data_ptr() % 16 == 4
    got, nbt = _run(c, act=act, training=training, save_y=True, x_dev=xv)
    _check(c, got, nbt, act=act, training=training, what="offset view")


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("stat_repeats", [1, 2])
def test_linear_bn_groups_and_repeats(groups, stat_repeats):
    """groups launch GP = 2 slots per workgroup (3: an odd tail whose second slot stores nothing); the running
    statistics take groups x stat_repeats updates in group order."""
    for K, N, M in ((100, 256, 256), (64, 20, 33)):
        c = _block(K, N, M, 31 * groups + stat_repeats + K, groups=groups)
        got, nbt = _run(c, act=R.ACT_SIGMOID, training=True, save_y=True, groups=groups, stat_repeats=stat_repeats)
        _check(c, got, nbt, act=R.ACT_SIGMOID, training=True, groups=groups, stat_repeats=stat_repeats,
               what=f"groups={groups} stat_repeats={stat_repeats} K={K} N={N} M={M}")


def test_linear_bn_two_jobs_in_one_launch():
    c1, c2 = _block(100, 256, 256, 41, groups=2), _block(64, 4096, 16, 42)
    d1, d2 = ({k: v.to(DEV) for k, v in c.items()} for c in (c1, c2))
    n1, n2 = (torch.zeros((), dtype=torch.long, device=DEV) for _ in range(2))
    (o1, m1, i1), (o2, m2, i2) = ops.linear_bn_act_fwd_multi(
        [dict(d1, nbt=n1, groups=2), dict(d2, nbt=n2, stat_repeats=2)], act=R.ACT_SIGMOID)
    for c, d, o, m, i, nbt, kw in ((c1, d1, o1, m1, i1, n1, dict(groups=2)), (c2, d2, o2, m2, i2, n2,
                                                                              dict(stat_repeats=2))):
        ref = R.linear_bn_ref(*[c[k] for k in ("x", "w", "bias", "gamma", "beta", "running_mean", "running_var")], 0,
                              act=R.ACT_SIGMOID, **kw)
        R.check_linear_bn(dict(out=o, save_mean=m, save_invstd=i, running_mean=d["running_mean"],
                               running_var=d["running_var"]), ref, M=c["x"].shape[0] // kw.get("groups", 1),
                          what=f"multi {kw}")
        assert int(nbt.item()) == ref["num_batches_tracked"]


# ------------------------------------------------------------------------------------------------ fused DCNN
def _nb_from_workspace(B, T):
    return _lib.load().gdm_dcnn_fused_workspace_bytes(B, T, 1) // (4 * R.slab_width(T)) - 65


def _params(t, seed=8):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(16, 2, 4, 4, generator=g) * 0.1, torch.randn(16, generator=g) * 0.1,
            torch.randn(32, 16, 4, 4, generator=g) * 0.05, torch.randn(32, generator=g) * 0.1,
            torch.randn(1, R.dims(t)["KFC"], generator=g) * 0.01, torch.randn(1, generator=g) * 0.1]


def _launch(x, B, bs, t, ya, yb, pack, *, want_grad=True, loss_init=None, adam=None, grad_out=None):
    xa = x[:bs].contiguous() if bs else None
    planes = (x[bs:B, 0].contiguous(), x[bs:B, 1].contiguous()) if bs < B else None
    lo = torch.full((1,), 0.0 if loss_init is None else loss_init, device=DEV)
    logits, grads = ops.dcnn_fused(xa, planes, t, ya, yb, pack, loss_out=lo, want_grad=want_grad,
                                   accumulate_loss=loss_init is not None, adam=adam, grad_out=grad_out)
    assert logits.numel() == B
    got = dict(logits=logits, loss=lo)
    if want_grad:
        got.update(zip(R.GRAD_NAMES, grads))
    return got


def _inputs(B, t, seed, continuous):
    x = synthetic.mmgan_inputs(B, t, seed=seed)["fake_a"]
    if continuous:                  # values bf16 does not hold: the kernel's input rounding is seen
        x = x + torch.rand(x.shape, generator=torch.Generator().manual_seed(seed))
    return x


@pytest.mark.parametrize("t", R.T_VALUES)
def test_dcnn_fused_vs_float64(t):
    """gdm_dcnn_fused against the same-rounding float64 reference (||err|| / ||M|| <= RL_BF16 per output): logits,
    loss and all six gradients.  T = 50 runs the whole table -- B in dcnn_batches(cap) (1, 2, 12, cap, cap + 1, 512,
    2 cap + 1), every split of dcnn_splits(B), labels (0, 1) and for B = 512 also (1, 1), integer rolls and
    continuous inputs -- the other roll lengths a reduced one.  want_grad=False and accumulate_loss=True ride along.
    The workgroup count read back from the workspace size equals the mirror, which proves the 1-, 2- and 3-round and
    mixed-label regimes ran on this device."""
    cap = _cap()
    ps = _params(t)
    pack = ops.dcnn_pack(*[p.to(DEV).contiguous() for p in ps], t)
    Bs = R.dcnn_batches(cap) if t == 50 else [cap + 1, 512]
    seen, worst = set(), {}
    for B in Bs:
        nb = R.n_blocks(B, cap)
        assert _nb_from_workspace(B, t) == nb, B
        for continuous in ((False, True) if B == 512 or t != 50 else (False,)):
            x = _inputs(B, t, 61 + t + B, continuous)
            xd = x.to(DEV)
            splits = R.dcnn_splits(B) if t == 50 else [B // 2]
            for bs in splits:
                labels = [(0.0, 1.0), (1.0, 1.0)] if (B == 512 and bs == B // 2) else [(0.0, 1.0)]
                for ya, yb in labels:
                    reg = R.regimes(B, bs, cap)
                    seen.add((reg["rounds"], reg["mixed"]))
                    what = f"T={t} B={B} nb={nb} bsplit={bs} y=({ya},{yb}) continuous={continuous}"
                    got = _launch(xd, B, bs, t, ya, yb, pack)
                    ref = R.dcnn_ref(x, bs, ya, yb, ps)
                    for k, v in R.check_dcnn(got, ref, bound=R.RL_BF16, what=what).items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    fwd = _launch(xd, B, bs, t, ya, yb, pack, want_grad=False, loss_init=1.5)
                    assert torch.equal(fwd["logits"], got["logits"]), what
                    R.check_dcnn(dict(loss=fwd["loss"]), R.dcnn_ref(x, bs, ya, yb, ps, loss_init=1.5),
                                 bound=R.RL_BF16, what=what + " want_grad=False accumulate_loss")
    record("dcnn_fused_vs_float64", t=t, **{k: round(v, 4) for k, v in worst.items()})
    if t == 50:
        assert {1, 2, 3} <= {r for r, _ in seen} and any(m for _, m in seen), seen


@pytest.mark.parametrize("t", [50, 16])
def test_dcnn_fused_logits_do_not_depend_on_the_workgroup_schedule(t):
    """Every sample's logit is computed by one workgroup from its own planes: it must be bit-identical whether that
    workgroup handles it alone or as its 2nd / 3rd sample after others (halos and the column groups past OW1 stay
    zero across samples; staging of the next sample does not leak into the current one)."""
    cap = _cap()
    ps = _params(t, seed=9)
    pack = ops.dcnn_pack(*[p.to(DEV).contiguous() for p in ps], t)
    Bs = [cap + 1, 512, 2 * cap + 1] if t == 50 else [512]
    x = _inputs(max(Bs), t, 77 + t, t != 50).to(DEV)
    lo = torch.zeros(1, device=DEV)
    alone = torch.cat([ops.dcnn_fused(x[b:b + 1].contiguous(), None, t, 1.0, 1.0, pack, loss_out=lo,
                                      want_grad=False)[0] for b in range(max(Bs))])
    for B in Bs:
        nb = R.n_blocks(B, cap)
        logits = _launch(x, B, B // 2, t, 0.0, 1.0, pack)["logits"]
        bad = (logits != alone[:B]).nonzero()
        if bad.numel():
            raise AssertionError(f"T={t} B={B}: {bad.numel()} logits differ from single-sample launches; first "
                                 f"{R.where_sample(B, nb, B // 2)((int(bad[0]),))}")


def test_dcnn_fused_adam_at_b512():
    """FINISH = 2 (the optimizer step inside the slab sum): gradients bit-identical to a plain launch, parameters and
    moments equal to float64 Adam on those gradients (a few fp32 roundings), and the refreshed pack equal to
    dcnn_pack of the updated parameters byte for byte (except the last 16 padding bytes)."""
    t, B, bs = 50, 512, 256
    ps = _params(t, seed=12)
    x = _inputs(B, t, 5, False).to(DEV)
    dev_ps = [p.to(DEV).contiguous() for p in ps]
    plain = _launch(x, B, bs, t, 0.0, 1.0, ops.dcnn_pack(*dev_ps, t))
    lr, b1, b2, eps = 0.01, 0.5, 0.999, 1e-8
    m0 = [torch.randn(p.shape, generator=torch.Generator().manual_seed(i)) * 1e-3 for i, p in enumerate(ps)]
    v0 = [torch.rand(p.shape, generator=torch.Generator().manual_seed(10 + i)) * 1e-6 for i, p in enumerate(ps)]
    params = [p.clone() for p in dev_ps]
    adam = dict(params=params, exp_avg=[m.to(DEV) for m in m0], exp_avg_sq=[v.to(DEV) for v in v0],
                hyper=ops.adam_hyper(DEV, lr, b1, b2, eps, step=3), done=torch.zeros(1, dtype=torch.int32, device=DEV))
    pack = ops.dcnn_pack(*dev_ps, t)
    got = _launch(x, B, bs, t, 0.0, 1.0, pack, adam=adam)
    for k in R.GRAD_NAMES:
        assert torch.equal(got[k], plain[k]), k
    step = 4
    lr, b1, b2, eps = (float(torch.tensor(v, dtype=torch.float32)) for v in (lr, b1, b2, eps))   # the record's fp32 values
    for i, k in enumerate(R.GRAD_NAMES):
        g, p, m, v = (q.detach().cpu().double() for q in (got[k], ps[i], m0[i], v0[i]))
        g = g.reshape(p.shape)
        m1 = b1 * m + (1 - b1) * g
        v1 = b2 * v + (1 - b2) * g * g
        upd = (lr / (1 - b1 ** step)) * m1 / (v1.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
        p1 = p - upd
        u = 2.0 ** -24
        tol_m = 4 * u * (b1 * m.abs() + (1 - b1) * g.abs())
        tol_v = 4 * u * (b2 * v + (1 - b2) * g * g)
        tol_p = 2 * u * p.abs() + 16 * u * upd.abs() + (lr / (1 - b1 ** step)) * tol_m / (v1.sqrt() / (1 - b2 ** step)
                                                                                       ** 0.5 + eps)
        for name, got_, want, tol in (("m", adam["exp_avg"][i], m1, tol_m), ("v", adam["exp_avg_sq"][i], v1, tol_v),
                                      ("p", params[i], p1, tol_p)):
            err = (got_.detach().cpu().double().reshape(want.shape) - want).abs()
            assert bool((err <= tol + 1e-30).all()), (k, name, float((err - tol).max()))
    fresh = ops.dcnn_pack(*params, t)
    assert torch.equal(pack[:-16], fresh[:-16])


def test_dcnn_fp32_parity_path_at_b256():
    """functional.dcnn_forward / dcnn_backward in exact fp32 at b = 256 against the unrounded float64 reference."""
    from gan_des_midi_music_gen_amd import functional as Fn
    t, B = 50, 256
    ps = _params(t, seed=14)
    x = _inputs(B, t, 15, True)
    w1, b1, w2, b2, wf, bf = (p.to(DEV).contiguous() for p in ps)
    logits, saved = Fn.dcnn_forward(x.to(DEV), w1, b1, w2, b2, wf, bf, ops.F32)
    dl = ((torch.sigmoid(logits) - 1.0) / B).contiguous()
    grads = Fn.dcnn_backward(saved, dl, w2, wf, ops.F32)[:6]
    ref = R.dcnn_ref(x, 0, 0.0, 1.0, ps, bf16=False)
    got = dict(logits=logits.reshape(-1), **dict(zip(R.GRAD_NAMES, grads)))
    worst = R.check_dcnn(got, ref, bound=R.RL_F32, what="fp32 parity b=256")
    record("dcnn_fp32_parity_vs_float64", **{k: round(v, 4) for k, v in worst.items()})
