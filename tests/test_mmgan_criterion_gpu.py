"""GPU: model 2's criterion switch (MMGAN_MIDI_DES/network_tests.py:248-250: BCEWithLogitsLoss | MSELoss | L1Loss) from
the single-workgroup loss kernel through the fused discriminator kernel up to the trainer and ``training_loop``.

The CPU reference everywhere is plain torch in float64 with F.mse_loss / F.l1_loss -- the reference's own arithmetic.
A label travels through the C ABI as ONE fp32 number, so the float64 reference takes the label's fp32 value (0.9 is not
representable; 0 and 1 are): that is what makes "an element exactly equal to the target" a well-defined case.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import _lib, network_tests as NT, ops, synthetic  # noqa: E402
from gan_des_midi_music_gen_amd.train import MmganTrainer  # noqa: E402
from oracle import mmgan as om  # noqa: E402  (checker only)

from helpers import record, rel_l2, round_gradient, round_operand  # noqa: E402

DEV = "cuda"
CRIT64 = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy_with_logits}
# roll length -> data seed: with the weights of torch.manual_seed(8) every one of the 12 float64 logits is at least 0.1
# away from both labels (L1's gradient is discontinuous at z = y), max |z| <= 3.0
DATA_SEED = {50: 31, 48: 32, 34: 31, 32: 33, 18: 39, 16: 35}


def _crit64(criterion, z, y):
    z = torch.as_tensor(z).detach().double().cpu().reshape(-1)
    return CRIT64[criterion](z, torch.full_like(z, float(np.float32(y))))


# ---------------------------------------------------------------------------------------------------- 1. criterion_loss
@pytest.mark.parametrize("criterion", ["mse", "l1"])
@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_criterion_loss_vs_float64(n, target, criterion):
    """fp32 arithmetic with a fixed-order sum: loss to 1e-6 relative, dx to 1e-6 of its largest element."""
    g = torch.Generator().manual_seed(1000 * n + int(10 * target))
    x = torch.randn(n, generator=g) * 1.5 + 0.4
    exact = 5 if n > 5 else None
    if exact is not None:
        x[exact] = float(np.float32(target))          # an element exactly on the label
    x64 = x.double().requires_grad_(True)
    want = CRIT64[criterion](x64, torch.full((n,), float(np.float32(target)), dtype=torch.float64))
    want.backward()
    xd = x.to(DEV)
    loss = torch.full((1,), 123.0, device=DEV)
    out, dx = ops.criterion_loss(xd, target, criterion, loss_out=loss)
    assert out is loss and dx.shape == (n,)
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()), (loss.item(), want.item())
    scale = x64.grad.abs().max().item()
    assert (dx.double().cpu() - x64.grad).abs().max().item() <= 1e-6 * scale
    if exact is not None and criterion == "l1":
        assert dx[exact].item() == 0.0 and x64.grad[exact].item() == 0.0        # sign(0) = 0 as torch
    # accumulate_loss adds to what is there; want_grad=False returns no dx; dx_out is filled in place
    acc = torch.full((1,), 2.5, device=DEV)
    _, none = ops.criterion_loss(xd, target, criterion, loss_out=acc, accumulate_loss=True, want_grad=False)
    assert none is None and abs(acc.item() - (2.5 + want.item())) <= 1e-6 * (2.5 + abs(want.item()))
    buf = torch.zeros(n, device=DEV)
    _, same = ops.criterion_loss(xd, target, criterion, loss_out=acc, dx_out=buf)
    assert same is buf and torch.equal(buf, dx) and acc.item() == loss.item()


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_criterion_loss_bce_is_bce_with_logits(n):
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 2).to(DEV)
    for target in (0.0, 1.0, 0.9):
        la, lb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        _, da = ops.criterion_loss(x, target, "bce", loss_out=la)
        _, db = ops.bce_with_logits(x, target, loss_out=lb)
        assert torch.equal(la, lb) and torch.equal(da, db)
        ops.criterion_loss(x, target, "bce", loss_out=la, accumulate_loss=True, want_grad=False)
        ops.bce_with_logits(x, target, loss_out=lb, accumulate_loss=True, want_grad=False)
        assert torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------ 2. the fused kernel
@functools.lru_cache(maxsize=None)
def _case(t):
    """Everything of one roll length that does not depend on the criterion (computed once, never modified): weights,
    inputs, float64 oracle logits, the packed weights on the device."""
    b = 6
    torch.manual_seed(8)
    ref = om.DiscriminatorCNN(roll_size=(2, 128, t))
    d = synthetic.mmgan_inputs(b, t, seed=DATA_SEED[t])
    real_data = torch.stack([d["piano_roll"], d["durations"]]).permute(1, 0, 2, 3).contiguous()
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        z64 = torch.cat([ref64(d["fake_a"].double()), ref64(real_data.double())]).reshape(-1)
    ps = [p.detach().to(DEV).contiguous() for p in ref.parameters()]
    dev = {k: d[k].to(DEV) for k in ("fake_a", "piano_roll", "durations")}
    return dict(b=b, ref=ref, ref64=ref64, d=d, real_data=real_data, z64=z64, pack=ops.dcnn_pack(*ps, t), dev=dev)


@functools.lru_cache(maxsize=None)
def _big(t):
    return synthetic.mmgan_inputs(600, t, seed=32, device=DEV)["fake_a"].contiguous()


def _head64(criterion, logits, b):
    """Loss and sum of dl from given logits ([fake ; real], labels 0 / 1), in float64."""
    z = logits.detach().double().cpu().reshape(-1).requires_grad_(True)
    loss = CRIT64[criterion](z[:b], torch.zeros(b, dtype=torch.float64)) + \
        CRIT64[criterion](z[b:], torch.ones(len(z) - b, dtype=torch.float64))
    loss.backward()
    return loss.item(), z.grad.sum().item()


@pytest.mark.parametrize("criterion", ["mse", "l1"])
@pytest.mark.parametrize("t", [50, 48, 34, 32, 18, 16])
def test_fused_dcnn_kernel_criterion_vs_float64(t, criterion):
    c = _case(t)
    b, d, dv, pack = c["b"], c["d"], c["dev"], c["pack"]
    z64 = c["z64"]
    margin = torch.minimum(z64.abs(), (z64 - 1.0).abs()).min().item()
    assert margin >= 0.1, f"T={t}: a float64 logit lies {margin:.3f} from a label -- pick another data seed"
    assert z64.abs().max().item() <= 3.05

    lo = torch.zeros(1, device=DEV)
    logits, grads = ops.dcnn_fused(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack, loss_out=lo,
                                   criterion=criterion)
    # ---- the head, exactly: the criterion in float64 on the kernel's OWN logits (no bf16 conv error in between)
    want_loss, want_dbfc = _head64(criterion, logits, b)
    record("fused_dcnn_criterion_head", t=t, criterion=criterion, loss=lo.item(), loss_from_own_logits=want_loss,
           dbfc=grads[5].item(), dbfc_from_own_logits=want_dbfc)
    assert abs(lo.item() - want_loss) <= 1e-5 * abs(want_loss), (lo.item(), want_loss)
    assert abs(grads[5].item() - want_dbfc) <= 1e-5 * abs(want_dbfc) + 1e-7, (grads[5].item(), want_dbfc)

    # ---- against the float64 oracle (bounds of test_fused_dcnn_kernel_vs_oracle_bf16)
    ref64 = copy.deepcopy(c["ref64"])
    lo_f, lo_r = ref64(d["fake_a"].double()).reshape(-1), ref64(c["real_data"].double()).reshape(-1)
    loss64 = CRIT64[criterion](lo_f, torch.zeros(b, dtype=torch.float64)) + \
        CRIT64[criterion](lo_r, torch.ones(b, dtype=torch.float64))
    loss64.backward()
    err = (logits.double().cpu() - z64).abs().max().item()
    record("fused_dcnn_criterion_logits", t=t, criterion=criterion, max_err=err, scale=z64.abs().max().item(),
           loss=lo.item(), loss64=loss64.item())
    assert err <= 2e-2 * z64.abs().max().item(), err
    assert abs(lo.item() - loss64.item()) < 2e-2 * max(1.0, abs(loss64.item())), (lo.item(), loss64.item())
    for (k, pr), g in zip(ref64.named_parameters(), grads):
        if pr.numel() == 1:
            # fc.bias = the sum of dl: checked exactly above; under L1 it is a sum of signs / b that the margin fixes
            if criterion == "l1":
                assert abs(g.item() - pr.grad.item()) <= 1e-5 * abs(pr.grad.item()) + 1e-7, (g.item(), pr.grad.item())
            continue
        q = rel_l2(g.reshape(pr.shape), pr.grad)
        record("fused_dcnn_criterion_gradients", t=t, criterion=criterion, tensor=k, vs_float64_oracle=q)
        assert q < (1e-1 if k.endswith("bias") else 5e-2), (k, q)

    # ---- against the same pass on the CPU with the kernel's roundings in place (test_fused_dcnn_kernel_vs_oracle_bf16)
    rp = {k: v.detach().clone().requires_grad_(True) for k, v in c["ref"].named_parameters()}

    def rounded_pass(x):
        z1 = round_gradient(F.conv2d(x, round_operand(rp["conv1.weight"]), rp["conv1.bias"], stride=2, padding=1))
        h1 = round_operand(F.leaky_relu(z1, 0.2))
        z2 = round_gradient(F.conv2d(h1, round_operand(rp["conv2.weight"]), rp["conv2.bias"], stride=2, padding=1))
        h2 = round_operand(F.leaky_relu(z2, 0.2))
        return F.linear(h2.flatten(1), round_operand(rp["fc.weight"]), rp["fc.bias"])
    (CRIT64[criterion](rounded_pass(d["fake_a"]).squeeze(), torch.zeros(b))
     + CRIT64[criterion](rounded_pass(c["real_data"]).squeeze(), torch.ones(b))).backward()
    for (k, pr), g in zip(rp.items(), grads):
        if pr.numel() == 1:
            continue
        q = rel_l2(g.reshape(pr.shape), pr.grad)
        record("fused_dcnn_criterion_gradients", t=t, criterion=criterion, tensor=k, vs_same_rounding_cpu=q)
        assert q < (1e-2 if k.endswith("bias") else 1e-3), (k, q)

    # ---- behaviour: determinism, the forward-only variant, several samples per workgroup
    lo2 = torch.zeros(1, device=DEV)
    logits2, grads2 = ops.dcnn_fused(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack, loss_out=lo2,
                                     criterion=criterion)
    assert torch.equal(logits, logits2) and torch.equal(lo, lo2) and all(torch.equal(a, g) for a, g in zip(grads, grads2))
    lo_only = torch.zeros(1, device=DEV)
    logits3, none = ops.dcnn_fused(dv["fake_a"], None, t, 1.0, 1.0, pack, loss_out=lo_only, want_grad=False,
                                   criterion=criterion)
    assert none is None and torch.equal(logits3, logits[:b])
    want = _crit64(criterion, logits3, 1.0).item()
    assert abs(lo_only.item() - want) <= 1e-5 * abs(want), (lo_only.item(), want)
    want = CRIT64[criterion](z64[:b], torch.ones(b, dtype=torch.float64)).item()
    assert abs(lo_only.item() - want) < 2e-2 * max(1.0, abs(want))
    big = _big(t)
    lo_big = torch.zeros(1, device=DEV)
    lg_big, _ = ops.dcnn_fused(big, None, t, 1.0, 1.0, pack, loss_out=lo_big, criterion=criterion)
    lg_parts = torch.cat([ops.dcnn_fused(big[i:i + 200], None, t, 1.0, 1.0, pack, loss_out=lo2, want_grad=False,
                                         criterion=criterion)[0] for i in (0, 200, 400)])
    assert torch.equal(lg_big, lg_parts)
    want = _crit64(criterion, lg_big, 1.0).item()
    assert abs(lo_big.item() - want) <= 1e-5 * abs(want), (lo_big.item(), want)


def _fused_through_crit_entry(xa, planes, t, ya, yb, pack, crit, want_grad=True):
    """gdm_dcnn_fused_crit called directly (ops.dcnn_fused keeps "bce" on the original entry point)."""
    p0, p1 = planes
    b = xa.shape[0] + p0.shape[0]
    k = 32 * 32 * (((t // 2) - 2) // 2 + 1)
    logits = torch.empty(b, device=DEV)
    loss = torch.zeros(1, device=DEV)
    grads = [torch.empty(s, device=DEV) for s in ((16, 2, 4, 4), (16,), (32, 16, 4, 4), (32,), (1, k), (1,))]
    lib = _lib.load()
    nb = lib.gdm_dcnn_fused_workspace_bytes(b, t, 1 if want_grad else 0)
    ws = ops.workspace(nb, xa.device)
    gp = [ops._p(g) for g in grads] if want_grad else [None] * 6
    ops._call("gdm_dcnn_fused_crit", ops._p(xa), xa.shape[0], ops._p(p0), ops._p(p1), b, t, float(ya), float(yb),
              ops._p(pack), ops._p(logits), ops._p(loss), 0, 1 if want_grad else 0, *gp, crit, ops._p(ws), nb,
              ops._stream())
    return logits, loss, grads if want_grad else None


@pytest.mark.parametrize("t", [50, 48, 34, 32, 18, 16])
def test_fused_dcnn_kernel_bce_is_unchanged_through_the_new_entry_point(t):
    c = _case(t)
    dv, pack = c["dev"], c["pack"]
    lo = torch.zeros(1, device=DEV)
    logits, grads = ops.dcnn_fused(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack, loss_out=lo)
    lo_n = torch.zeros(1, device=DEV)
    logits_n, grads_n = ops.dcnn_fused(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack,
                                       loss_out=lo_n, criterion="bce")
    logits_c, lo_c, grads_c = _fused_through_crit_entry(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0,
                                                        pack, _lib.CRITERIA["bce"])
    for lg, ls, gs in ((logits_n, lo_n, grads_n), (logits_c, lo_c, grads_c)):
        assert torch.equal(lg, logits) and torch.equal(ls, lo)
        assert len(gs) == 6 and all(torch.equal(a, g) for a, g in zip(gs, grads))
    # and the criterion argument is honoured there: MSE through the raw entry point == ops.dcnn_fused(criterion="mse")
    logits_m, lo_m, grads_m = _fused_through_crit_entry(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0,
                                                        pack, _lib.CRITERIA["mse"])
    lo2 = torch.zeros(1, device=DEV)
    logits2, grads2 = ops.dcnn_fused(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack, loss_out=lo2,
                                     criterion="mse")
    assert torch.equal(logits_m, logits2) and torch.equal(lo_m, lo2) and not torch.equal(lo_m, lo)
    assert all(torch.equal(a, g) for a, g in zip(grads_m, grads2))
    with pytest.raises(ops.GdmError, match="unknown criterion"):
        _fused_through_crit_entry(dv["fake_a"], (dv["piano_roll"], dv["durations"]), t, 0.0, 1.0, pack, 3)
    with pytest.raises(ValueError):
        ops.dcnn_fused(dv["fake_a"], None, t, 1.0, 1.0, pack, loss_out=lo2, criterion="hinge")


# ------------------------------------------------------------------------------------------------------- 3./4. trainer
def _mm(seed, t):
    torch.manual_seed(seed)
    return NT.MultiModalGAN(z_dim=50, adj_size=(64, 64), roll_size=(2, 128, t), input_dim=50, output_dim=20,
                            instrument=0, start=100, end=100 + t, device="cpu")


KEYS = ("piano_roll", "durations", "beats", "noise1", "noise2", "fake_a", "fake_b", "g1_in_a", "g1_in_b")


def _run_bf16(criterion, batches, *, fuse=True, elide=False, graph=False):
    """Three iterations on batches[0], batches[0], batches[1] (capture() runs its two warm-up iterations on the tensors
    it is given; the third batch is copied into them before the replay)."""
    mm = _mm(13, 16).to(DEV)
    tr = MmganTrainer(mm, lr=0.01, compute_dtype="bf16", criterion=criterion, fuse_optimizer=fuse,
                      elide_dead_backward=elide)
    losses = []
    if graph:
        st = {k: batches[0][k].clone() for k in KEYS}
        tr.capture(*[st[k] for k in KEYS])
        for k in KEYS:
            st[k].copy_(batches[1][k])
        dl, gl = tr.replay()
        torch.cuda.synchronize()
        losses.append((dl.item(), gl.item()))
    else:
        for d in (batches[0], batches[0], batches[1]):
            dl, gl = tr.step(*[d[k] for k in KEYS[:7]], g1_in_a=d["g1_in_a"], g1_in_b=d["g1_in_b"])
            losses.append((dl.item(), gl.item()))
    torch.cuda.synchronize()
    assert tr._fused_ok(16) and getattr(tr, "_adam_in_kernel", False) == fuse
    return losses, tr.d.flat.clone(), tr.d.exp_avg.clone(), tr.d.exp_avg_sq.clone()


@pytest.mark.parametrize("criterion", ["mse", "l1"])
def test_trainer_bf16_paths_agree_bit_for_bit(criterion):
    batches = [synthetic.mmgan_inputs(4, 16, seed=700 + i, device=DEV) for i in range(2)]
    base = _run_bf16(criterion, batches)
    assert np.all(np.isfinite(base[0])) and len(base[0]) == 3
    for name, kw in (("fuse_optimizer=False", dict(fuse=False)), ("elide_dead_backward=True", dict(elide=True))):
        other = _run_bf16(criterion, batches, **kw)
        assert other[0] == base[0], (name, other[0], base[0])
        for a, c in zip(base[1:], other[1:]):
            assert torch.equal(a, c), name
    rep = _run_bf16(criterion, batches, graph=True)
    assert rep[0][-1] == base[0][-1], (rep[0], base[0])
    for a, c in zip(base[1:], rep[1:]):
        assert torch.equal(a, c), "capture() + replay()"
    # the criterion reaches the kernel: not the BCE run
    assert _run_bf16("bce", batches)[0] != base[0]


@pytest.mark.parametrize("criterion", ["mse", "l1"])
@pytest.mark.parametrize("t", [16, 30])
def test_trainer_fp32_path_vs_float64_loop(t, criterion):
    """The unfused parity path (T = 30 has no fused kernel instance at all) against a float64 CPU loop of
    network_tests.py:293-315 with torch.optim.Adam(lr=0.01): the tolerances of test_trainer_reproduces_golden_iterations_fp32
    (losses 2e-3 relative to max(1, |loss|), parameters 2e-3 absolute)."""
    b = 4
    assert not ops.dcnn_fused_supported(30)
    mm = _mm(5, t)
    ref = om.DiscriminatorCNN(roll_size=(2, 128, t)).double()
    ref.load_state_dict({k: v.double() for k, v in mm.discriminator.state_dict().items()}, strict=True)
    opt = torch.optim.Adam(ref.parameters(), lr=0.01)
    mm.to(DEV).train()
    results = {}
    for elide in (False, True):
        mme = copy.deepcopy(mm)
        tr = MmganTrainer(mme, lr=0.01, compute_dtype="fp32", criterion=criterion, elide_dead_backward=elide)
        got = []
        for it in range(3):
            d = synthetic.mmgan_inputs(b, t, seed=800 + it, device=DEV)
            dl, gl = tr.step(*[d[k] for k in KEYS[:7]], g1_in_a=d["g1_in_a"], g1_in_b=d["g1_in_b"])
            got.append((dl.item(), gl.item()))
        results[elide] = (got, {k: v.detach().cpu() for k, v in mme.discriminator.state_dict().items()})
    assert results[False][0] == results[True][0]
    assert all(torch.equal(results[False][1][k], results[True][1][k]) for k in results[False][1])
    zeros, ones = torch.zeros(b, dtype=torch.float64), torch.ones(b, dtype=torch.float64)
    for it in range(3):
        d = {k: v.double() for k, v in synthetic.mmgan_inputs(b, t, seed=800 + it).items()}
        real_data = torch.stack([d["piano_roll"], d["durations"]]).permute(1, 0, 2, 3)      # 290
        opt.zero_grad()                                                                     # 293
        disc_loss = CRIT64[criterion](ref(d["fake_a"]).squeeze(), zeros) + \
            CRIT64[criterion](ref(real_data).squeeze(), ones)                               # 304-306
        disc_loss.backward()                                                                # 307
        opt.step()                                                                          # 308
        with torch.no_grad():
            gen_loss = CRIT64[criterion](ref(d["fake_b"]).squeeze(), ones)                  # 313 (D is not stepped again)
        dl, gl = results[False][0][it]
        record("mmgan_trainer_criterion_fp32", t=t, criterion=criterion, it=it, d_loss=dl, d_loss64=disc_loss.item(),
               g_loss=gl, g_loss64=gen_loss.item())
        assert abs(dl - disc_loss.item()) <= 2e-3 * max(1.0, abs(disc_loss.item())), (it, dl, disc_loss.item())
        assert abs(gl - gen_loss.item()) <= 2e-3 * max(1.0, abs(gen_loss.item())), (it, gl, gen_loss.item())
    for k, v in ref.state_dict().items():
        np.testing.assert_allclose(results[False][1][k].numpy(), v.numpy(), rtol=0, atol=2e-3, err_msg=k)


# ------------------------------------------------------------------------------------------------------ 5. training_loop
def test_training_loop_takes_the_criterion():
    kw = dict(num_epochs=1, steps_per_epoch=2, seed=0, log=lambda *_: None)
    d_l1, g_l1 = NT.training_loop(8, criterion="l1", **kw)
    assert len(d_l1) == 2 and len(g_l1) == 2 and np.all(np.isfinite(d_l1 + g_l1))
    d_bce, g_bce = NT.training_loop(8, **kw)
    assert d_l1 != d_bce and g_l1 != g_bce
    with pytest.raises(ValueError):
        MmganTrainer(_mm(0, 50).to(DEV), criterion="hinge")
    with pytest.raises(ValueError):
        NT.training_loop(8, criterion="hinge", **kw)
