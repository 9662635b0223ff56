"""GPU: model 1's eval-mode generator forward in one launch (gdm_simnn_gen_eval, csrc/simnn_gen.hip gen_eval_kernel)
against the float64 references of tests/simnn_gen_eval_ref.py: every layer on the kernel's own taps with the derived
bounds of simnn_gen_ref, the whole chain by rel-L2, the checkpoint fixture on its deviation from 0.5, bit-level
properties (taps change nothing, a sample does not depend on its batch, graph replay), the module surface
(Generator.eval() in bf16, SIMNN.sample_matrices) and the argument checks.

Parameters are calibrated (simnn_gen_eval_ref.calibrated_params) and every float64 comparison first asserts that its
reference output spans 0.35 .. 0.65: a kernel that returns 0.5 everywhere fails each of them.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import SIMNN, functional as Fn, ops  # noqa: E402

import simnn_gen_eval_ref as E  # noqa: E402
import simnn_gen_ref as R  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
FAMILY_CASES = [("base", B, nd) for nd in E.NOISE_DIMS for B in E.BATCHES] + \
               [("zero", 5, 100), ("zero", 129, 100), ("saturate", 16, 100), ("saturate", 257, 100)]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _dev(ws, bns):
    return [w.to(DEV) for w in ws], [tuple(v.to(DEV) for v in bn) for bn in bns]


def _setup(seed, family, B, noise_dim, noise_seed=None):
    ws, bns = E.calibrated_params(seed, family, noise_dim)
    noise = E.case_noise(B, noise_dim, B if noise_seed is None else noise_seed)
    ws_d, bn_d = _dev(ws, bns)
    pack = ops.simnn_gen_pack(ws_d[0], ws_d[1], ws_d[2])
    return ws, bns, noise, ws_d, bn_d, pack


@pytest.mark.parametrize("family,B,noise_dim", FAMILY_CASES, ids=lambda v: str(v))
def test_every_layer_against_float64(family, B, noise_dim):
    """tap_y1 against first_ref, tap_invstd within 4 u, tap_y2 / tap_y3 against convt_ref on the previous tap, out
    against last_ref on tap_y3: each element within its derived bound."""
    ws, bns, noise, ws_d, bn_d, pack = _setup(1000 * noise_dim + B, family, B, noise_dim)
    ref = E.chain_eval_ref(noise, ws, bns)
    what = f"{family} B={B} noise_dim={noise_dim}"
    if family == "saturate":
        assert float(ref.min()) < 1e-6 and float(ref.max()) > 1 - 1e-6, "the family must saturate the sigmoid"
    else:
        E.assert_moves(ref, what)
    got = ops.simnn_gen_eval(noise.to(DEV), pack, ws_d[3], bn_d, taps=True)
    torch.cuda.synchronize()
    out, y1, y2, y3, inv = got
    assert out.shape == (B, 1, 20, 20) and y1.shape == (B * 16, 128) and y2.shape == (B * 64, 64)
    assert y3.shape == (B * 256, 32) and inv.shape == (224,)
    worst = E.check_layers(noise, ws, bns, *got, what=what)
    if family == "zero":
        assert float(y2[:, 7].abs().max()) == 0.0 and float(inv[128 + 7]) == pytest.approx(1 / R.EPS ** 0.5, rel=1e-6)
    print(what, {k: round(v, 4) for k, v in worst.items()})
    record("simnn_gen_eval_layers_vs_float64", case=what, **{k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("B", [1, 16, 257])
def test_taps_change_nothing(B):
    ws, bns, noise, ws_d, bn_d, pack = _setup(7 + B, "base", B, 100)
    x = noise.to(DEV)
    plain = ops.simnn_gen_eval(x, pack, ws_d[3], bn_d)
    tapped = ops.simnn_gen_eval(x, pack, ws_d[3], bn_d, taps=True)[0]
    again = ops.simnn_gen_eval(x, pack, ws_d[3], bn_d)
    torch.cuda.synchronize()
    assert torch.equal(plain, tapped) and torch.equal(plain, again)
    E.assert_moves(plain.cpu())


@pytest.mark.parametrize("B", [257, 31])
def test_a_sample_does_not_depend_on_its_batch(B):
    """Row i of a call with B samples is bit-identical to a B = 1 call on that row's noise."""
    ws, bns, noise, ws_d, bn_d, pack = _setup(40 + B, "base", B, 100)
    x = noise.to(DEV)
    whole = ops.simnn_gen_eval(x, pack, ws_d[3], bn_d)
    rows = torch.cat([ops.simnn_gen_eval(x[i:i + 1].contiguous(), pack, ws_d[3], bn_d) for i in range(B)])
    torch.cuda.synchronize()
    E.assert_moves(whole.cpu())
    assert torch.equal(whole, rows), f"{int((whole != rows).any(dim=(1, 2, 3)).sum())} of {B} rows differ"


@pytest.mark.parametrize("B,noise_dim", [(1, 100), (3, 37), (16, 100), (129, 128), (256, 100), (257, 100), (512, 1)],
                         ids=str)
def test_whole_chain_against_float64(B, noise_dim):
    """functional.simnn_gen_forward in eval mode (the route every caller takes) against chain_eval_ref by rel-L2 <=
    CHAIN_RELL2.  Measured worst value: simnn_gen_eval_ref.MEASURED_CHAIN_RELL2."""
    ws, bns, noise, ws_d, bn_d, _ = _setup(50 + B, "base", B, noise_dim)
    ref = E.chain_eval_ref(noise, ws, bns)
    E.assert_moves(ref, f"B={B}")
    x = noise.to(DEV).view(B, noise_dim, 1, 1)
    assert Fn._gen_eval_ok(ws_d, False, Fn.BF16)
    out, saved = Fn.simnn_gen_forward(x, ws_d, bn_d, False, Fn.BF16, cache={}, need_backward=True)
    torch.cuda.synchronize()
    assert saved is None and out.shape == (B, 1, 20, 20)
    rl2, ratio = E.chain_ratio(out, ref)
    print(f"whole chain B={B} noise_dim={noise_dim}: rel-L2 {rl2:.3g}")
    record("simnn_gen_eval_chain_vs_float64", case=f"B={B} noise_dim={noise_dim}", out_rel_l2=float(f"{rl2:.3g}"))
    E.check_chain(out, ref, what=f"B={B} noise_dim={noise_dim}")


def _module_state(gen):
    return {k: v.detach().clone() for k, v in gen.state_dict().items()}


def _same_state(gen, before):
    return all(torch.equal(v, before[k]) for k, v in gen.state_dict().items())


def _calibrated_generator(seed):
    ws, bns = E.calibrated_params(seed)
    gen = SIMNN.Generator()
    with torch.no_grad():
        for m, w in zip((gen.conv1, gen.conv2, gen.conv3, gen.conv4), ws):
            m.weight.copy_(w)
        for m, (g, be, rm, rv, nbt) in zip((gen.batch_norm1, gen.batch_norm2, gen.batch_norm3), bns):
            m.weight.copy_(g), m.bias.copy_(be), m.running_mean.copy_(rm), m.running_var.copy_(rv)
            m.num_batches_tracked.fill_(int(nbt))
    return gen.to(DEV), ws, bns


@pytest.mark.parametrize("B", [1, 5])
def test_module_in_eval_mode_takes_the_kernel(B):
    gen, ws, bns = _calibrated_generator(21)
    gen.eval()
    gen.compute_dtype = "bf16"
    noise = E.case_noise(B, 100, 9 + B).to(DEV).view(B, 100, 1, 1)
    before = _module_state(gen)
    with torch.no_grad():
        out = gen(noise)
    ws_d, bn_d = _dev(ws, bns)
    want = ops.simnn_gen_eval(noise.view(B, 100), ops.simnn_gen_pack(ws_d[0], ws_d[1], ws_d[2]), ws_d[3], bn_d)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and _same_state(gen, before) and not gen.training
    E.check_chain(out, E.chain_eval_ref(noise.cpu(), ws, bns))
    # a weight changed in place: the cached pack follows
    with torch.no_grad():
        gen.conv2.weight.mul_(0.5)
        out2 = gen(noise)
    ws2 = [ws[0], ws[1] * 0.5, ws[2], ws[3]]
    E.check_chain(out2, E.chain_eval_ref(noise.cpu(), ws2, bns), what="after an in-place weight update")
    # backward through eval-mode BatchNorm keeps raising
    loss = gen(noise.clone().requires_grad_(True)).sum()
    with pytest.raises(NotImplementedError):
        loss.backward()


def test_fp32_eval_keeps_the_layerwise_route():
    gen, ws, bns = _calibrated_generator(22)
    ws_d, bn_d = _dev(ws, bns)
    noise = E.case_noise(3, 100, 1).to(DEV).view(3, 100, 1, 1)
    assert not Fn._gen_eval_ok(ws_d, False, Fn.F32) and not Fn._gen_eval_ok(ws_d, True, Fn.BF16)
    out, saved = Fn.simnn_gen_forward(noise, ws_d, bn_d, False, Fn.F32)
    assert saved is not None and len(saved) == 4
    gen.eval()
    gen.compute_dtype = "fp32"
    with torch.no_grad():
        assert torch.equal(gen(noise), out)
    ref = E.chain_eval_ref(noise.cpu(), ws, bns, rounding=False)
    assert float((out.cpu().double() - ref).abs().max()) < 1e-5


def test_checkpoint_fixture_and_sample_matrices(tmp_path):
    sd, noise, want = E.checkpoint()
    path = str(tmp_path / "gen_100_0.pt")
    torch.save(sd, path)
    out = SIMNN.sample_matrices(path, noise=noise, device=DEV)
    assert out.shape == (3, 1, 20, 20) and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    assert out.stride() == (400, 400, 20, 1)
    ratio = E.check_deviation(out, want, what="sample_matrices from the checkpoint")
    record("simnn_gen_eval_checkpoint", err_over_bound=round(ratio, 4))
    # a module in TRAIN mode: the eval arithmetic all the same, nothing of the module changes
    gen = SIMNN.Generator()
    gen.load_state_dict(sd)
    gen.to(DEV).train()
    before = _module_state(gen)
    out2 = SIMNN.sample_matrices(gen, noise=noise.to(DEV))
    assert torch.equal(out2, out) and _same_state(gen, before) and gen.training and gen.compute_dtype is None
    drawn = SIMNN.sample_matrices(gen, 7)
    assert drawn.shape == (7, 1, 20, 20) and float((drawn - 0.5).abs().max()) < 0.05
    exact = SIMNN.sample_matrices(gen, noise=noise.to(DEV), compute_dtype="fp32")
    assert float((exact.cpu() - want).abs().max()) < 1e-5
    # generate_song passes compute_dtype through
    adj = SIMNN.generate_song(path, device=DEV, compute_dtype="bf16")
    assert adj.shape == (20, 20) and abs(float(adj.mean()) - 0.5) < 0.05


def test_graph_capture_replays_bit_identically():
    ws, bns, noise, ws_d, bn_d, _ = _setup(61, "base", 16, 100)
    cache = {}
    static = noise.to(DEV).view(16, 100, 1, 1).clone()
    Fn.simnn_gen_forward(static, ws_d, bn_d, False, Fn.BF16, cache=cache)       # one eager call: the pack is cached
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured, _ = Fn.simnn_gen_forward(static, ws_d, bn_d, False, Fn.BF16, cache=cache)
    fills = [E.case_noise(16, 100, 100 + k).to(DEV).view(16, 100, 1, 1) for k in range(3)]
    for x in fills:
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, Fn.simnn_gen_forward(x, ws_d, bn_d, False, Fn.BF16, cache=cache)[0])
    E.assert_moves(captured.cpu())


def test_argument_checks():
    ws, bns, noise, ws_d, bn_d, pack = _setup(3, "base", 4, 100)
    x = noise.to(DEV)
    with pytest.raises(ops.GdmError):
        ops.simnn_gen_eval(torch.zeros(0, 100, device=DEV), pack, ws_d[3], bn_d)            # B = 0
    with pytest.raises(ops.GdmError):
        ops.simnn_gen_eval(torch.zeros(4, 129, device=DEV), pack, ws_d[3], bn_d)            # noise_dim = 129
    with pytest.raises(ops.GdmError):
        ops.simnn_gen_eval(x.cpu(), pack, ws_d[3], bn_d)                                    # a CPU tensor
    with pytest.raises(ops.GdmError):
        ops.simnn_gen_eval(x, pack, ws_d[3], [tuple(v.cpu() for v in bn) for bn in bn_d])
    big = torch.zeros(pack.numel() + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ops.GdmError, match="alignment"):
        ops.simnn_gen_eval(x, big[8:8 + pack.numel()], ws_d[3], bn_d)                       # a misaligned pack
    out = ops.simnn_gen_eval(x, pack, ws_d[3], bn_d)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
