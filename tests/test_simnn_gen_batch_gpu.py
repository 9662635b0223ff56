"""GPU: model 1's fused generator forward (csrc/simnn_gen.hip) op by op against the float64 references of
tests/simnn_gen_ref.py at every batch size of its table, and the whole chain -- directly and inside one
SimnnTrainer.step -- against the float64 chain reference.

Each op runs on the previous kernel's actual output, so every check isolates one kernel: layer 1 (gen_first, or the
bf16 GEMM + gdm_bn_stats for B > 256), convt_s2_bn of layers 2 and 3 with their per-workgroup partials, bn_finalize's
mean / invstd / running statistics / num_batches_tracked, and the last layer.  Every element of every output is held
to its derived bound; helpers.record writes the worst err / bound per op and case.

Families: "base" (gamma in 1 +- 0.5, beta in +-0.5, non-default running statistics), "zero" (conv2's output channel
7 zeroed: a constant channel, var = 0, whose M2 must come out exactly 0), "saturate" (conv4 x 40: the sigmoid
saturates at both ends).  The float64 work of the file is about 20 GMAC (the layer-2 and layer-3 references and their
magnitudes over the table): budget 60 s on 16 threads; the whole file measured 5 s of wall time on MI355X.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import SIMNN, functional as Fn, ops, synthetic  # noqa: E402
from gan_des_midi_music_gen_amd.train import SimnnTrainer  # noqa: E402

import simnn_gen_ref as R  # noqa: E402
from helpers import record, rel_l2  # noqa: E402

DEV = "cuda"
FAMILY_BATCHES = {"base": R.BATCHES, "zero": [5, 129, 260], "saturate": [16, 257]}
CASES = [(f, B) for f, bs in FAMILY_BATCHES.items() for B in bs]
ZERO_CH = 7


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _params(seed, family="base", noise_dim=100):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(noise_dim, 128, 4, 4, generator=g) * 0.02, torch.randn(128, 64, 4, 4, generator=g) * 0.02,
          torch.randn(64, 32, 4, 4, generator=g) * 0.02, torch.randn(32, 1, 5, 5, generator=g) * 0.05]
    if family == "zero":
        ws[1][:, ZERO_CH] = 0.0
    if family == "saturate":
        ws[3] *= 40.0
    bns = [(1 + 0.5 * (2 * torch.rand(c, generator=g) - 1), 0.5 * (2 * torch.rand(c, generator=g) - 1),
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, torch.tensor(3))
           for c in (128, 64, 32)]
    return ws, bns


def _dev_bns(bns):
    return [(g.to(DEV), be.to(DEV), rm.to(DEV).clone(), rv.to(DEV).clone(), nbt.to(DEV).clone())
            for g, be, rm, rv, nbt in bns]


def _first(noise, ws_d, pack, bn_d, B):
    rm, rv, nbt = bn_d[2:]
    if B <= 256:
        return ops.simnn_gen_first(noise, pack, rm, rv, nbt)
    y1 = Fn.convT_forward(noise, ws_d[0], B, 1, 1, 1, 0, Fn.BF16)[0]
    return (y1, *ops.bn_stats(y1, rm, rv, nbt))


def _stats_got(mean, invstd, bn_d):
    return dict(mean=mean, invstd=invstd, running_mean=bn_d[2], running_var=bn_d[3],
                num_batches_tracked=int(bn_d[4].item()))


def _check_layer1(noise, ws, bns, ws_d, bn_d, pack, B, what):
    y1, mean, inv = _first(noise, ws_d, pack, bn_d[0], B)
    torch.cuda.synchronize()
    ref, M = R.first_ref(noise.cpu(), ws[0])
    worst = {"y1": R.check_elementwise(y1, ref, M, rtol=R.RTOL_L1, out_dtype=torch.float32, where=R.where_l1(B),
                                       what=f"{what} layer 1")}
    st = R.stats_ref(y1, 1, B, *bns[0][2:])
    worst.update({f"l1 {k}": v for k, v in R.check_stats(_stats_got(mean, inv, bn_d[0]), st, 1, what=what).items()})
    return y1, mean, inv, worst


@pytest.mark.parametrize("family,B", CASES, ids=lambda v: str(v))
def test_every_op_against_float64(family, B):
    torch.manual_seed(B)
    ws, bns = _params(B, family)
    noise = torch.randn(B, 100, generator=torch.Generator().manual_seed(1000 + B)).to(DEV)
    ws_d, bn_d = [w.to(DEV) for w in ws], _dev_bns(bns)
    pack = ops.simnn_gen_pack(ws_d[0], ws_d[1], ws_d[2])
    what = f"{family} B={B}"
    y, mean, inv, worst = _check_layer1(noise, ws, bns, ws_d, bn_d, pack, B, what)
    for layer in (2, 3):
        g, be = bn_d[layer - 2][:2]
        yout, part, chunks = ops.simnn_gen_convt_bn(layer, y, mean, inv, g, be, B, pack)
        assert chunks == R.convt_chunks(layer, B)
        _, oh, C = R.GEOM[layer]
        mean2, inv2 = ops.bn_finalize(part, chunks, B * oh * oh, C, *bn_d[layer - 1][2:])
        torch.cuda.synchronize()
        ref, _, E = R.convt_ref(y, mean, inv, g, be, ws[layer - 1], layer, B)
        worst[f"l{layer} out"] = R.check_abs(yout, ref, E, what=f"{what} layer {layer} out",
                                             where=R.where_convt(layer, B))
        pref = R.partials_ref(yout, layer, B)
        worst.update({f"l{layer} partial {k}": v for k, v in R.check_partials(part, pref, layer, B, what=what).items()})
        st = R.stats_ref(yout, layer, B, *bns[layer - 1][2:])
        got = _stats_got(mean2, inv2, bn_d[layer - 1])
        worst.update({f"l{layer} {k}": v for k, v in R.check_stats(got, st, layer, what=what).items()})
        if family == "zero" and layer == 2:
            assert float(yout[:, ZERO_CH].abs().max()) == 0.0
            assert float(part[:, ZERO_CH, 2].abs().max()) == 0.0 and float(mean2[ZERO_CH]) == 0.0
        y, mean, inv = yout, mean2, inv2
    g, be = bn_d[2][:2]
    out = ops.simnn_gen_last(y, mean, inv, g, be, ws_d[3], B)
    torch.cuda.synchronize()
    ref, E = R.last_ref(y, mean, inv, g, be, ws[3], B)
    worst["l4 out"] = R.check_abs(out, ref, E, what=f"{what} layer 4", where=R.where_last)
    if family == "saturate":
        o = out.cpu()
        assert float(o.min()) < 1e-6 and float(o.max()) > 1 - 1e-6, "the family must saturate the sigmoid"
    record("simnn_gen_ops_vs_float64", case=what, **{k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("noise_dim,offset", [(1, 0), (37, 0), (100, 0), (128, 0), (100, 1)], ids=str)
def test_layer1_noise_staging(noise_dim, offset):
    """gen_l1_kernel's vector staging (noise_dim % 4 == 0 and a 16-byte aligned pointer) and its scalar path (any other
    noise_dim, or a noise view 4 bytes into its buffer), at a partial batch tile and a full batch."""
    for B in (13, 256):
        ws, bns = _params(7 + noise_dim, noise_dim=noise_dim)
        buf = torch.randn(B * noise_dim + offset, generator=torch.Generator().manual_seed(B)).to(DEV)
        noise = buf[offset:].view(B, noise_dim)
        assert (noise.data_ptr() % 16 == 0) == (offset == 0)
        ws_d, bn_d = [w.to(DEV) for w in ws], _dev_bns(bns)
        pack = ops.simnn_gen_pack(ws_d[0], ws_d[1], ws_d[2])
        what = f"noise_dim={noise_dim} offset={offset} B={B} ({R.regimes(B, noise_dim, offset == 0)['staging']})"
        worst = _check_layer1(noise, ws, bns, ws_d, bn_d, pack, B, what)[3]
        record("simnn_gen_layer1_staging", case=what, **{k: round(v, 4) for k, v in worst.items()})


def _stat_ratio(got, ref, init):
    """||got - ref|| over its allowance CHAIN_STATS_RELL2 ||blended|| + 4 u (||ref|| + ||blended||), blended = what the
    batch blended into the running statistic: ref - (1 - momentum) init (simnn_gen_ref's docstring)"""
    got, ref, init = (t.detach().double().cpu() for t in (got, ref, init))
    blended = (ref - (1 - R.MOMENTUM) * init).norm()
    allow = R.CHAIN_STATS_RELL2 * blended + 4 * R.U * (ref.norm() + blended)
    return float((got - ref).norm() / allow)


def _check_chain(out, bn_after, ws, bns, noise, what):
    ref, stats = R.chain_ref(noise.cpu(), ws, bns)
    rl2 = rel_l2(out, ref)
    res = {"out": rl2 / R.CHAIN_RELL2}
    for i, ((rm, rv, nbt), (_, _, rm0, rv0, nbt0), (rrm, rrv, rnbt)) in enumerate(zip(bn_after, bns, stats)):
        assert int(nbt) == rnbt == int(nbt0) + 1, (what, i, int(nbt))
        res[f"rm{i + 1}"] = _stat_ratio(rm, rrm, rm0)
        res[f"rv{i + 1}"] = _stat_ratio(rv, rrv, rv0)
    record("simnn_gen_chain_vs_float64", case=what, out_rel_l2=float(f"{rl2:.3g}"),
           **{k: round(v, 4) for k, v in res.items()})
    assert max(res.values()) <= 1.0, (what, "err / bound", res)


@pytest.mark.parametrize("B", [2, 16, 129, 256, 257, 512])
def test_fused_chain_against_float64(B):
    """functional.simnn_gen_forward through the fused route (six launches) against chain_ref: catches wiring mistakes
    between the kernels (statistics of the wrong layer, the wrong row count to bn_finalize)."""
    ws, bns = _params(50 + B)
    noise = torch.randn(B, 100, 1, 1, generator=torch.Generator().manual_seed(B)).to(DEV)
    ws_d, bn_d = [w.to(DEV) for w in ws], _dev_bns(bns)
    assert Fn._gen_fused_ok(noise, ws_d, True, Fn.BF16, False)
    out, saved = Fn.simnn_gen_forward(noise, ws_d, bn_d, True, Fn.BF16, cache={}, need_backward=False)
    torch.cuda.synchronize()
    assert saved is None and out.shape == (B, 1, 20, 20)
    _check_chain(out, [b[2:] for b in bn_d], ws, bns, noise, f"fused chain B={B}")


@pytest.mark.parametrize("b", [256, 16])
def test_trainer_step_generator_state(b):
    """One SimnnTrainer.step at the bench configuration (B = 256, 128 x 256) and at B = 16: last_generated and the
    generator's running statistics against chain_ref, num_batches_tracked == 1 for each BatchNorm."""
    torch.manual_seed(5)
    gen, disc = SIMNN.Generator().apply(SIMNN.weights_init), SIMNN.Discriminator(input_hw=(128, 256))
    disc.apply(SIMNN.weights_init)
    g = gen
    ws = [m.weight.detach().clone() for m in (g.conv1, g.conv2, g.conv3, g.conv4)]
    bns = [(m.weight.detach().clone(), m.bias.detach().clone(), m.running_mean.clone(), m.running_var.clone(),
            m.num_batches_tracked.clone()) for m in (g.batch_norm1, g.batch_norm2, g.batch_norm3)]
    real, fake, noise = synthetic.simnn_inputs(b, (128, 256), seed=99)
    gen.to(DEV).train(), disc.to(DEV).train()
    tr = SimnnTrainer(gen, disc, compute_dtype="bf16")
    tr.step(real.to(DEV), noise.to(DEV), fake.to(DEV))
    torch.cuda.synchronize()
    after = [(m.running_mean, m.running_var, m.num_batches_tracked) for m in (g.batch_norm1, g.batch_norm2,
                                                                               g.batch_norm3)]
    assert all(int(n) == 1 for _, _, n in after)
    _check_chain(tr.last_generated, after, ws, bns, noise, f"trainer step B={b}")
