"""CPU: the float64 eval-mode references of tests/simnn_gen_eval_ref.py.  The chain reference without rounding is
torch.nn's generator in eval mode, it reproduces the committed checkpoint fixture, the calibrated parameters move the
output in every case of the GPU table, each injected fault fails the check the GPU test applies, and the host side of
gdm_simnn_gen_eval refuses bad arguments before any launch."""
import ctypes

import pytest
import torch

from oracle import simnn as osn

import simnn_gen_eval_ref as E
import simnn_gen_ref as R


def _oracle_generator(ws, bns, noise_dim=100):
    gen = osn.Generator(noise_dim=noise_dim).double().eval()
    with torch.no_grad():
        for m, w in zip((gen.conv1, gen.conv2, gen.conv3, gen.conv4), ws):
            m.weight.copy_(w.double())
        for m, (g, be, rm, rv, nbt) in zip((gen.batch_norm1, gen.batch_norm2, gen.batch_norm3), bns):
            m.weight.copy_(g.double()), m.bias.copy_(be.double())
            m.running_mean.copy_(rm.double()), m.running_var.copy_(rv.double()), m.num_batches_tracked.fill_(int(nbt))
    return gen


# ------------------------------------------------------------------------------------------------- faithfulness
@pytest.mark.parametrize("B,noise_dim", [(1, 100), (5, 37), (17, 128)])
def test_chain_reference_without_rounding_is_torch_nn_in_eval_mode(B, noise_dim):
    ws, bns = E.calibrated_params(3, noise_dim=noise_dim)
    noise = E.case_noise(B, noise_dim, B)
    gen = _oracle_generator(ws, bns, noise_dim)
    with torch.no_grad():
        want = gen(noise.double().view(B, noise_dim, 1, 1))
    assert not gen.training and all(int(m.num_batches_tracked) == int(bn[4]) for m, bn in
                                    zip((gen.batch_norm1, gen.batch_norm2, gen.batch_norm3), bns))
    torch.testing.assert_close(E.chain_eval_ref(noise, ws, bns, rounding=False), want, rtol=1e-12, atol=1e-14)


def test_chain_reference_reproduces_the_checkpoint_fixture():
    """The fixture's eval output (fp32 torch.nn) against the float64 chain: without rounding to fp32 accuracy, with the
    bf16 rounding points within the deviation bound the GPU test uses (5.7e-3 of max |want - 0.5| measured: a factor 3.5
    inside 2e-2)."""
    sd, noise, want = E.checkpoint()
    ws, bns = E.checkpoint_params(sd)
    assert float((want - 0.5).abs().max()) < 3e-3, "the fixture's output barely moves: why it is compared on the deviation"
    torch.testing.assert_close(E.chain_eval_ref(noise, ws, bns, rounding=False), want.double(), rtol=0, atol=2e-7)
    ratio = E.check_deviation(E.chain_eval_ref(noise, ws, bns), want, what="chain reference with rounding")
    assert ratio < 0.5


# ------------------------------------------------------------------------------------------- the inputs move
@pytest.mark.parametrize("noise_dim", E.NOISE_DIMS)
def test_calibrated_parameters_move_the_output(noise_dim):
    for B in E.BATCHES:
        ws, bns = E.calibrated_params(1000 * noise_dim + B, noise_dim=noise_dim)
        ref = E.chain_eval_ref(E.case_noise(B, noise_dim, B), ws, bns)
        E.assert_moves(ref, f"noise_dim={noise_dim} B={B}")


def test_families():
    ws, bns = E.calibrated_params(5, "zero")
    assert float(bns[1][3][7]) == 0.0 and float(bns[1][2][7]) == 0.0, "a constant channel: running_var 0"
    inv, _ = E.invstd_ref(bns)
    assert float(inv[128 + 7]) == pytest.approx(1 / R.EPS ** 0.5)
    ws, bns = E.calibrated_params(6, "saturate")
    ref = E.chain_eval_ref(E.case_noise(16, 100, 1), ws, bns)
    assert float(ref.min()) < 1e-6 and float(ref.max()) > 1 - 1e-6


# ------------------------------------------------------------------------------------------------ fault detection
def _emulated_kernel(noise, ws, bns):
    """Every op's float64 reference rounded to fp32 standing in for the kernel: what check_layers sees on the GPU."""
    B = noise.shape[0]
    y1 = R.first_ref(noise, ws[0])[0].float()
    inv = E.invstd_ref(bns)[0].float()
    i1, i2, i3 = torch.split(inv, [128, 64, 32])
    y2 = R.convt_ref(y1, bns[0][2], i1, bns[0][0], bns[0][1], ws[1], 2, B)[0].float()
    y3 = R.convt_ref(y2, bns[1][2], i2, bns[1][0], bns[1][1], ws[2], 3, B)[0].float()
    out = R.last_ref(y3, bns[2][2], i3, bns[2][0], bns[2][1], ws[3], B)[0].float()
    return out, y1, y2, y3, inv


@pytest.fixture(scope="module")
def case():
    B = 9
    ws, bns = E.calibrated_params(11)
    noise = E.case_noise(B, 100, 4)
    ref = E.chain_eval_ref(noise, ws, bns)
    E.assert_moves(ref)
    return dict(B=B, ws=ws, bns=bns, noise=noise, ref=ref, emu=_emulated_kernel(noise, ws, bns))


def test_the_emulated_kernel_passes_every_check(case):
    out = case["emu"][0]
    worst = E.check_layers(case["noise"], case["ws"], case["bns"], *case["emu"])
    assert max(worst.values()) <= 1.0
    rl2 = E.check_chain(out, case["ref"])
    assert rl2 < R.CHAIN_RELL2 / 3, rl2       # fp32 accumulation against float64 on identical rounding points


FAULTS = ["no_eps", "swap_mean_beta", "batch_stats", "no_relu", "const_half"]


@pytest.mark.parametrize("fault", FAULTS)
def test_chain_check_flags_fault(case, fault):
    """The whole-chain check of the GPU test (rel-L2 <= CHAIN_RELL2) fails for: running variance used without eps,
    running mean and beta swapped, batch statistics in place of the running ones, ReLU dropped, output == 0.5."""
    bad = E.chain_eval_ref(case["noise"], case["ws"], case["bns"], faults=(fault,))
    with pytest.raises(E.CheckError):
        E.check_chain(bad.float(), case["ref"], what=fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_checkpoint_deviation_check_flags_fault(fault):
    """The same faults against the checkpoint fixture's deviation bound (max |out - want| <= 2e-2 max |want - 0.5|)."""
    sd, noise, want = E.checkpoint()
    ws, bns = E.checkpoint_params(sd)
    bad = E.chain_eval_ref(noise, ws, bns, faults=(fault,))
    with pytest.raises(E.CheckError):
        E.check_deviation(bad.float(), want, what=fault)


def test_layer_checks_flag_faults(case):
    """Per-layer checks on the taps: invstd without eps (the zero family's constant channel makes it infinite; on the
    base family it is off by eps / (2 var) >> 4 u), a tap of layer 2 computed without ReLU, running mean and beta
    swapped in layer 3's staging, a bf16-staged layer 4."""
    noise, ws, bns, B = case["noise"], case["ws"], case["bns"], case["B"]
    out, y1, y2, y3, inv = case["emu"]
    bad_inv = torch.cat([1.0 / torch.sqrt(bn[3].double()) for bn in bns]).float()
    with pytest.raises(E.CheckError, match="invstd"):
        E.check_layers(noise, ws, bns, out, y1, y2, y3, bad_inv)
    i1, i2, i3 = torch.split(inv, [128, 64, 32])
    bad_y2 = R.convt_ref(y1, bns[0][2], i1, bns[0][0], bns[0][1], ws[1], 2, B, faults=("no_relu",))[0].float()
    with pytest.raises(E.CheckError, match="layer 2"):
        E.check_layers(noise, ws, bns, out, y1, bad_y2, y3, inv)
    bad_y3 = R.convt_ref(y2, bns[1][1], i2, bns[1][0], bns[1][2], ws[2], 3, B)[0].float()
    with pytest.raises(E.CheckError, match="layer 3"):
        E.check_layers(noise, ws, bns, out, y1, y2, bad_y3, inv)
    bad_out = R.last_ref(y3, bns[2][2], i3, bns[2][0], bns[2][1], ws[3], B, faults=("bf16_input",))[0].float()
    with pytest.raises(E.CheckError, match="layer 4"):
        E.check_layers(noise, ws, bns, bad_out, y1, y2, y3, inv)
    with pytest.raises(E.CheckError, match="layer 4"):
        E.check_layers(noise, ws, bns, torch.full_like(out, 0.5), y1, y2, y3, inv)


# ----------------------------------------------------------------------------------------------- the ABI (host)
@pytest.fixture(scope="module")
def lib():
    from gan_des_midi_music_gen_amd import _lib, build
    build.build()
    return _lib.load()


def test_ops_wrapper_exists_and_refuses_cpu_tensors(lib):
    from gan_des_midi_music_gen_amd import ops
    ws, bns = E.calibrated_params(1)
    pack = torch.zeros(lib.gdm_simnn_gen_pack_bytes(), dtype=torch.uint8)
    with pytest.raises(ops.GdmError):
        ops.simnn_gen_eval(torch.zeros(2, 100), pack, ws[3], bns)


def test_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """B = 0, noise_dim 0 and 129, a null pointer, a misaligned pack / out / tap: GDM_EINVAL on the host.  Without a GPU
    the pointers are placeholders (nothing is launched either way)."""
    P = ctypes.c_void_p
    if torch.cuda.is_available():
        keep = [torch.zeros(1 << 20, device="cuda") for _ in range(5)] + [torch.zeros(128, device="cuda") for _ in range(12)]
        ptrs = [t.data_ptr() for t in keep]
    else:
        ptrs = [4096 * (i + 1) for i in range(17)]
    noise, pack, w4, out, tap = ptrs[:5]
    vecs = [P(v) for v in ptrs[5:]]

    def call(noise=noise, B=4, nd=100, pack=pack, w4=w4, out=out, taps=(None, None, None, None)):
        return lib.gdm_simnn_gen_eval(P(noise), B, nd, P(pack), P(w4), *vecs, 1e-5, P(out), *[P(t) if t else None for t in taps],
                                      None)
    for kw in (dict(B=0), dict(B=-3), dict(nd=0), dict(nd=129), dict(noise=None), dict(pack=None), dict(w4=None),
               dict(out=None), dict(pack=pack + 8), dict(out=out + 4), dict(taps=(tap + 4, None, None, None)),
               dict(taps=(None, None, tap + 8, None))):
        assert call(**kw) == -1 and b"gdm_simnn_gen_eval" in lib.gdm_last_error(), kw
