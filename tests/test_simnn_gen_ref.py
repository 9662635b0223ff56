"""CPU: the float64 references of tests/simnn_gen_ref.py.  They are faithful to oracle.simnn.Generator, the batch table
of tests/test_simnn_gen_batch_gpu.py reaches every regime of the fused generator, the checkers flag each injected fault
at the bounds the GPU tests use, and the host-side ABI agrees with the mirrors (no compute calls)."""
import copy

import pytest
import torch

from oracle import simnn as osn

import simnn_gen_ref as R


def _params(seed, noise_dim=100, gamma_spread=0.5):
    """weights at the reference's init scale, gamma in 1 +- gamma_spread, beta in +-0.5, non-default running stats"""
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(noise_dim, 128, 4, 4, generator=g) * 0.02, torch.randn(128, 64, 4, 4, generator=g) * 0.02,
          torch.randn(64, 32, 4, 4, generator=g) * 0.02, torch.randn(32, 1, 5, 5, generator=g) * 0.05]
    bns = []
    for c in (128, 64, 32):
        bns.append((1 + gamma_spread * (2 * torch.rand(c, generator=g) - 1), 0.5 * (2 * torch.rand(c, generator=g) - 1),
                    torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, torch.tensor(3)))
    return ws, bns


def _noise(B, noise_dim=100, seed=0):
    return torch.randn(B, noise_dim, generator=torch.Generator().manual_seed(seed))


def _emulated_chain(B, seed=0):
    """The fused chain on the CPU with each op's float64 reference rounded to fp32 standing in for the kernel: the
    inputs every per-op check of the GPU test sees, op by op."""
    ws, bns = _params(seed)
    c = dict(ws=ws, bns=bns, noise=_noise(B, seed=seed), B=B)
    c["y1"] = R.first_ref(c["noise"], ws[0])[0].float()
    ys = {1: c["y1"]}
    for layer in (1, 2, 3):
        g, be, rm, rv, nbt = bns[layer - 1]
        st = R.stats_ref(ys[layer], layer, B, rm, rv, nbt)
        c[f"st{layer}"] = st
        mean, inv = st["mean"][0].float(), st["invstd"][0].float()
        c[f"mi{layer}"] = (mean, inv)
        if layer < 3:
            ys[layer + 1] = R.convt_ref(ys[layer], mean, inv, g, be, ws[layer], layer + 1, B)[0].float()
            c[f"y{layer + 1}"] = ys[layer + 1]
    return c


# ------------------------------------------------------------------------------------------------- faithfulness
@pytest.mark.parametrize("B", [2, 5, 257])
def test_chain_reference_without_rounding_is_the_oracle_generator(B):
    ws, bns = _params(1)
    noise = _noise(B, seed=B)
    gen = osn.Generator().double().train()
    with torch.no_grad():
        for m, w in zip((gen.conv1, gen.conv2, gen.conv3, gen.conv4), ws):
            m.weight.copy_(w.double())
        for m, (g, be, rm, rv, nbt) in zip((gen.batch_norm1, gen.batch_norm2, gen.batch_norm3), bns):
            m.weight.copy_(g.double()), m.bias.copy_(be.double())
            m.running_mean.copy_(rm.double()), m.running_var.copy_(rv.double()), m.num_batches_tracked.fill_(int(nbt))
        want = gen(noise.double().view(B, 100, 1, 1))
    out, stats = R.chain_ref(noise, ws, bns, rounding=False)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-14)
    for m, (rm, rv, nbt) in zip((gen.batch_norm1, gen.batch_norm2, gen.batch_norm3), stats):
        torch.testing.assert_close(rm, m.running_mean, rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(rv, m.running_var, rtol=1e-12, atol=1e-14)
        assert nbt == int(m.num_batches_tracked) == 4


def test_chain_reference_rounding_points_are_the_per_op_references():
    """chain_ref's rounding model is the per-op references' composed: its layer-1 output and its running statistics
    of layer 1 match the per-op path (layer 1 has no staged operand, so the two agree to float64 rounding)."""
    B = 5
    c = _emulated_chain(B)
    out, stats = R.chain_ref(c["noise"], c["ws"], c["bns"])
    y1, _ = R.first_ref(c["noise"], c["ws"][0])
    st = R.stats_ref(y1, 1, B, *c["bns"][0][2:])
    torch.testing.assert_close(stats[0][0], st["running_mean"][0], rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(stats[0][1], st["running_var"][0], rtol=1e-12, atol=1e-14)
    assert out.shape == (B, 1, 20, 20) and stats[2][2] == 4


# ------------------------------------------------------------------------------------------------- regime table
def test_batch_table_reaches_every_regime():
    got = {B: R.regimes(B) for B in R.BATCHES}
    assert {g["tail2"] for g in got.values()} == set(range(8)), "every tail size of the 8-sample workgroups"
    assert {g["tail3"] for g in got.values()} == set(range(4)), "every tail size of the 4-sample workgroups"
    assert {g["rounds2"] for g in got.values()} == {1, 2}
    assert {g["rounds3"] for g in got.values()} == {1, 2, 3, 4}
    assert got[128]["rounds3"] == 1 and got[129]["rounds3"] == 2 and got[257]["rounds3"] == 3
    assert got[256]["rounds2"] == 1 and got[257]["rounds2"] == 2
    assert got[256]["first"] == "gen_first" and got[257]["first"] == "fallback"
    assert R.bn_row_chunks(16 * 512) == 32 and R.bn_row_chunks(16 * 257) == 17
    staging = {R.regimes(16, nd)["staging"] for nd in R.NOISE_DIMS} | {R.regimes(16, 100, aligned=False)["staging"]}
    assert staging == {"vector", "scalar"}
    assert all(R.regimes(16, nd, al)["staging"] == "scalar" for nd, al in ((37, True), (1, True), (100, False)))


def test_chunk_of_rows_matches_the_partial_layout():
    """stats_ref's chunk map and partials_ref's loop order agree: counting rows per chunk gives the partials' n."""
    for layer, B in ((2, 13), (3, 130)):
        k = R.chunk_of_rows(layer, B)
        y = torch.randn(B * R.GEOM[layer][1] ** 2, R.GEOM[layer][2])
        n = R.partials_ref(y, layer, B)["n"][0]
        assert len(n) == R.convt_chunks(layer, B)
        assert torch.equal(torch.bincount(k, minlength=len(n)).double(), n)


# ----------------------------------------------------------------------------------------------- the ABI (host)
@pytest.fixture(scope="module")
def lib():
    from gan_des_midi_music_gen_amd import _lib, build
    build.build()
    return _lib.load()


def test_convt_chunks_entry_point_matches_the_mirror(lib):
    for B in list(range(1, 600)) + [1024]:
        for layer in (2, 3):
            assert lib.gdm_simnn_gen_convt_chunks(layer, B) == R.convt_chunks(layer, B), (layer, B)


def test_gen_first_refuses_batches_and_noise_dims_it_cannot_hold(lib):
    """gdm_simnn_gen_first owns the whole batch in one workgroup (B <= 256) and stages K <= 128: it refuses B = 1,
    B = 257, noise_dim 0 and 129 on the host.  Without a GPU the pointers are placeholders (nothing is launched
    either way); with one they are real buffers large enough for any of these calls."""
    if torch.cuda.is_available():
        keep = [torch.zeros(n, device="cuda") for n in (257 * 129, 1 << 20, 257 * 16 * 128, 128, 128, 128, 128)]
        keep.append(torch.zeros(1, dtype=torch.long, device="cuda"))
        noise, pack, y1, rm, rv, sm, si, nbt = (t.data_ptr() for t in keep)
    else:
        noise, pack, y1, rm, rv, sm, si, nbt = (4096 * (i + 1) for i in range(8))
    for B, nd in ((1, 100), (257, 100), (16, 0), (16, 129), (0, 100)):
        rc = lib.gdm_simnn_gen_first(noise, B, nd, pack, y1, 0.1, 1e-5, rm, rv, nbt, sm, si, None)
        assert rc == -1 and b"gdm_simnn_gen_first" in lib.gdm_last_error(), (B, nd)
    rc = lib.gdm_simnn_gen_first(None, 16, 100, pack, y1, 0.1, 1e-5, rm, rv, nbt, sm, si, None)
    assert rc == -1 and b"null pointer" in lib.gdm_last_error()


# ------------------------------------------------------------------------------------------------ fault detection
@pytest.fixture(scope="module")
def chains():
    return {B: _emulated_chain(B) for B in (2, 5, 129)}


def _flag_stats(c, layer, faults):
    B = c["B"]
    y = c[f"y{layer}"]
    rm, rv, nbt = c["bns"][layer - 1][2:]
    ref = R.stats_ref(y, layer, B, rm, rv, nbt)
    bad = R.stats_ref(y, layer, B, rm, rv, nbt, faults=faults)
    got = {k: ref[k][0] for k in ("mean", "invstd", "running_mean", "running_var")}
    got["num_batches_tracked"] = ref["num_batches_tracked"]
    R.check_stats(got, ref, layer)                                      # the reference passes its own check
    with pytest.raises(R.CheckError):
        R.check_stats({**{k: bad[k][0] for k in ("mean", "invstd", "running_mean", "running_var")},
                       "num_batches_tracked": bad["num_batches_tracked"]}, ref, layer, what=str(faults))


def _flag_convt(c, layer, faults):
    B = c["B"]
    g, be = c["bns"][layer - 2][:2]
    args = (c[f"y{layer - 1}"], *c[f"mi{layer - 1}"], g, be, c["ws"][layer - 1], layer, B)
    ref, _, E = R.convt_ref(*args)
    bad = R.convt_ref(*args, faults=faults)[0]
    R.check_abs(ref, ref, E)
    with pytest.raises(R.CheckError):
        R.check_abs(bad, ref, E, what=str(faults), where=R.where_convt(layer, B))


STATS_FAULTS = [  # (B, layer, fault)
    (2, 1, "biased_var"), (2, 2, "biased_var"), (2, 3, "biased_var"), (5, 1, "drop_last"), (5, 2, "drop_last"),
    (5, 3, "drop_last"), (129, 3, ("chunk_twice", 127)), (129, 3, ("chunk_twice", 128)), (2, 1, "momentum_swap"),
    (2, 3, "momentum_swap"), (2, 2, ("nbt", 0)), (2, 2, ("nbt", 2)),
]


@pytest.mark.parametrize("B,layer,fault", STATS_FAULTS, ids=lambda v: str(v))
def test_stats_checker_flags_fault(chains, B, layer, fault):
    """Batch-statistics faults: biased running variance (layer 1 in gen_l1_kernel, layers 2/3 in bn_finalize), the last
    sample left out, a chunk counted twice either side of bn_finalize's round boundary (128 chunks: layer 3 at
    B = 129 has 132), swapped momentum weights, num_batches_tracked advanced 0 or 2 times."""
    _flag_stats(chains[B], layer, (fault,))


CONVT_FAULTS = [(2, 2, "no_relu"), (2, 3, "no_relu"), (2, 2, "no_gamma"), (5, 3, "no_gamma"), (2, 2, "wrong_tap"),
                (5, 3, "wrong_tap"), (2, 2, "no_halo"), (5, 3, "no_halo")]


@pytest.mark.parametrize("B,layer,fault", CONVT_FAULTS, ids=lambda v: str(v))
def test_convt_checker_flags_fault(chains, B, layer, fault):
    """Layer 2 / 3 faults: ReLU missing on load, gamma dropped from the scale (gamma in 1 +- 0.5), class (0, 0) reading
    kh = qy + 2a, no zero halo between samples."""
    _flag_convt(chains[B], layer, (fault,))


@pytest.mark.parametrize("B,layer", [(5, 2), (5, 3), (129, 3)])
def test_partials_checker_flags_a_tail_that_counts_its_padding(chains, B, layer):
    c = chains[B]
    y = c[f"y{layer}"]
    ref = R.partials_ref(y, layer, B)
    part = torch.stack([ref["n"][0][:, None].expand_as(ref["mean"][0]), ref["mean"][0], ref["m2"][0]], -1)
    R.check_partials(part, ref, layer, B)
    bad = R.partials_ref(y, layer, B, faults=("tail_pad_n",))
    part = torch.stack([bad["n"][0][:, None].expand_as(bad["mean"][0]), bad["mean"][0], bad["m2"][0]], -1)
    with pytest.raises(R.CheckError, match="chunk"):
        R.check_partials(part, ref, layer, B)


def test_last_checker_flags_a_bf16_input(chains):
    c = chains[2]
    g, be = c["bns"][2][:2]
    y3 = R.convt_ref(c["y2"], *c["mi2"], *c["bns"][1][:2], c["ws"][2], 3, 2)[0].float()
    st = R.stats_ref(y3, 3, 2, *c["bns"][2][2:])
    args = (y3, st["mean"][0].float(), st["invstd"][0].float(), g, be, c["ws"][3], 2)
    ref, E = R.last_ref(*args)
    bad, _ = R.last_ref(*args, faults=("bf16_input",))
    R.check_abs(ref, ref, E)
    with pytest.raises(R.CheckError):
        R.check_abs(bad, ref, E, what="bf16_input", where=R.where_last)


def test_constant_channel_bound_is_exact():
    """A zeroed conv2 output channel: y2's channel is 0 everywhere, M2 = 0 and its bound is 0 (exact)."""
    B = 5
    c = _emulated_chain(B)
    ws = copy.deepcopy(c["ws"])
    ws[1][:, 7] = 0.0
    g, be = c["bns"][0][:2]
    y2 = R.convt_ref(c["y1"], *c["mi1"], g, be, ws[1], 2, B)[0].float()
    assert float(y2[:, 7].abs().max()) == 0.0
    st = R.stats_ref(y2, 2, B, *c["bns"][1][2:])
    assert float(st["mean"][1][7]) == 0.0
    assert float(st["invstd"][0][7]) == pytest.approx(1 / 1e-5 ** 0.5)
    part = R.partials_ref(y2, 2, B)
    assert float(part["m2"][1][:, 7].abs().max()) == 0.0 and float(part["m2"][0][:, 7].abs().max()) == 0.0
