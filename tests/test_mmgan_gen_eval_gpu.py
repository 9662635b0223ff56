"""GPU: the one-launch eval-mode generators of model 2 (csrc/mmgan_gen_eval.hip) against the float64 chain and bounds
of tests/mmgan_gen_eval_ref.py: every tap per layer from the kernel's own previous tap, the outputs against the
propagated chain bound, at the checkpoints' and the class defaults' geometries and a ragged edge, one and two jobs per
launch, batch sizes around the 16-row tile and beyond the block kernel's 256-row cap."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402

import mmgan_gen_eval_ref as G  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
SENTINEL = -77.25
GUARD = 64


@functools.lru_cache(maxsize=None)
def _device_params(name):
    """(host params, device layers, pack, dims, copies taken before any launch)"""
    params = G.make_params(name)
    layers = [tuple(p[k].to(DEV) for k in ("w",) + G.VEC_NAMES) for p in params]
    nbt = [torch.full((), 5, dtype=torch.long, device=DEV) for _ in params]
    before = [[t.clone() for t in la] for la in layers]
    pack, dims = ops.mmgan_gen_eval_pack(layers, eps=G.EPS)
    return params, layers, pack, dims, before, nbt


@functools.lru_cache(maxsize=None)
def _case(name, B, broadcast=False):
    z, n_in, _n4 = G.GEOMETRIES[name]
    noise, inp = G.make_inputs(B, z, n_in, 31 * B + z, broadcast=broadcast)
    return noise, inp, G.chain_ref(noise, inp, G.make_params(name))


def _guarded(shapes):
    """One sentinel-filled buffer holding a view per shape with GUARD floats before, between and after them."""
    sizes = [s[0] * s[1] for s in shapes]
    total = GUARD + sum(n + GUARD for n in sizes)
    buf = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    views, off = [], GUARD
    for s, n in zip(shapes, sizes):
        views.append(buf[off:off + n].view(s))
        inside[off:off + n] = True
        off += n + GUARD
    return buf, inside, views


def _launch(names, B, *, taps=True, inputs=None):
    """One launch of len(names) jobs.  Returns per job dict(ys, acts, out) (taps) or dict(out) and checks the guards."""
    jobs, guards = [], []
    for i, name in enumerate(names):
        _params, _layers, pack, dims, _before, _nbt = _device_params(name)
        noise, inp = inputs[i] if inputs is not None else _case(name, B)[:2]
        widths = (*G.HIDDEN, dims[4])
        shapes = [(B, dims[4])] + ([(B, n) for n in widths] + [(B, n) for n in G.HIDDEN] if taps else [])
        buf, inside, views = _guarded(shapes)
        job = dict(noise=noise.to(DEV), input=inp.to(DEV), pack=pack, dims=dims, out=views[0])
        if taps:
            job["tap_buffers"] = (views[1:5], views[5:8])
        jobs.append(job)
        guards.append((buf, inside, views))
    res = ops.mmgan_gen_eval(jobs, taps=taps)
    torch.cuda.synchronize()
    got = []
    for name, r, (buf, inside, views) in zip(names, res, guards):
        assert bool((buf[~inside] == SENTINEL).all()), f"{name} B={B}: a guard word was overwritten"
        assert not bool((buf[inside] == SENTINEL).any()), f"{name} B={B}: an output or tap element was not written"
        got.append(dict(out=views[0], ys=views[1:5], acts=views[5:8]) if taps else dict(out=views[0]))
    return got


def _assert_state_untouched(names):
    for name in names:
        _params, layers, _pack, _dims, before, nbt = _device_params(name)
        for la, lb in zip(layers, before):
            for a, b in zip(la, lb):
                assert torch.equal(a, b), f"{name}: a parameter or running statistic changed"
        assert all(int(n.item()) == 5 for n in nbt)


def _check(names, B, got):
    for name, g in zip(names, got):
        noise, inp, chain = _case(name, B)
        what = f"{'+'.join(names)}:{name} B={B}"
        worst = G.check_run(g, noise, inp, G.make_params(name), chain=chain, what=what)
        print(what, {k: round(v, 4) for k, v in worst.items()})
        record("mmgan_gen_eval_vs_float64", case=what, **{k: round(v, 4) for k, v in worst.items()})
        assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", G.GEOMETRIES)
def test_one_job_every_batch_size(name):
    for B in G.BATCHES:
        _check((name,), B, _launch((name,), B))
    _assert_state_untouched((name,))


@pytest.mark.parametrize("pair", G.PAIRS, ids="+".join)
def test_two_jobs_in_one_launch(pair):
    for B in G.BATCHES:
        got = _launch(pair, B)
        _check(pair, B, got)
        if B in (1, G.ROW_TILE + 1, 300):            # a job's bits do not depend on what rides beside it
            for name, g in zip(pair, got):
                alone = _launch((name,), B)[0]
                assert torch.equal(alone["out"], g["out"]) and all(torch.equal(a, b) for a, b in zip(alone["ys"], g["ys"]))
    _assert_state_untouched(pair)


@pytest.mark.parametrize("name", ["g1_checkpoint", "g2_checkpoint", "edge"])
def test_a_rows_bits_depend_on_neither_the_batch_nor_its_position(name):
    noise, inp, _chain = _case(name, 300)
    full = _launch((name,), 300)[0]
    for r in (0, 17, 299):
        one = _launch((name,), 1, inputs=[(noise[r:r + 1], inp[r:r + 1])])[0]
        assert torch.equal(one["out"][0], full["out"][r]), f"row {r}"
        for a, b in zip(one["ys"] + one["acts"], full["ys"] + full["acts"]):
            assert torch.equal(a[0], b[r]), f"row {r}"


@pytest.mark.parametrize("name", ["g1_default", "g2_checkpoint", "edge"])
def test_stride_zero_input_equals_the_row_repeated(name):
    B = 2 * G.ROW_TILE + 1
    noise, inp, _ = _case(name, B, True)
    assert inp.shape[0] == 1
    bro = _launch((name,), B, inputs=[(noise, inp)])[0]
    rep = _launch((name,), B, inputs=[(noise, inp.expand(B, -1).contiguous())])[0]
    for a, b in zip([bro["out"]] + bro["ys"] + bro["acts"], [rep["out"]] + rep["ys"] + rep["acts"]):
        assert torch.equal(a, b)
    G.check_run(bro, noise, inp, G.make_params(name), what=f"{name} broadcast")


@pytest.mark.parametrize("names", [("g1_checkpoint",), ("edge",), G.PAIRS[0]], ids="+".join)
def test_the_instance_without_taps_gives_the_same_outputs(names):
    for B in (1, G.ROW_TILE + 1, 300):
        with_taps = _launch(names, B)
        without = _launch(names, B, taps=False)
        for a, b in zip(with_taps, without):
            assert torch.equal(a["out"], b["out"])


def test_unsupported_geometries_are_refused():
    for dims in ((100, 128, 64, 32, 16), (513, 256, 128, 64, 16)):
        assert not ops.mmgan_gen_eval_supported(*dims)
        g = torch.Generator().manual_seed(1)
        widths = dims
        layers = []
        for K, N in zip(widths[:-1], widths[1:]):
            layers.append(tuple(t.to(DEV) for t in (torch.randn(N, K, generator=g), torch.zeros(N), torch.ones(N),
                                                    torch.zeros(N), torch.zeros(N), torch.ones(N))))
        with pytest.raises(ops.GdmError):
            ops.mmgan_gen_eval_pack(layers)
        z = dims[0] // 2
        job = dict(noise=torch.zeros(4, z, device=DEV), input=torch.zeros(4, dims[0] - z, device=DEV),
                   pack=torch.zeros(1 << 20, dtype=torch.uint8, device=DEV), dims=dims)
        with pytest.raises(ops.GdmError):
            ops.mmgan_gen_eval([job])
    assert ops.mmgan_gen_eval_supported(100, 256, 128, 64, 4096)
