"""GPU: the 16-byte paths of the transposing Adam tile (csrc/adam_pc.h) -- the contiguous gradient gather, the
contiguous operand-copy store and the software-pipelined p / m / v loads -- for both kernels built on it
(gdm_simnn_adam_step, gdm_adam_step_dev_pc) and both operand-copy types.

A tile takes the wide gather and store when C == 32, it is full in p, and the gradient and the operand copy are
16-byte aligned; it takes the 16-byte p / m / v accesses when P % 4 == 0, p / m / v are aligned and it is full both
ways.  Every case therefore runs the same values through four placements -- everything aligned; everything one element
off (the scalar gather, update and scatter); only the gradient and the operand copy off; only p / m / v off -- and all
four must agree bit for bit in p, m, v and the operand copy (the one-launch step: also in the small range, conv2's
packed images and `hyper`).  Two consecutive launches per case, so both slots of the bias-correction record are read and
the pipelined loop runs from the kernel's own state.

The aligned run of every launch is also held to adam_fused_ref.pc_step_ref (float64, lowering_ref.adam_ref's bounds; the
operand copy bit-equal to the rounded parameter), one reference per (shape, step) shared by every case that starts from
the same bits.  No tolerance is introduced here.

test_every_element_lands_at_its_own_place: a gradient that encodes (n, p, c) with beta1 = 0, so the updated m IS the
gradient: exact equality element by element, which a permutation inside the tile would break.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402

import adam_fused_ref as A  # noqa: E402
import lowering_ref as R  # noqa: E402

DEV = "cuda"
TYPES = (torch.bfloat16, torch.float32)
# (N, C, P): two full tiles per row; one full tile; a full and a partial tile in one launch; C != 32 (fallback);
# ty = 2 with one full and one half c-tile; the production row geometry
SHAPES = [(3, 32, 256), (3, 32, 128), (2, 32, 132), (2, 16, 128), (2, 48, 128), (1, 32, 2048)]
# placement -> (p / m / v one element off, gradient and operand copy one element off)
PLACEMENTS = {"aligned": (0, 0), "all off": (1, 1), "g, copy off": (0, 1), "p, m, v off": (1, 0)}
HP = A.hyper32(2e-5, (0.5, 0.999), A.EPS, 0.125)
NS, W2_OFF = A.SMALL_DEFAULT[:2]
LAUNCHES = 2


def _placed(src, off, dtype=torch.float32):
    """a contiguous device view holding src, `off` elements behind a 16-byte boundary"""
    buf = torch.zeros(src.numel() + 8, dtype=dtype, device=DEV)
    view = buf[off:off + src.numel()]
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    view.copy_(src.reshape(-1))
    return view


_inputs = {}


def _values(shape):
    """start state, the gradients of every launch ((N, P, C) order) and the small range's, one set per shape"""
    if shape not in _inputs:
        N, C, P = shape
        g = torch.Generator().manual_seed(1000 * N + 10 * C + P)
        nb = N * C * P
        v = dict(p=torch.randn(nb, generator=g), m=torch.randn(nb, generator=g) * 1e-3,
                 v=torch.rand(nb, generator=g) * 1e-5 + 1e-12,
                 g=[torch.randn(nb, generator=g) * 10.0 ** -(s + 1) for s in range(LAUNCHES)],
                 ps=torch.randn(NS, generator=g) * 0.1, ms=torch.randn(NS, generator=g) * 1e-3,
                 vs=torch.rand(NS, generator=g) * 1e-5 + 1e-12,
                 gs=[torch.randn(NS, generator=g) * 10.0 ** -(s + 1) for s in range(LAUNCHES)])
        _inputs[shape] = v
    return _inputs[shape]


def _hyper(hp, step=0):
    h = torch.zeros(8)
    h[1:6] = torch.tensor(hp)
    h.view(torch.int32)[0] = step
    return h.to(DEV)


def _run(entry, shape, dtype, placement, hp=HP, values=None):
    """LAUNCHES steps; returns the state after each launch (host copies)"""
    N, C, P = shape
    val = values or _values(shape)
    off_pmv, off_g = PLACEMENTS[placement]
    p, m, v = (_placed(val[k], off_pmv) for k in "pmv")
    shadow = _placed(torch.zeros(N * C * P), off_g, dtype)
    hyper = _hyper(hp)
    if entry == "step":
        ps, ms, vs = (_placed(val[k], 0) for k in ("ps", "ms", "vs"))
        pack = torch.zeros(A.pack_elems(dtype) * shadow.element_size(), dtype=torch.uint8, device=DEV)
        rec = torch.zeros(A.REC_INTS, dtype=torch.int32, device=DEV)
    states = []
    for s in range(LAUNCHES):
        g = _placed(val["g"][s], off_g)
        if entry == "step":
            ops.simnn_adam_step(p, g, m, v, N, C, P, shadow, ps, _placed(val["gs"][s], 0), ms, vs,
                                ps[W2_OFF:W2_OFF + A.W2_ELEMS], pack, hyper, rec)
        else:
            ops.adam_step_dev_pc(p, g, m, v, N, C, P, shadow, hyper, advance_step=True)
        torch.cuda.synchronize()
        st = dict(p=p, m=m, v=v, shadow=shadow, hyper=hyper)
        if entry == "step":
            st.update(ps=ps, ms=ms, vs=vs, pack=pack)
        states.append({k: t.cpu().clone() for k, t in st.items()})
    return states


_refs = {}


def _ref(shape, step, dtype, before, g_pc):
    """pc_step_ref of this launch; shared by the cases whose state before the launch has the same bits"""
    key = (shape, step, dtype)
    if key in _refs and all(torch.equal(R.bits(_refs[key][0][k]), R.bits(before[k])) for k in "pmv"):
        return _refs[key][1]
    N, C, P = shape
    ref = A.pc_step_ref(before["p"], g_pc, before["m"], before["v"], N, C, P, step, HP, dtype)
    _refs[key] = (before, ref)
    return ref


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("entry", ["step", "pc"])
def test_wide_paths_equal_the_fallback_and_float64(entry, shape, dtype):
    N, C, P = shape
    val = _values(shape)
    runs = {pl: _run(entry, shape, dtype, pl) for pl in PLACEMENTS}
    fails = []
    for s in range(LAUNCHES):
        what = f"{entry} {shape} {dtype} launch {s + 1}"
        got = runs["aligned"][s]
        for pl in PLACEMENTS:
            for k, t in runs[pl][s].items():
                if not torch.equal(R.bits(t), R.bits(got[k])):
                    fails.append(f"{what}: {k} of placement '{pl}' differs from the aligned run's in "
                                 f"{int((R.bits(t) != R.bits(got[k])).sum())} element(s)")
        before = runs["aligned"][s - 1] if s else {k: val[k] for k in "pmv"}
        ref = _ref(shape, s + 1, dtype, {k: before[k] for k in "pmv"}, val["g"][s])
        f, worst = A.check_pc(got, ref, what=what)
        print(what, {k: round(x, 4) for k, x in worst.items()})
        fails += f
        if int(got["hyper"].view(torch.int32)[0]) != s + 1:
            fails.append(f"{what}: device step counter {int(got['hyper'].view(torch.int32)[0])}")
    assert not fails, fails[:8]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("entry", ["step", "pc"])
def test_every_element_lands_at_its_own_place(entry, shape, dtype):
    """g[n, p, c] = n 2^20 + p 2^6 + c (exact in fp32: below 2^22), beta1 = 0, grad_scale = 1: m' = g bit for bit, so
    m'[n, c, p] names the place it was gathered from; the operand copy must be rnd(p') at [n, p, c]."""
    N, C, P = shape
    n, p, c = torch.meshgrid(torch.arange(N), torch.arange(P), torch.arange(C), indexing="ij")
    g_pc = (n * 2 ** 20 + p * 2 ** 6 + c).float().reshape(-1)
    val = dict(_values(shape), g=[g_pc] * LAUNCHES)
    hp = A.hyper32(2e-5, (0.0, 0.999), A.EPS, 1.0)
    want_m = g_pc.view(N, P, C).permute(0, 2, 1).contiguous().view(-1)
    fails = []
    for pl in ("aligned", "all off"):
        for s, st in enumerate(_run(entry, shape, dtype, pl, hp=hp, values=val)):
            what = f"{entry} {shape} {dtype} '{pl}' launch {s + 1}"
            fails += R.check_bits(st["m"], want_m, what=f"{what} m")
            want = R.rnd(st["p"].view(N, C, P), dtype).permute(0, 2, 1).contiguous().view(-1)
            fails += R.check_bits(st["shadow"], want, what=f"{what} operand copy")
    assert not fails, fails[:8]
