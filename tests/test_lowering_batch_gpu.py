"""GPU: the patch-lowering kernels of csrc/lowering.hip (gdm_im2col, gdm_col2im, gdm_permute_pc, gdm_maxpool2_fwd /
_bwd) against the float64 references of tests/lowering_ref.py, at every geometry the package calls them with and at
the index edges no call site reaches (lowering_ref.IM2COL_GEOMS / COL2IM_GEOMS / PERMUTE_SHAPES / POOL_SHAPES; the CPU
test test_shape_tables_reach_every_regime shows what the tables cover).  Every operand takes each type the ABI accepts.

Conditions.  im2col, permute_pc and maxpool2 (values, idx, routed gradient) are bit-equal to the reference, rounded
once when the destination is bf16; no element is left out of a comparison (the reference sees the same exactly
representable inputs, so ties are not ambiguous).  col2im is held per element to
    |got - ref| <= (taps - 1) 2^-24 sum|terms|        (+ one bf16 rounding of the result for a bf16 destination)
from the reference's own per-element tap count and sum of magnitudes; positions no window covers (taps = 0) are exactly
act(0).  With the sigmoid fused, o (1 - o) E + SIGMOID_ULPS 2^-23 o (lowering_ref.act_bound): no device-library
document states expf's error, so the sigmoid's own error is measured here -- what is left of |got - ref| after the
o (1 - o) E term, in ulps of the result, recorded as "sigmoid_ulps" by helpers.record: at most 0.94 on MI355X;
SIGMOID_ULPS is 4 times that.  The worst err / bound of every case is recorded as "col2im" (the summation bound is
attained: 1.0 without activation, where a two-tap sum rounds at a tie).

The 64-bit-index variant col2im_kernel<int64_t> needs more than 2^31 elements and stays untested.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402
from gan_des_midi_music_gen_amd.ops import BF16, F32  # noqa: E402

import lowering_ref as R  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
DT = {torch.float32: F32, torch.bfloat16: BF16}
TYPES = (torch.float32, torch.bfloat16)
def _kw(g):
    return {k: g[k] for k in ("B", "H", "W", "C", "KH", "KW", "stride", "pad", "OH", "OW")}


def _ops_kw(g):
    return dict(b=g["B"], h=g["H"], w=g["W"], c=g["C"], kh=g["KH"], kw=g["KW"], stride=g["stride"], pad=g["pad"])


@pytest.mark.parametrize("g", R.IM2COL_GEOMS, ids=lambda g: g["name"])
def test_im2col_is_the_reference_bit_for_bit(g):
    fails = []
    x32 = torch.randn(g["B"] * g["H"] * g["W"] * g["C"], generator=torch.Generator().manual_seed(g["H"] * g["C"]))
    for st in TYPES:
        src = x32.to(st)
        ref = R.im2col_ref(src, planar=g["planar"], **_kw(g))
        for ct in TYPES:
            cols, oh, ow = ops.im2col(src.to(DEV), planar=g["planar"], out_dtype=DT[ct], **_ops_kw(g))
            assert (oh, ow) == (g["OH"], g["OW"])
            fails += R.check_bits(cols, R.rnd(ref, ct), what=f"{g['name']} src {st} cols {ct}")
    assert not fails, fails


@pytest.mark.parametrize("g", R.COL2IM_GEOMS, ids=lambda g: g["name"])
def test_col2im_within_its_summation_bound(g):
    fails, worst = [], 0.0
    act, tap_major = g.get("act", R.ACT_NONE), g.get("tap_major", False)
    c32 = torch.randn(g["B"] * g["OH"] * g["OW"], g["C"] * g["KH"] * g["KW"],
                      generator=torch.Generator().manual_seed(g["W"] * g["C"]))
    if act == R.ACT_SIGMOID:
        c32 = c32 * 3                       # reach both tails of the sigmoid
    for ct in TYPES:
        cols = c32.to(ct)
        ref = R.col2im_ref(cols, planar=g["planar"], tap_major=tap_major, act=act, **_kw(g))
        for dt in TYPES:
            got = ops.col2im(cols.to(DEV), oh=g["OH"], ow=g["OW"], out_dtype=DT[dt], planar=g["planar"],
                             tap_major=tap_major, act=act, **_ops_kw(g))
            f, w = R.check_col2im(got, ref, dt, what=f"{g['name']} cols {ct} dst {dt}")
            fails += f
            worst = max(worst, w)
            if act == R.ACT_SIGMOID and dt == torch.float32:      # the sigmoid's own error, in ulps of the result
                o = ref["out"]
                E_pre = (ref["taps"] - 1).clamp_min(0) * R.U * ref["mag"]
                res = ((got.cpu().double().reshape(o.shape) - o).abs() - (o * (1 - o) + E_pre) * E_pre) / (2.0 ** -23 * o)
                record("sigmoid_ulps", case=g["name"], cols=str(ct), ulps=round(float(res.max()), 4))
            none = ref["taps"] == 0
            if bool(none.any()):            # exact zeros before the activation: act(0) bit for bit
                want0 = R.rnd(R.act_ref(torch.zeros(1, dtype=torch.float64), act), dt)
                fails += R.check_bits(got.cpu()[none], want0.expand(int(none.sum())).contiguous(),
                                      what=f"{g['name']} uncovered positions")
    record("col2im", case=g["name"], act=act, worst=round(worst, 4))
    if g["name"].startswith("edge uncovered"):
        assert bool((ref["taps"] == 0).any())
    assert not fails, fails


@pytest.mark.parametrize("B,P,C", R.PERMUTE_SHAPES)
def test_permute_pc_is_the_transpose_bit_for_bit(B, P, C):
    fails = []
    x32 = torch.randn(B, P, C, generator=torch.Generator().manual_seed(P + C))
    for st in TYPES:
        src = x32.to(st)
        for dt in TYPES:
            got = ops.permute_pc(src.to(DEV), B, P, C, out_dtype=DT[dt])
            fails += R.check_bits(got, R.permute_ref(src, B, P, C, dt), what=f"({B},{P},{C}) {st} -> {dt}")
    assert not fails, fails


@pytest.mark.parametrize("B,H,W,C", R.POOL_SHAPES)
@pytest.mark.parametrize("dtype", TYPES, ids=str)
def test_maxpool2_forward_and_backward_exact(B, H, W, C, dtype):
    x = R.pool_input(B, H, W, C, dtype)
    v, idx = R.maxpool2_ref(x, B, H, W, C)
    out, got_idx = ops.maxpool2_fwd(x.to(DEV).reshape(-1, C), B, H, W, C)
    fails = R.check_bits(out, R.rnd(v, dtype).reshape(-1, C), what="values")
    fails += R.check_bits(got_idx, idx.reshape(-1, C), what="idx")
    out2, none = ops.maxpool2_fwd(x.to(DEV).reshape(-1, C), B, H, W, C, want_idx=False)
    assert none is None
    fails += R.check_bits(out2, out, what="values without idx")
    d = torch.randn(B * (H // 2) * (W // 2), C, generator=torch.Generator().manual_seed(H)).to(dtype)
    dx = ops.maxpool2_bwd(d.to(DEV), got_idx, B, H, W, C)
    want = R.rnd(R.maxpool2_bwd_ref(d, idx, B, H, W, C), dtype).reshape(-1, C)
    fails += R.check_bits(dx, want, what="routed gradient")
    if H % 2:
        assert float(dx.float().reshape(B, H, W, C)[:, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(dx.float().reshape(B, H, W, C)[:, :, W - 1].abs().max()) == 0.0
    assert not fails, fails
