"""float64 references, code decoders and a per-element checker for model 1's convolution trunk (csrc/simnn_trunk.h and the
simnn_conv*.hip / simnn_slab_sum.hip files it lists).

A plain module next to helpers.py: the GPU tests of tests/test_simnn_trunk_batch_gpu.py and the CPU tests of
tests/test_trunk_plans.py import it.

Every reference runs ONE op in isolation on the kernel's own inputs (its p1, dp1, dp2 and argmax codes; the weights
rounded as the pack rounds them), in float64 with torch on the CPU.  The backward references route gradients through
the kernel's DECODED codes; the codes themselves are checked separately (check_codes) under the tie rule below, so a
near-tie cannot fail a gradient check and a wrong route cannot hide in one.  Each reference also returns a magnitude
M = sum |a_i * b_i| per output element (the same op on |inputs| and |weights|, plus |bias|).

Element bound (check_elementwise):  |got - ref| <= rtol * M + 1/2 ulp_out(|ref| + rtol * M)
  * The kernels accumulate in fp32.  bf16 operands have 8-bit significands, so their products are exact in fp32; an
    fp32 x fp32 product is rounded once.  Any summation order of n terms with fp32 roundings has
    |err| <= n * 2^-24 * sum |terms|  (n = the number of roundings on the longest path to the result, products included).
  * conv1 forward: 4 taps + bias -> n <= 9 -> 5.4e-7.  conv1 input gradient: <= 64 (channel, tap) terms -> 4e-6.
    conv2 forward: 144 products + bias -> 8.6e-6.  Each is held to RTOL = 1e-5.
  * conv2 data gradient: 288 (output channel, tap) terms -> 1.7e-5: RTOL_BD = 2e-5.
  * weight gradients: a conv2 tap sums one term per conv-output position, B * 2H2 * 2W2 (routed positions non-zero);
    a conv1 tap sums one term per POOLING window, B * H1 * W1 (only a window's argmax position is routed).  A
    workgroup's lane adds its items' rows into one fp32 accumulator, then the workgroups' slabs are added in fixed order (slab_sum_kernel: 16 partial chains of nslabs / 16, then 16).  The worst-case bound of that chain
    (n ~ 10^3 .. 10^4 roundings) is 10^-4 .. 10^-3; rounding errors of unrelated partial sums are not aligned.  Held
    to RTOL_DW = 1e-5 of M like the conv ops: the measured worst over the shape table is 0.011 of that bound (dW2,
    fp32).  A single wrong item of one workgroup changes a weight-gradient element by only its share of M; it is found
    through the data-gradient outputs of the same item instead.
  * bf16 stores: the fp32 result is rounded once more to bf16 (1/2 ulp of the stored value); fp32 stores add nothing.
  * Rounding the kernel does INSIDE an op is applied to the reference operands: the fused bf16 epilogue contracts the
    bf16-rounded dp1 (the value it also stores when asked to) with x split into bf16 high + low parts (x_hilo).

Tie rule (check_codes): the decoded position must be the float64 first maximum in scan order (dy * 2 + dx, as
aten::max_pool2d_with_indices) and the live bit must be "pooled value > 0".  The exceptions: another position is
accepted when ITS value lies below the maximum by no more than twice the element bound (both values can be off by one
bound), and the live bit is free when |maximum| is within one bound of 0.  A window with such a value (or maximum) is
a near-tie.  A later position that holds exactly the float64 maximum is accepted only when its magnitude M differs
from the first maximum's: an exact tie of different products (bf16 operands make rare ones) can round apart in fp32.
Equal input patches (clamped inputs make many) give equal M and equal fp32 sums, so there "first maximum" must hold
exactly.  An exact tie at the top with a third value inside the band still excuses that third value.  The count is
bounded by NEAR_TIE_FRAC of the windows (+ 8).  For a top-two gap (or pooled value) whose density near 0 is p / M,
the expected fraction is ~ 2 * rtol * p per window; conv2's pre-activations crowd around 0 (ReLU threshold), so p is
large there.  Measured over the shape table: <= 1.4e-4 of conv1's windows and <= 5.5e-4 of conv2's; NEAR_TIE_FRAC =
2e-3 keeps a factor >= 3.6 over both.
"""
import math

import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------------- plan mirrors (csrc/simnn_trunk.h)
ROWS = 4                # simnn_trunk.h ROWS: conv-output rows per step / tile
COLS = 64               # simnn_trunk.h COLS: conv-output columns per tile (conv2 forward, backward weight)
BD_COLS = 64            # simnn_conv2_bwd_data.hip BD_COLS: columns per backward-data item
BD_CAP_FUSE = 512       # simnn_trunk.h cap::c2_bwd_fused
BD_CAP = 768            # simnn_trunk.h cap::c2_bwd_data
BW_CAP = 768            # simnn_trunk.h cap::c2_bwd_weight
C2F_CAP = 768           # simnn_trunk.h cap::c2_fwd
C1_CAP = 1536           # simnn_trunk.h cap::c1_fwd
C1_SLABS_CAP = 1024     # simnn_trunk.h cap::c1_slabs (simnn_conv1.hip conv1_slabs)
C1BD_CAP = 8192         # simnn_trunk.h cap::c1_bwd_data: conv1 input-gradient blocks
PLAN_ENV = ("GDM_BD_CAP", "GDM_BW_CAP", "GDM_BW_NSEG", "GDM_C2F_CAP", "GDM_C1_CAP")

# (B, H, W, bsplit, what) -- the shape table of tests/test_simnn_trunk_batch_gpu.py; tests/test_trunk_plans.py asserts which regime each one reaches
SHAPES = [
    (512, 128, 256, 256, "production 2B launch"),
    (256, 128, 256, 128, "production B launch; fused items == cap; weight gradient 1024 items in 2 segments"),
    (256, 128, 216, 128, "reference geometry"),
    (32, 128, 216, 16, "reference geometry, small batch"),
    (257, 128, 256, 128, "fused items = cap + 2"),
    (700, 12, 258, 350, ">= 2 items per workgroup, uneven tail"),
    (385, 16, 260, 192, ">= 2 items per workgroup, uneven tail"),
    (130, 40, 130, 65, "row segments with wrap, short last segment"),
    (1100, 9, 66, 550, "odd H1 / W1, partial last column tile"),
    (300, 8, 130, 150, "odd W1, partial last column tile"),
]

DTYPES = ("fp32", "bf16")    # every shape runs in both compute dtypes
RTOL = 1e-5
RTOL_BD = 2e-5
RTOL_DW = 1e-5
NEAR_TIE_FRAC = 2e-3


def _seg_plan(B, H1, W1, target, cols, cap):
    """seg_plan (simnn_trunk.h): items = (image, row segment, column tile)."""
    nrq = (H1 + ROWS - 1) // ROWS
    n_ctiles = (W1 + cols - 1) // cols
    strips = B * n_ctiles
    nseg = (target + strips - 1) // strips
    max_seg = nrq // 2 if nrq // 2 > 1 else 1
    nseg = min(max(nseg, 1), max_seg)
    seg_len = (nrq + nseg - 1) // nseg
    nseg = (nrq + seg_len - 1) // seg_len
    n_items = strips * nseg
    return dict(nrq=nrq, n_ctiles=n_ctiles, nseg=nseg, seg_len=seg_len, n_items=n_items, blocks=min(n_items, cap),
                last_seg_len=nrq - (nseg - 1) * seg_len)


def bd_plan(B, H1, W1, fuse):
    return _seg_plan(B, H1, W1, 512, BD_COLS, BD_CAP_FUSE if fuse else BD_CAP)


def bw_plan(B, H1, W1):
    return _seg_plan(B, H1, W1, 1024, COLS, BW_CAP)


def c2f_plan(B, H1, W1):
    """gdm_simnn_conv2_fwd and conv2_fwd_kernel's walk over its tiles (simnn_conv2_fwd.hip)."""
    H2, W2 = H1 // 2, W1 // 2
    n_ctiles = (2 * W2 + COLS - 1) // COLS
    nrq = (2 * H2 + ROWS - 1) // ROWS
    n_tiles = B * nrq * n_ctiles
    G = min(n_tiles, C2F_CAP)
    rounds = [len(range(u, n_tiles, G)) for u in range(G)]     # tiles walked by each (remapped) start id
    return dict(n_ctiles=n_ctiles, nrq=nrq, n_tiles=n_tiles, grid=G, xcd_remap=G % 8 == 0,
                pair_rounds=max(rounds) // 2, odd_tail=any(r % 2 == 1 for r in rounds))


def c2f_workgroup(u, G):
    """The workgroup that runs conv2 forward tile u (inverse of the XCD remap in simnn_conv2_fwd.hip's conv2_fwd_kernel)."""
    u0 = u % G
    if G % 8 == 0:
        return (u0 % (G // 8)) * 8 + u0 // (G // 8)
    return u0


def conv1_fwd_blocks(B, H):
    """gdm_simnn_conv1_fwd_pair (simnn_conv1.hip): 4 pooled rows per workgroup, capped."""
    n_rows = B * ((H + 1) // 2)
    return dict(n_rows=n_rows, blocks=min((n_rows + 3) // 4, C1_CAP))


def conv1_slabs(B, H, W):
    """conv1_slabs (simnn_conv1.hip)"""
    total = B * ((H + 1) // 2) * ((W + 1) // 2)
    return max(1, min((total + 2047) // 2048, C1_SLABS_CAP))


def conv1_bwd_data_blocks(B, H, W):
    """gdm_simnn_conv1_bwd_data (simnn_conv1.hip)"""
    return min((B * H * W + 255) // 256, C1BD_CAP)


def plan_env_overrides():
    import os
    return {k: os.environ[k] for k in PLAN_ENV if os.environ.get(k)}


# -------------------------------------------------------------------------------------------- fc1's GEMM plan
def _fast_ok(m, n):
    """gdm_gemm_bf16_fast_ok for these contiguous operands: M * N >= 64 * 64 (gemm_bf16.hip, gdm_gemm_bf16_fast_ok)"""
    return m * n >= 64 * 64


def gemm_path(m, n, k, compute):
    """mirror of gdm_gemm's plan (gemm_plan in gemm.hip, gdm_gemm_bf16_fast_deep in gemm_bf16.hip) for fc1's products.

    Assumptions of the mirror (true for fc1's contiguous operands): the fast path's gdm_gemm_bf16_fast_ok is reduced to
    M * N >= 64 * 64; operand_ok (bf16/fp32 operands with one unit stride), the vector epilogue's row / pointer
    alignment (N % 4 == 0) and the 16-byte bias alignment hold.  test_fc1_gemms_at_their_real_shapes asserts that it
    equals the library's own plan (ops.gemm_plan) on the device tensors of all three products; the dispatch itself is
    covered by tests/test_gemm_ref.py."""
    from gan_des_midi_music_gen_amd import ops
    split = ops.default_split_k(m, n, k, compute)
    fast = compute == ops.BF16 and _fast_ok(m, n)
    kt = 64 if (fast or compute == ops.BF16) else 32
    tiles = (k + kt - 1) // kt
    split = min(split, tiles)
    per = (tiles + split - 1) // split
    split = (tiles + per - 1) // per
    last = tiles - (split - 1) * per
    variant = None
    if fast:
        outer = ((n + 127) // 128) * split
        variant = 1 if (split > 1 and outer * ((m + 127) // 128) <= 512 and per * kt >= 256) else 0
    return dict(split=split, per_tiles=per, last_tiles=last, kt=kt, fast=fast, variant=variant)


# ----------------------------------------------------------------------------------------------- code decoders
def _code1_fields(code1):
    """int64 (B, H1, 4 Q1) -> int32 fields (B, H1, 4 Q1 pixels, 4 groups) (include/gdm.h: [row][quad][g][pw % 4])."""
    B, H1, n = code1.shape
    f = code1.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return f.view(B, H1, n // 4, 4, 4).permute(0, 1, 2, 4, 3).reshape(B, H1, n, 4)


def decode_code1(code1, W1):
    """-> pos (B, H1, W1, 16) int64 in 0..3, live (B, H1, W1, 16) bool, pad_ok (pixels >= W1 hold 0, bit 3 is 0)."""
    f = _code1_fields(code1.cpu())
    nib = torch.stack([(f >> (4 * k)) & 0xF for k in range(4)], dim=-1)           # (B, H1, 4Q1, g, k)
    nib = nib.reshape(*f.shape[:3], 16).long()                                     # channel 4g + k
    pad_ok = bool((nib[:, :, W1:] == 0).all()) and bool(((nib[:, :, :W1] & 8) == 0).all())
    nib = nib[:, :, :W1]
    return nib & 3, (nib & 4) != 0, pad_ok


def encode_code1(pos, live):
    """inverse of decode_code1: pos / live (B, H1, W1, 16) -> int64 (B, H1, 4 Q1), pixels >= W1 zero."""
    B, H1, W1, _ = pos.shape
    q1 = (W1 + 3) // 4
    nib = torch.zeros(B, H1, 4 * q1, 16, dtype=torch.int32)
    nib[:, :, :W1] = (pos.to(torch.int32) & 3) | (live.to(torch.int32) << 2)
    nib = nib.view(B, H1, 4 * q1, 4, 4)
    f = sum(nib[..., k] << (4 * k) for k in range(4))                              # (B, H1, 4Q1, g)
    f = f.view(B, H1, q1, 4, 4).permute(0, 1, 2, 4, 3).reshape(B, H1, 16 * q1)   # [quad][g][pw % 4]
    f = torch.where(f >= 0x8000, f - 0x10000, f).to(torch.int16)
    return f.contiguous().view(torch.int64)


def decode_code2(code2):
    """uint8 (B, H2, W2, 16), byte j = 8 (c_even + 5 c_odd) -> pos (B, H2, W2, 32) int64 in 0..3 (0 where dead),
    live bool, ok (every byte a valid code)."""
    c = code2.cpu().long()
    n = c >> 3
    ok = bool(((c & 7) == 0).all()) and bool((n < 25).all())
    cc = torch.stack([n % 5, n // 5], dim=-1).reshape(*c.shape[:3], 32)
    live = cc != 4
    return torch.where(live, cc, torch.zeros_like(cc)), live, ok


def encode_code2(pos, live):
    c = torch.where(live, pos.long(), torch.full_like(pos.long(), 4))
    return (8 * (c[..., 0::2] + 5 * c[..., 1::2])).to(torch.uint8)


# -------------------------------------------------------------------------------------- float64 references
def _d(t):
    return t.detach().cpu().double()


def x_hilo(x):
    """x as the fused bf16 epilogue holds it: bf16 high part + bf16 low part of the remainder (exact to ~2^-17)."""
    x = x.detach().cpu().float()
    hi = x.bfloat16().float()
    return (hi.double() + (x - hi).bfloat16().double())


def _windows(v, h, w):
    """(B, C, >= 2h, >= 2w) -> pooling windows (B, h, w, C, 4) in scan order dy * 2 + dx."""
    B, C = v.shape[:2]
    v = v[:, :, :2 * h, :2 * w].reshape(B, C, h, 2, w, 2)
    return v.permute(0, 2, 4, 1, 3, 5).reshape(B, h, w, C, 4)


def conv1_windows(x, w1, b1):
    """conv1 (k2 s1 p1) pre-activation windows and their magnitudes, (B, H1, W1, 16, 4) float64."""
    x = _d(x)[:, None]
    H, W = x.shape[2], x.shape[3]
    h1, ww1 = (H + 1) // 2, (W + 1) // 2
    v = F.conv2d(x, _d(w1), _d(b1), padding=1)
    m = F.conv2d(x.abs(), _d(w1).abs(), _d(b1).abs(), padding=1)
    return _windows(v, h1, ww1), _windows(m, h1, ww1)


def conv2_windows(p1, w2r, b2):
    """conv2 (k3 s1 p1) on the kernel's p1 (B, H1, W1, 16) with the packed-precision weight: (B, H2, W2, 32, 4)."""
    p = _d(p1).permute(0, 3, 1, 2)
    H2, W2 = p.shape[2] // 2, p.shape[3] // 2
    v = F.conv2d(p, _d(w2r), _d(b2), padding=1)
    m = F.conv2d(p.abs(), _d(w2r).abs(), _d(b2).abs(), padding=1)
    return _windows(v, H2, W2), _windows(m, H2, W2)


def pool(vw, mw):
    """ReLU(max over the window) and its bound magnitude (the largest M of the window)."""
    return vw.max(-1).values.clamp_min(0.0), mw.max(-1).values


def _scatter_windows(g, pos, live, hout, wout):
    """gradient (B, h, w, C) routed to position pos of each window where live -> (B, C, hout, wout) float64."""
    B, h, w, C = g.shape
    sel = torch.nn.functional.one_hot(pos.long(), 4).to(torch.float64) * live[..., None].to(torch.float64)
    full = (_d(g)[..., None] * sel)                                               # (B, h, w, C, 4)
    full = full.reshape(B, h, w, C, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, C, 2 * h, 2 * w)
    return F.pad(full, (0, wout - 2 * w, 0, hout - 2 * h))


def conv2_bwd_data_ref(dp2, pos2, live2, w2r, H1, W1):
    """dp1 (B, H1, W1, 16) and M, routed through the kernel's code2."""
    dc = _scatter_windows(dp2, pos2, live2, H1, W1)
    w = _d(w2r)
    dp1 = F.conv_transpose2d(dc, w, padding=1)
    mag = F.conv_transpose2d(dc.abs(), w.abs(), padding=1)
    return dp1.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def conv2_bwd_weight_ref(dp2, pos2, live2, p1):
    """(dw2 (32,16,3,3), db2 (32)) and their magnitudes for a chunk of images (sum chunks in float64)."""
    H1, W1 = p1.shape[1], p1.shape[2]
    dc = _scatter_windows(dp2, pos2, live2, H1, W1)
    p = _d(p1).permute(0, 3, 1, 2)
    dw = torch.nn.grad.conv2d_weight(p, (32, 16, 3, 3), dc, padding=1)
    mw = torch.nn.grad.conv2d_weight(p.abs(), (32, 16, 3, 3), dc.abs(), padding=1)
    return dw, dc.sum((0, 2, 3)), mw, dc.abs().sum((0, 2, 3))


def conv1_bwd_weight_ref(dp1, pos1, live1, x):
    """(dw1 (16,1,2,2), db1 (16)) and magnitudes for a chunk; x as the kernel reads it (x_hilo for the bf16 fused
    epilogue, the fp32 input otherwise)."""
    xx = _d(x)[:, None]
    H, W = xx.shape[2], xx.shape[3]
    dc = _scatter_windows(dp1, pos1, live1, H + 1, W + 1)
    dw = torch.nn.grad.conv2d_weight(xx, (16, 1, 2, 2), dc, padding=1)
    mw = torch.nn.grad.conv2d_weight(xx.abs(), (16, 1, 2, 2), dc.abs(), padding=1)
    return dw, dc.sum((0, 2, 3)), mw, dc.abs().sum((0, 2, 3))


def conv1_bwd_data_ref(dp1, pos1, live1, w1, H, W):
    """dx (B, H, W) and M."""
    dc = _scatter_windows(dp1, pos1, live1, H + 1, W + 1)
    w = _d(w1)
    dx = F.conv_transpose2d(dc, w, padding=1)[:, 0]
    mag = F.conv_transpose2d(dc.abs(), w.abs(), padding=1)[:, 0]
    return dx, mag


# -------------------------------------------------------------------------------------------------- checkers
_MANT = {torch.bfloat16: 8, torch.float16: 11}


def ulp(v, out_dtype):
    """ulp of |v| in the stored dtype (0 for fp32: an fp32 accumulator stored as fp32 is not rounded again)."""
    if out_dtype not in _MANT:
        return torch.zeros_like(v)
    _, e = torch.frexp(v.abs().to(torch.float64))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - _MANT[out_dtype]).to(torch.int32)) * (v != 0)


class CheckError(AssertionError):
    pass


def check_elementwise(got, ref, mag, *, rtol, out_dtype, where, what=""):
    """Pass iff |got - ref| <= rtol * M + 1/2 ulp_out(|ref| + rtol * M) for every element.  Returns the worst
    |err| / bound; on failure names the worst element through ``where(index tuple) -> str``."""
    got = got.detach().cpu().double()
    ref, mag = ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    err = (got - ref).abs()
    bound = rtol * mag + 0.5 * ulp(ref.abs() + rtol * mag, out_dtype)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        flat = int(ratio.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        n_bad = int((ratio > 1.0).sum())
        raise CheckError(f"{what}: {n_bad} element(s) out of bound; worst at {where(idx)}: got {float(got[idx]):.8g} "
                         f"ref {float(ref[idx]):.8g} |err| {float(err[idx]):.3g} > bound {float(bound[idx]):.3g} "
                         f"(M {float(mag[idx]):.3g}, rtol {rtol})")
    return worst


def check_codes(pos_k, live_k, vw, mw, *, rtol, where, what="", pos_when_dead=True):
    """The kernel's decoded codes against the float64 windows vw / magnitudes mw (.., 4).  Returns (near-tie count,
    window count); raises on a mismatch outside the tie rule or on too many near-ties.  pos_when_dead: the position is
    recorded even for ReLU-dead windows (code1); code2 records none."""
    vw, mw = vw.double(), mw.double()
    e = 2.0 * rtol * mw.max(-1).values                                  # two values, each off by <= one bound
    vmax = vw.max(-1).values
    ref_pos = vw.argmax(-1)                                             # first maximum in scan order
    ref_live = vmax > 0
    below = vmax[..., None] - vw                                        # >= 0; 0 at every (exactly) maximal position
    # values inside the tie band: non-maximal ones within e of the maximum, and later EXACT maxima whose operands
    # differ (a different magnitude M): an exact float64 tie of different products can round apart in fp32
    m_first = mw.gather(-1, ref_pos[..., None])
    in_band = ((below > 0) & (below <= e[..., None])) | ((below == 0) & (mw != m_first))
    pos_tie = in_band.any(-1)
    live_tie = vmax.abs() <= e / 2
    pos_k, live_k = pos_k.long(), live_k.bool()
    bad_live = (live_k != ref_live) & ~live_tie
    check_pos = torch.ones_like(live_k) if pos_when_dead else (live_k & ref_live)
    # a position other than the first maximum is excused only if ITS value lies in the band; a later position holding
    # exactly the maximum of the same operands (equal input patches) breaks "first maximum in scan order"
    k_in_band = in_band.gather(-1, pos_k.clamp(0, 3)[..., None])[..., 0]
    bad_pos = (pos_k != ref_pos) & ~k_in_band & check_pos
    bad = bad_live | bad_pos
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise CheckError(f"{what}: {int(bad.sum())} wrong code(s); first at {where(idx)}: kernel pos "
                         f"{int(pos_k[idx])} live {bool(live_k[idx])}, float64 pos {int(ref_pos[idx])} "
                         f"live {bool(ref_live[idx])} (window {[float(v) for v in vw[idx]]}, tie band {float(e[idx]):.3g})")
    ties = int(((pos_tie & check_pos) | live_tie).sum())
    n = int(vmax.numel())
    if ties > NEAR_TIE_FRAC * n + 8:
        raise CheckError(f"{what}: {ties} near-ties in {n} windows (bound {NEAR_TIE_FRAC} of the windows + 8)")
    return ties, n


# ------------------------------------------------------------------------------- where: element -> schedule
def where_bd(B, H1, W1, fuse, b0=0):
    """dp1 element (b, ih, iw, c) of a chunk starting at image b0 -> its backward-data plan item."""
    p = bd_plan(B, H1, W1, fuse)

    def f(idx):
        b, ih, iw, c = idx[0] + b0, idx[1], idx[2], idx[3] if len(idx) > 3 else 0
        rq = ih // ROWS
        sg, ct = rq // p["seg_len"], iw // BD_COLS
        s = (b * p["nseg"] + sg) * p["n_ctiles"] + ct
        return (f"(image {b}, row {ih}, column {iw}, channel {c}) = item {s} (image {b}, segment {sg}, column tile "
                f"{ct}), workgroup {s % p['blocks']} item #{s // p['blocks']} of {p['n_items']} on {p['blocks']}")
    return f


def where_c2f(B, H1, W1, b0=0):
    """p2 / code2 element (b, ph, pw, c) -> conv2 forward tile id and the workgroup that runs it."""
    p = c2f_plan(B, H1, W1)

    def f(idx):
        b, ph, pw, c = idx[0] + b0, idx[1], idx[2], idx[3] if len(idx) > 3 else 0
        u = (b * p["nrq"] + (2 * ph) // ROWS) * p["n_ctiles"] + (2 * pw) // COLS
        return (f"(image {b}, row {ph}, column {pw}, channel {c}) = tile {u} of {p['n_tiles']}, workgroup "
                f"{c2f_workgroup(u, p['grid'])} round {u // p['grid']} on {p['grid']}")
    return f


def where_rows(B, H, b0=0, what="pooled row"):
    """conv1 outputs: the global pooled-row index a wave walks (conv1_fwd_kernel)."""
    def f(idx):
        b, r = idx[0] + b0, idx[1]
        rest = ", ".join(str(i) for i in idx[2:])
        return f"(image {b}, row {r}, {rest}) = {what} {b * H + r}"
    return f


def where_tap(shape_name):
    def f(idx):
        return f"{shape_name}{list(idx)}"
    return f
