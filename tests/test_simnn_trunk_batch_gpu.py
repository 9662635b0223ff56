"""GPU: model 1's conv trunk kernels and fc1's GEMMs at the batch sizes the trainers run, element by element against
float64 (tests/trunk_ref.py states the bounds and the tie rule).

The shape table reaches the persistent kernels' multi-item regimes (several items per workgroup, row segments, the
uneven tails, conv2 forward's pair loop and XCD remap, the grid caps); tests/test_trunk_plans.py proves that on the
CPU.  Every op runs in isolation on the kernel's own inputs, so a failure names the plan item it sits in.
Measured worst |err| / bound and near-tie counts go to helpers.record.
"""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops, synthetic  # noqa: E402
from gan_des_midi_music_gen_amd.ops import BF16, F32  # noqa: E402

import trunk_ref as tr  # noqa: E402
from trunk_ref import SHAPES, gemm_path  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"

# the clamped family runs on every shape; the tie-free family on every shape except 256x128x216 and 257x128x256, whose
# plans the production launches and 32x128x216 already cover (the float64 reference of each big case costs 10-25 s of
# the file's time budget)
CONTINUOUS = {(512, 128, 256), (256, 128, 256), (32, 128, 216), (700, 12, 258), (385, 16, 260), (130, 40, 130),
              (1100, 9, 66), (300, 8, 130)}


def _cases():
    for (b, h, w, bs, what) in SHAPES:
        for dt in (F32 if d == "fp32" else BF16 for d in tr.DTYPES):
            fams = ["clamped", "continuous"] if (b, h, w) in CONTINUOUS else ["clamped"]
            for fam in fams:
                yield pytest.param(b, h, w, bs, dt, fam, id=f"{b}x{h}x{w}-{'bf16' if dt == BF16 else 'fp32'}-{fam}")


def _inputs(b, h, w, fam, seed):
    g = torch.Generator().manual_seed(seed)
    if fam == "clamped":
        x = synthetic.spectrogram_batch(b, (h, w), seed=seed)           # clamp(N(-35, 18^2), -80, 30): exact ties
    else:
        x = torch.randn(b, h, w, generator=g, dtype=torch.float64).mul(18.0).sub(35.0).float()   # tie-free
    w1 = torch.randn(16, 1, 2, 2, generator=g) * 0.1
    b1 = torch.randn(16, generator=g) * 0.5 + 2.0
    w2 = torch.randn(32, 16, 3, 3, generator=g) * 0.05
    b2 = torch.randn(32, generator=g) * 0.1
    return x, w1, b1, w2, b2


class _Log:
    """collects every check's worst ratio; failures are gathered so that one run reports all of them"""
    def __init__(self, name):
        self.name, self.worst, self.ties, self.fail = name, {}, {}, []

    def elem(self, key, *a, **k):
        try:
            r = tr.check_elementwise(*a, what=key, **k)
        except tr.CheckError as e:
            self.fail.append(str(e))
            r = float("inf")
        self.worst[key] = max(self.worst.get(key, 0.0), r)

    def codes(self, key, *a, **k):
        try:
            t, n = tr.check_codes(*a, what=key, **k)
            tt, nn = self.ties.get(key, (0, 0))
            self.ties[key] = (tt + t, nn + n)
        except tr.CheckError as e:
            self.fail.append(str(e))

    def finish(self, **extra):
        record(self.name, worst_ratio=self.worst, near_ties=self.ties, n_fail=len(self.fail), **extra)
        assert not self.fail, "\n".join(self.fail[:12])


def _chunk(h1, w1):
    return max(1, 3_000_000 // (h1 * w1 * 16))


@pytest.mark.parametrize("b,h,w,bsplit,dt,fam", list(_cases()))
def test_trunk_kernels_against_float64(b, h, w, bsplit, dt, fam):
    assert not tr.plan_env_overrides(), f"GDM_* plan overrides set: {tr.plan_env_overrides()}"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    t0 = time.time()
    x, w1, b1, w2, b2 = _inputs(b, h, w, fam, seed=b * 7 + h * 3 + w)
    h1, ww1 = (h + 1) // 2, (w + 1) // 2
    h2, w2n = h1 // 2, ww1 // 2
    tdt = ops.torch_dtype(dt)
    out_dt = torch.bfloat16 if dt == BF16 else torch.float32
    w2r = w2.bfloat16().float() if dt == BF16 else w2                     # the pack's operand precision
    xd, w1d, b1d, w2d, b2d = (t.to(DEV) for t in (x, w1, b1, w2, b2))
    g = torch.Generator().manual_seed(b + h + w)
    dp2 = (torch.randn(b, h2, w2n, 32, generator=g) * 0.1).to(tdt)

    # ---------------------------------------------------------------------------------------- the kernels
    p1, code1 = ops.simnn_conv1_fwd(xd, w1d, b1d, dt)
    for bs in sorted({1, bsplit, b - 1}):
        pp, cc = ops.simnn_conv1_fwd(xd[:bs].contiguous(), w1d, b1d, dt, x1=xd[bs:].contiguous())
        assert torch.equal(pp, p1) and torch.equal(cc, code1), f"conv1 pair form, bsplit {bs}"
    pack = ops.simnn_conv2_pack(w2d, dt)
    p2, code2 = ops.simnn_conv2_fwd(p1, pack, b2d)
    dp2d = dp2.to(DEV)
    dp1 = ops.simnn_conv2_bwd_data(dp2d, code2, pack, h1, ww1)
    dw1f, db1f, dp1f = ops.simnn_conv2_bwd_fused(dp2d, code2, pack, code1, xd, want_dp1=True)
    fused = {"fused want_dp1": (dw1f, db1f)}
    fused["fused no dp1"] = ops.simnn_conv2_bwd_fused(dp2d, code2, pack, code1, xd)[:2]
    for bs in sorted({1, bsplit, b - 1}):
        fused[f"fused 2B bsplit {bs}"] = ops.simnn_conv2_bwd_fused(dp2d, code2, pack, code1, xd[:bs].contiguous(),
                                                                   xd[bs:].contiguous())[:2]
    # x1 four bytes off a 16-byte boundary: the scalar x-window path
    buf = torch.empty(xd[bsplit:].numel() + 1, device=DEV)
    x1v = buf[1:].view(b - bsplit, h, w)
    x1v.copy_(xd[bsplit:])
    fused["fused 2B scalar x"] = ops.simnn_conv2_bwd_fused(dp2d, code2, pack, code1, xd[:bsplit].contiguous(), x1v)[:2]
    dw2, db2 = ops.simnn_conv2_bwd_weight(dp2d, code2, p1)
    dw2b, db2b = ops.simnn_conv2_bwd_weight(dp2d, code2, p1)
    assert torch.equal(dw2, dw2b) and torch.equal(db2, db2b), "conv2 weight gradient must be bit-reproducible"
    dw1s, db1s = ops.simnn_conv1_bwd_weight(dp1, code1, xd)
    dw1a, db1a = dw1s.clone(), db1s.clone()
    ops.simnn_conv1_bwd_weight(dp1, code1, xd, out=(dw1a, db1a), accumulate=True)
    dx = ops.simnn_conv1_bwd_data(dp1, code1, w1d, h, w)
    torch.cuda.synchronize()
    t_gpu = time.time() - t0

    # ------------------------------------------------------------------------------- float64, chunk by chunk
    c = lambda t: t.cpu()   # noqa: E731
    p1c, code1c, p2c, code2c, dp1c, dp1fc, dxc = map(c, (p1, code1, p2, code2, dp1, dp1f, dx))
    log = _Log(f"trunk_batch {b}x{h}x{w} {'bf16' if dt == BF16 else 'fp32'} {fam}")
    pos1, live1, pad_ok = tr.decode_code1(code1c, ww1)
    assert pad_ok, "code1: pixels >= W1 of a row's last quad (or bit 3) not zero"
    pos2, live2, ok2 = tr.decode_code2(code2c)
    assert ok2, "code2: byte outside 8 * (0..24)"
    xh = tr.x_hilo(x) if dt == BF16 else x.double()
    acc = {k: 0 for k in ("dw2", "db2", "mdw2", "mdb2", "dw1f", "db1f", "mdw1f", "mdb1f", "dw1", "db1", "mdw1", "mdb1")}
    n = _chunk(h1, ww1)
    for b0 in range(0, b, n):
        s = slice(b0, min(b, b0 + n))
        vw, mw = tr.conv1_windows(x[s], w1, b1)
        ref, mag = tr.pool(vw, mw)
        log.elem("conv1 p1", p1c[s], ref, mag, rtol=tr.RTOL, out_dtype=out_dt, where=tr.where_rows(b, h1, b0))
        log.codes("conv1 code1", pos1[s], live1[s], vw, mw, rtol=tr.RTOL, where=tr.where_rows(b, h1, b0))
        del vw, mw
        vw, mw = tr.conv2_windows(p1c[s], w2r, b2)
        ref, mag = tr.pool(vw, mw)
        log.elem("conv2 p2", p2c[s], ref, mag, rtol=tr.RTOL, out_dtype=out_dt, where=tr.where_c2f(b, h1, ww1, b0))
        log.codes("conv2 code2", pos2[s], live2[s], vw, mw, rtol=tr.RTOL, where=tr.where_c2f(b, h1, ww1, b0),
                  pos_when_dead=False)
        del vw, mw
        ref, mag = tr.conv2_bwd_data_ref(dp2[s], pos2[s], live2[s], w2r, h1, ww1)
        log.elem("conv2 bwd data dp1", dp1c[s], ref, mag, rtol=tr.RTOL_BD, out_dtype=out_dt,
                 where=tr.where_bd(b, h1, ww1, False, b0))
        log.elem("fused dp1", dp1fc[s], ref, mag, rtol=tr.RTOL_BD, out_dtype=out_dt,
                 where=tr.where_bd(b, h1, ww1, True, b0))
        for k, v in zip(("dw2", "db2", "mdw2", "mdb2"), tr.conv2_bwd_weight_ref(dp2[s], pos2[s], live2[s], p1c[s])):
            acc[k] = acc[k] + v
        # the fused epilogue contracts its own (stored) dp1 with x as it holds it; the standalone kernel reads dp1
        for k, v in zip(("dw1f", "db1f", "mdw1f", "mdb1f"), tr.conv1_bwd_weight_ref(dp1fc[s], pos1[s], live1[s], xh[s])):
            acc[k] = acc[k] + v
        for k, v in zip(("dw1", "db1", "mdw1", "mdb1"), tr.conv1_bwd_weight_ref(dp1c[s], pos1[s], live1[s], x[s])):
            acc[k] = acc[k] + v
        ref, mag = tr.conv1_bwd_data_ref(dp1c[s], pos1[s], live1[s], w1, h, w)
        log.elem("conv1 bwd data dx", dxc[s], ref, mag, rtol=tr.RTOL, out_dtype=torch.float32,
                 where=tr.where_rows(b, h, b0, what="input row"))
    tap = tr.where_tap
    log.elem("conv2 bwd weight dw2", dw2.cpu(), acc["dw2"], acc["mdw2"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
             where=tap("dw2"))
    log.elem("conv2 bwd weight db2", db2.cpu(), acc["db2"], acc["mdb2"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
             where=tap("db2"))
    for name, (dwk, dbk) in fused.items():
        log.elem(f"{name} dw1", dwk.cpu(), acc["dw1f"], acc["mdw1f"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
                 where=tap("dw1"))
        log.elem(f"{name} db1", dbk.cpu(), acc["db1f"], acc["mdb1f"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
                 where=tap("db1"))
    log.elem("conv1 bwd weight dw1", dw1s.cpu(), acc["dw1"], acc["mdw1"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
             where=tap("dw1"))
    log.elem("conv1 bwd weight db1", db1s.cpu(), acc["db1"], acc["mdb1"], rtol=tr.RTOL_DW, out_dtype=torch.float32,
             where=tap("db1"))
    log.elem("conv1 bwd weight dw1 accumulate", dw1a.cpu(), 2 * acc["dw1"], 2 * acc["mdw1"], rtol=tr.RTOL_DW,
             out_dtype=torch.float32, where=tap("dw1"))
    log.elem("conv1 bwd weight db1 accumulate", db1a.cpu(), 2 * acc["db1"], 2 * acc["mdb1"], rtol=tr.RTOL_DW,
             out_dtype=torch.float32, where=tap("db1"))
    log.finish(seconds_gpu=round(t_gpu, 2), seconds_total=round(time.time() - t0, 2))


# ---------------------------------------------------------------------------------------- fc1 at its real shapes
def _gemm_check(name, got, a, bm, *, bias=None, relu=False, n_chain, out_dt):
    """float64 reference of a @ bm (+ bias, ReLU) and the element bound.  The worst case of the longest fp32 rounding
    chain (one slab's contraction plus the split-K reduction, n_chain * 2^-24: up to 8.5e-5) would let a split-K slab
    off by 1e-3 pass.  Held to tr.RTOL_DW = 1e-5 of M instead, on the same argument as the trunk's weight gradients
    (rounding errors of unrelated partial sums are not aligned): measured worst 0.045 of it (dW, fp32); the bf16
    dX output adds its half ulp.  n_chain is recorded beside it."""
    ref = a.double() @ bm.double()
    mag = a.double().abs() @ bm.double().abs()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    rtol = tr.RTOL_DW
    r = tr.check_elementwise(got, ref, mag, rtol=rtol, out_dtype=out_dt, what=name,
                             where=lambda i: f"(row {i[0]}, column {i[1]})")
    record(f"fc1 {name}", worst_ratio=r, rtol=rtol, worst_case_rtol=n_chain * 2.0 ** -24)


def _mirror_is_the_library(mirror, plan, what):
    """trunk_ref.gemm_path against gdm_gemm_plan on the tensors of the call: split, slab width, fast path, variant"""
    lib = dict(split=plan["split_k"], k_per_split=plan["k_per_split"], fast=plan["kernel"].startswith("fast"),
               variant={"fast_k32": 0, "fast_k64": 1}.get(plan["kernel"]))
    mine = dict(split=mirror["split"], k_per_split=mirror["per_tiles"] * mirror["kt"], fast=mirror["fast"],
                variant=mirror["variant"])
    assert mine == lib, f"{what}: trunk_ref.gemm_path says {mine}, the library {lib}"


@pytest.mark.parametrize("comp", [F32, BF16])
@pytest.mark.parametrize("m,k", [(512, 65536), (256, 65536), (256, 55296), (32, 55296)])
def test_fc1_gemms_at_their_real_shapes(comp, m, k):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = torch.Generator().manual_seed(m + k)
    n = 128
    tdt = torch.bfloat16 if comp == BF16 else torch.float32
    rb = (lambda t: t.bfloat16().float()) if comp == BF16 else (lambda t: t)
    flat = torch.relu(torch.randn(m, k, generator=g)).to(tdt)          # p2 (ReLU output) in the compute dtype
    wf1p = torch.randn(n, k, generator=g) / k ** 0.5
    bf1 = torch.randn(n, generator=g) * 0.1
    dh = torch.randn(m, n, generator=g) * 1e-2
    fd, wd, bd, dhd = flat.to(DEV), wf1p.to(DEV), bf1.to(DEV), dh.to(DEV)
    tag = f"{'bf16' if comp == BF16 else 'fp32'} M={m} K={k}"
    # forward: flat (M,K) @ wf1p^T + bias, ReLU (functional.py:76)
    pf = gemm_path(m, n, k, comp)
    assert pf["split"] > 1
    if comp == BF16:
        assert pf["fast"] and pf["variant"] == 1, pf
    if (m, k, comp) == (256, 55296, BF16):
        assert pf["last_tiles"] < pf["per_tiles"], pf          # a short last split-K slab
    _mirror_is_the_library(pf, ops.gemm_plan(fd, wd.t(), bias_n=bd, act=ops.ACT_RELU, compute=comp), f"forward {tag}")
    h1 = ops.gemm(fd, wd.t(), bias_n=bd, act=ops.ACT_RELU, compute=comp)
    _gemm_check(f"forward {tag}", h1.cpu(), rb(flat.float()), rb(wf1p).t(), bias=bf1, relu=True,
                n_chain=pf["per_tiles"] * pf["kt"] + pf["split"] + 2, out_dt=torch.float32)
    # dW = dh^T (128, M) @ flat (functional.py:97, train.py:456)
    pw = gemm_path(n, k, m, comp)
    _mirror_is_the_library(pw, ops.gemm_plan(dhd.t(), fd, compute=comp), f"dW {tag}")
    dw = ops.gemm(dhd.t(), fd, compute=comp)
    _gemm_check(f"dW {tag}", dw.cpu(), rb(dh).t(), rb(flat.float()), n_chain=pw["per_tiles"] * pw["kt"] + pw["split"] + 2,
                out_dt=torch.float32)
    # dX = dh @ wf1p, stored in the compute dtype (functional.py:99, train.py:464)
    px = gemm_path(m, k, n, comp)
    _mirror_is_the_library(px, ops.gemm_plan(dhd, wd, compute=comp, out_dtype=comp), f"dX {tag}")
    dxf = ops.gemm(dhd, wd, compute=comp, out_dtype=comp)
    _gemm_check(f"dX {tag}", dxf.float().cpu(), rb(dh), rb(wf1p), n_chain=px["per_tiles"] * px["kt"] + px["split"] + 2,
                out_dt=tdt)
    record(f"fc1 paths {tag}", forward=pf, dW=pw, dX=px)
