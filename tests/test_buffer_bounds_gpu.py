"""GPU: every MFMA-path and layer-wise entry point inside guarded buffers (tests/guarded.py): the conv trunk, model 2's
fused discriminator, model 1's generator, the Linear+BatchNorm block, the lowering and pointwise kernels, the GEMM's
split-K workspace, and the device entries whose outputs no other file puts between guard bytes (DES prologue, pack,
tracks and notes kernels, the math probe, the piano-roll raster, model 2's eval pack, the dB stage).

Each case is one production wrapper of gan_des_midi_music_gen_amd.ops run four times by guarded.run_case: twice plainly
(the result R; bit-reproducible or the case fails as non-deterministic), then with every input, output and the
workspace inside an arena filled with 0xFF (NaN / -1), then with 0x7F (3.39e38, finite: the library is built with
-fno-honor-nans, a max that drops a NaN would still pick it).  The workspace is exactly the bytes the library's own
*_workspace_bytes / *_chunks / *_pack_bytes functions ask for.  After each guarded run every guard byte must be intact
and every output and in-out tensor must equal R byte for byte.  Equality in BOTH guarded runs proves four things at
once: the result does not depend on bytes outside the inputs (halo lanes, descriptor extents, the per-half extents of
the pair forms, code1's quad-padded rows); not on earlier workspace content; not on earlier output content; and every
output byte is written.  No float64 reference is involved: the value tests stay where they are.

EXEMPT (guarded.EXEMPT, a closed list): the last 16 bytes of the DCNN weight pack -- padding behind the biases that no
kernel reads or writes (include/gdm.h, gdm_dcnn_pack_bytes; tests/test_mmgan_batch_gpu.py sets the same bytes aside).

Inputs come from the existing makers (trunk_bits.make_inputs, synthetic.mmgan_inputs, the _block / _params helpers of
the mmgan tests, the tables of lowering_ref / gemm_ref / mmgan_ref); shapes are the smallest at which each kernel's
tiling can still go wrong.  COVERED is the set of library entries the cases reach, checked against what ``_call``
actually saw, so a case that silently takes another path cannot hide; tests/test_guarded.py pins that every device
entry of the library is in COVERED or guarded by another file.

Measured wall time of the file on MI355X: 9.1 s for its 1012 cases (helpers.record "buffer_bounds"; 11 s with the
collection), the slowest case 0.6 s -- far below the float64 files, which recompute convolutions on the CPU.
"""
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import _lib, ops  # noqa: E402
from gan_des_midi_music_gen_amd.ops import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F32  # noqa: E402

import gemm_ref as GR  # noqa: E402
import guarded as G  # noqa: E402
import lowering_ref as LR  # noqa: E402
import mmgan_ref as MR  # noqa: E402
import trunk_bits as TB  # noqa: E402
import trunk_ref as TR  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
TDT = {F32: torch.float32, BF16: torch.bfloat16}
DTN = {F32: "fp32", BF16: "bf16"}
TYPES = (torch.float32, torch.bfloat16)
GDT = {torch.float32: F32, torch.bfloat16: BF16}

COVERED = {
    "gdm_simnn_conv1_fwd", "gdm_simnn_conv1_fwd_pair", "gdm_simnn_conv2_pack", "gdm_simnn_conv2_fwd",
    "gdm_simnn_conv2_bwd_data", "gdm_simnn_conv2_bwd_fused", "gdm_simnn_conv2_bwd_fused_finish",
    "gdm_simnn_conv2_bwd_weight", "gdm_simnn_conv1_bwd_weight", "gdm_simnn_conv1_bwd_data",
    "gdm_dcnn_pack", "gdm_dcnn_fused", "gdm_dcnn_fused_crit", "gdm_dcnn_fused_adam", "gdm_dcnn_fused_adam_crit",
    "gdm_simnn_gen_pack", "gdm_simnn_gen_first", "gdm_simnn_gen_convt_bn", "gdm_simnn_gen_last", "gdm_simnn_gen_eval",
    "gdm_bn_stats", "gdm_bn_partials", "gdm_bn_finalize",
    "gdm_linear_bn_act_fwd", "gdm_linear_bn_act_fwd_multi",
    "gdm_im2col", "gdm_col2im", "gdm_permute_pc", "gdm_maxpool2_fwd", "gdm_maxpool2_bwd",
    "gdm_bn_act_fwd", "gdm_bn_apply", "gdm_bn_act_bwd", "gdm_bias_act_fwd", "gdm_act_bwd", "gdm_colsum", "gdm_cast",
    "gdm_bce_with_logits", "gdm_criterion_loss", "gdm_adam_step", "gdm_adam_step_dev", "gdm_simnn_head",
    "gdm_concat_cols_multi", "gdm_nonfinite_count", "gdm_gemm",
    # device entries whose outputs no other file puts between guard bytes
    "gdm_des_scan", "gdm_des_routing", "gdm_des_pack", "gdm_piano_roll_raster", "gdm_des_log_to_roll",
    "gdm_des_math_probe", "gdm_des_log_tracks_count", "gdm_des_log_tracks", "gdm_des_log_to_notes",
    "gdm_des_log_to_notes_pc", "gdm_mmgan_gen_eval_pack", "gdm_power_to_db",
}

CASES = []                   # (id, builder); builder() -> dict(fn, inputs, inout, entry)
_ran = set()
_t0 = [None]


def case(cid, **kw):
    def deco(build):
        CASES.append((cid, functools.partial(build, **kw)))
        return build
    return deco


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(*shape, seed, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(dtype)


def _cap():
    return MR.cap_for(torch.cuda.get_device_properties(0).multi_processor_count)


# ===================================================================================================== a. conv trunk
# p1 geometries (B, H1, W1) of trunk_bits.SHAPES[:4], and the three small rows (B, H, W) of trunk_ref.SHAPES whose
# labels name a regime
P1_SHAPES = TB.SHAPES[:4]
X_ROWS = [(b, h, w) for (b, h, w, _bs, _what) in TR.SHAPES if (b, h, w) in ((300, 8, 130), (1100, 9, 66), (385, 16, 260))]
TRUNK = [("p1", s) for s in P1_SHAPES] + [("x", s) for s in X_ROWS]


def _geom(kind, s):
    """(B, H, W, H1, W1) of a trunk row"""
    b = s[0]
    h, w = (2 * s[1], 2 * s[2]) if kind == "p1" else (s[1], s[2])
    return b, h, w, (h + 1) // 2, (w + 1) // 2


def _tid(kind, s, dt):
    b, h, w, h1, w1 = _geom(kind, s)
    return f"x{b}x{h}x{w}-p1_{h1}x{w1}-{DTN[dt]}"


@functools.lru_cache(maxsize=2)
def _trunk(kind, s, dt):
    """trunk_bits.make_inputs for the p1 geometries; the same recipe on an odd-sized spectrogram for the (B, H, W) rows.
    Adds conv1's weight and bias, conv2's code2 and a gradient map dp1."""
    b, h, w, h1, w1 = _geom(kind, s)
    g = _gen(7919 * b + 131 * h1 + w1 + 1)
    cw1 = (torch.randn(16, 1, 2, 2, generator=g) * 0.1).to(DEV)
    cb1 = (torch.randn(16, generator=g) * 0.5 + 2.0).to(DEV)
    if kind == "p1":
        inp = dict(TB.make_inputs(s, dt, DEV))
    else:
        x = (torch.randn(b, h, w, generator=g) * 18 - 35).clamp(-80, 30).to(DEV)
        cw2 = torch.randn(32, 16, 3, 3, generator=g) * 0.05
        p1, code1 = ops.simnn_conv1_fwd(x, cw1, cb1, dt)
        if dt == F32:
            p1 = p1.to(torch.bfloat16).float()
        inp = {"x": x, "p1": p1.contiguous(), "code1": code1, "pack": ops.simnn_conv2_pack(cw2.to(DEV), dt),
               "b2": (torch.randn(32, generator=g) * 0.1).to(DEV),
               "dp2": (torch.randn(b, h1 // 2, w1 // 2, 32, generator=g) * 0.1).to(TDT[dt]).to(DEV)}
    assert inp["x"].shape == (b, h, w) and inp["p1"].shape == (b, h1, w1, 16)
    inp["w1"], inp["b1"] = cw1, cb1
    inp["code2"] = ops.simnn_conv2_fwd(inp["p1"], inp["pack"], inp["b2"])[1]
    inp["dp1"] = (torch.randn(b, h1, w1, 16, generator=g) * 0.1).to(TDT[dt]).to(DEV)
    return inp


def _bsplits(b):
    return sorted({1, b - 1}) if b >= 2 else []


def _conv1_fwd_abi(x, w, bias, dt):
    """gdm_simnn_conv1_fwd, the single-tensor entry (ops.simnn_conv1_fwd always takes the pair entry)"""
    b, h, wd = x.shape
    h1, w1 = (h + 1) // 2, (wd + 1) // 2
    p1 = ops.torch.empty((b, h1, w1, 16), dtype=TDT[dt], device=x.device)
    code1 = ops.torch.empty((b, h1, ops.simnn_code1_width(w1)), dtype=torch.int64, device=x.device)
    ops._call("gdm_simnn_conv1_fwd", ops._p(x), ops._p(w), ops._p(bias), b, h, wd, ops._p(p1), ops._p(code1), dt,
              ops._stream())
    return p1, code1


def _halves(x, bs):
    return x[:bs].contiguous(), x[bs:].contiguous()


for _kind, _s in TRUNK:
    for _dt in (F32, BF16):
        _k = dict(kind=_kind, s=_s, dt=_dt)
        _id = _tid(_kind, _s, _dt)
        _b = _s[0]

        @case(f"conv1_fwd-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            return dict(fn=lambda t: ops.simnn_conv1_fwd(t["x"], t["w"], t["b"], dt),
                        inputs=dict(x=i["x"], w=i["w1"], b=i["b1"]))

        @case(f"conv1_fwd_abi-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            return dict(fn=lambda t: _conv1_fwd_abi(t["x"], t["w"], t["b"], dt),
                        inputs=dict(x=i["x"], w=i["w1"], b=i["b1"]))

        for _bs in _bsplits(_b):
            @case(f"conv1_fwd_pair-bsplit{_bs}-{_id}", bs=_bs, **_k)
            def _c(kind, s, dt, bs):
                i = _trunk(kind, s, dt)
                x0, x1 = _halves(i["x"], bs)
                return dict(fn=lambda t: ops.simnn_conv1_fwd(t["x0"], t["w"], t["b"], dt, x1=t["x1"]),
                            inputs=dict(x0=x0, x1=x1, w=i["w1"], b=i["b1"]))

        @case(f"conv2_fwd-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            return dict(fn=lambda t: ops.simnn_conv2_fwd(t["p1"], t["pack"], t["b2"]),
                        inputs=dict(p1=i["p1"], pack=i["pack"], b2=i["b2"]))

        @case(f"conv2_bwd_data-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            h1, w1 = i["p1"].shape[1:3]
            return dict(fn=lambda t: ops.simnn_conv2_bwd_data(t["dp2"], t["code2"], t["pack"], h1, w1),
                        inputs=dict(dp2=i["dp2"], code2=i["code2"], pack=i["pack"]))

        for _want in (True, False):
            for _bs in [None] + _bsplits(_b):
                @case(f"conv2_bwd_fused-dp1{int(_want)}-{'whole' if _bs is None else f'bsplit{_bs}'}-{_id}", want=_want,
                      bs=_bs, **_k)
                def _c(kind, s, dt, want, bs):
                    i = _trunk(kind, s, dt)
                    x0, x1 = (i["x"], None) if bs is None else _halves(i["x"], bs)
                    return dict(fn=lambda t: ops.simnn_conv2_bwd_fused(t["dp2"], t["code2"], t["pack"], t["code1"],
                                                                       t["x0"], t["x1"], want_dp1=want),
                                inputs=dict(dp2=i["dp2"], code2=i["code2"], pack=i["pack"], code1=i["code1"], x0=x0, x1=x1))

        @case(f"conv2_bwd_weight-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            return dict(fn=lambda t: ops.simnn_conv2_bwd_weight(t["dp2"], t["code2"], t["p1"]),
                        inputs=dict(dp2=i["dp2"], code2=i["code2"], p1=i["p1"]))

        for _acc in (False, True):
            @case(f"conv1_bwd_weight-{'accumulate' if _acc else 'plain'}-{_id}", acc=_acc, **_k)
            def _c(kind, s, dt, acc):
                i = _trunk(kind, s, dt)
                inputs = dict(dp1=i["dp1"], code1=i["code1"], x=i["x"])
                if not acc:
                    return dict(fn=lambda t: ops.simnn_conv1_bwd_weight(t["dp1"], t["code1"], t["x"]), inputs=inputs)
                inputs.update(dw=_randn(16, 1, 2, 2, seed=5), db=_randn(16, seed=6))

                def fn(t):
                    ops.simnn_conv1_bwd_weight(t["dp1"], t["code1"], t["x"], out=(t["dw"], t["db"]), accumulate=True)
                    return {}
                return dict(fn=fn, inputs=inputs, inout=("dw", "db"))

        @case(f"conv1_bwd_data-{_id}", **_k)
        def _c(kind, s, dt):
            i = _trunk(kind, s, dt)
            h, w = i["x"].shape[1:]
            return dict(fn=lambda t: ops.simnn_conv1_bwd_data(t["dp1"], t["code1"], t["w"], h, w),
                        inputs=dict(dp1=i["dp1"], code1=i["code1"], w=i["w1"]))

for _dt in (F32, BF16):
    @case(f"conv2_pack-{DTN[_dt]}", dt=_dt)
    def _c(dt):
        return dict(fn=lambda t: ops.simnn_conv2_pack(t["w"], dt), inputs=dict(w=_randn(32, 16, 3, 3, seed=2, scale=0.05)))


# ============================================================================== b. fused discriminator of model 2
def _dcnn_params(t, seed=8):
    from test_mmgan_batch_gpu import _params
    return _params(t, seed)


def _dcnn_inputs(B, t, seed):
    from test_mmgan_batch_gpu import _inputs
    return _inputs(B, t, seed, True)


def _dcnn_B(sym):
    return _cap() + 1 if sym == "cap+1" else sym


for _t in (16, 18, 50):
    @case(f"dcnn_pack-T{_t}", t=_t)
    def _c(t):
        ps = _dcnn_params(t)
        names = ("w1", "b1", "w2", "b2", "wfc", "bfc")
        return dict(fn=lambda q: {"pack": ops.dcnn_pack(*[q[n] for n in names], t)}, inputs=dict(zip(names, ps)),
                    entry="gdm_dcnn_pack")

    for _B in (1, 3, "cap+1"):
        for _bs in ((0, 1) if _B == 1 else (0, 1, "B")):
            for _crit in ("bce", "mse"):
                for _want in (True, False):
                    for _acc in (False, True):
                        @case(f"dcnn_fused-T{_t}-B{_B}-bsplit{_bs}-{_crit}-grad{int(_want)}-acc{int(_acc)}", t=_t, B=_B,
                              bs=_bs, crit=_crit, want=_want, acc=_acc)
                        def _c(t, B, bs, crit, want, acc):
                            B = _dcnn_B(B)
                            bs = B if bs == "B" else bs
                            x = _dcnn_inputs(B, t, 61 + t + B)
                            pack = ops.dcnn_pack(*[p.to(DEV).contiguous() for p in _dcnn_params(t)], t)
                            inputs = dict(xa=x[:bs].contiguous() if bs else None,
                                          p0=x[bs:, 0].contiguous() if bs < B else None,
                                          p1=x[bs:, 1].contiguous() if bs < B else None, pack=pack,
                                          loss=torch.full((1,), 1.5) if acc else None)

                            def fn(q):
                                lo = q["loss"] if acc else ops.torch.empty(1, dtype=torch.float32, device=DEV)
                                logits, grads = ops.dcnn_fused(q["xa"], None if q["p0"] is None else (q["p0"], q["p1"]), t,
                                                               0.0, 1.0, q["pack"], loss_out=lo, accumulate_loss=acc,
                                                               want_grad=want, criterion=crit)
                                out = dict(logits=logits, **({} if acc else {"loss_out": lo}))
                                out.update(zip(MR.GRAD_NAMES, grads or ()))
                                return out
                            return dict(fn=fn, inputs=inputs, inout=("loss",) if acc else ())

for _crit in ("bce", "mse"):
    @case(f"dcnn_fused_adam-T50-B3-{_crit}", crit=_crit)
    def _c(crit):
        t, B, bs = 50, 3, 1
        ps = _dcnn_params(t, seed=12)
        x = _dcnn_inputs(B, t, 5)
        inputs = dict(xa=x[:bs].contiguous(), p0=x[bs:, 0].contiguous(), p1=x[bs:, 1].contiguous(),
                      pack=ops.dcnn_pack(*[p.to(DEV).contiguous() for p in ps], t),
                      hyper=ops.adam_hyper("cpu", 0.01, 0.5, 0.999, 1e-8, step=3), done=torch.zeros(1, dtype=torch.int32))
        for i, p in enumerate(ps):
            inputs[f"p{i}_param"] = p
            inputs[f"m{i}"] = _randn(*p.shape, seed=i, scale=1e-3)
            inputs[f"v{i}"] = torch.rand(p.shape, generator=_gen(10 + i)) * 1e-6
        state = tuple(f"{k}{i}{s}" for i in range(6) for k, s in (("p", "_param"), ("m", ""), ("v", "")))

        def fn(q):
            adam = dict(params=[q[f"p{i}_param"] for i in range(6)], exp_avg=[q[f"m{i}"] for i in range(6)],
                        exp_avg_sq=[q[f"v{i}"] for i in range(6)], hyper=q["hyper"], done=q["done"])
            lo = ops.torch.empty(1, dtype=torch.float32, device=DEV)
            logits, grads = ops.dcnn_fused(q["xa"], (q["p0"], q["p1"]), t, 0.0, 1.0, q["pack"], loss_out=lo, adam=adam,
                                           criterion=crit)
            return dict(logits=logits, loss_out=lo, **dict(zip(MR.GRAD_NAMES, grads)))
        return dict(fn=fn, inputs=inputs, inout=state + ("hyper", "done", "pack"),
                    entry="gdm_dcnn_fused_adam" + ("" if crit == "bce" else "_crit"))


# ========================================================================================= c. generator of model 1
def _gen_weights(nd, seed=21):
    g = _gen(seed)
    return [torch.randn(nd, 128, 4, 4, generator=g) * 0.02, torch.randn(128, 64, 4, 4, generator=g) * 0.02,
            torch.randn(64, 32, 4, 4, generator=g) * 0.02, torch.randn(32, 1, 5, 5, generator=g) * 0.05]


def _bn_vecs(c, seed):
    g = _gen(seed)
    return dict(gamma=1 + 0.5 * (2 * torch.rand(c, generator=g) - 1), beta=0.5 * (2 * torch.rand(c, generator=g) - 1),
                rm=torch.randn(c, generator=g) * 0.1, rv=torch.rand(c, generator=g) + 0.5, nbt=torch.tensor(3))


def _gen_pack(nd):
    w = [q.to(DEV) for q in _gen_weights(nd)]
    return ops.simnn_gen_pack(w[0], w[1], w[2])


GEN_LAYER = {2: (128, 64, 4), 3: (64, 32, 8)}          # cin, cout, input height

for _nd in (1, 100):
    @case(f"simnn_gen_pack-nd{_nd}", nd=_nd)
    def _c(nd):
        w = _gen_weights(nd)
        return dict(fn=lambda t: ops.simnn_gen_pack(t["w1"], t["w2"], t["w3"]), inputs=dict(w1=w[0], w2=w[1], w3=w[2]))

    for _B in (2, 5, 256):
        @case(f"simnn_gen_first-B{_B}-nd{_nd}", nd=_nd, B=_B)
        def _c(nd, B):
            v = _bn_vecs(128, B)
            return dict(fn=lambda t: ops.simnn_gen_first(t["noise"], t["pack"], t["rm"], t["rv"], t["nbt"]),
                        inputs=dict(noise=_randn(B, nd, seed=1000 + B), pack=_gen_pack(nd), rm=v["rm"], rv=v["rv"],
                                    nbt=v["nbt"]), inout=("rm", "rv", "nbt"))

for _layer in (2, 3):
    for _B in (2, 5, 129):
        @case(f"simnn_gen_convt_bn-layer{_layer}-B{_B}", layer=_layer, B=_B)
        def _c(layer, B):
            cin, cout, ih = GEN_LAYER[layer]
            v = _bn_vecs(cin, B + layer)
            inputs = dict(yin=_randn(B * ih * ih, cin, seed=B + layer), mean=v["rm"], invstd=v["rv"], gamma=v["gamma"],
                          beta=v["beta"], pack=_gen_pack(100))

            def fn(t):
                yout, part, chunks = ops.simnn_gen_convt_bn(layer, t["yin"], t["mean"], t["invstd"], t["gamma"], t["beta"],
                                                            B, t["pack"])
                assert chunks == _lib.load().gdm_simnn_gen_convt_chunks(layer, B) and part.shape[0] == chunks
                return dict(yout=yout, partials=part)
            return dict(fn=fn, inputs=inputs)

        @case(f"bn_finalize-convt-layer{_layer}-B{_B}", layer=_layer, B=_B)
        def _c(layer, B):
            cin, cout, ih = GEN_LAYER[layer]
            v, w = _bn_vecs(cin, B + layer), _bn_vecs(cout, B)
            _, part, chunks = ops.simnn_gen_convt_bn(layer, _randn(B * ih * ih, cin, seed=B + layer).to(DEV),
                                                     v["rm"].to(DEV), v["rv"].to(DEV), v["gamma"].to(DEV),
                                                     v["beta"].to(DEV), B, _gen_pack(100))
            rows = B * 4 * ih * ih
            return dict(fn=lambda t: ops.bn_finalize(t["part"], chunks, rows, cout, t["rm"], t["rv"], t["nbt"]),
                        inputs=dict(part=part, rm=w["rm"], rv=w["rv"], nbt=w["nbt"]), inout=("rm", "rv", "nbt"))

for _B in (1, 5, 129):
    @case(f"simnn_gen_last-B{_B}", B=_B)
    def _c(B):
        v = _bn_vecs(32, B)
        return dict(fn=lambda t: ops.simnn_gen_last(t["yin"], t["mean"], t["invstd"], t["gamma"], t["beta"], t["w4"], B),
                    inputs=dict(yin=_randn(B * 256, 32, seed=B), mean=v["rm"], invstd=v["rv"], gamma=v["gamma"],
                                beta=v["beta"], w4=_gen_weights(100)[3]))

    for _taps in (False, True):
        @case(f"simnn_gen_eval-B{_B}-taps{int(_taps)}", B=_B, taps=_taps)
        def _c(B, taps):
            inputs = dict(noise=_randn(B, 100, seed=2000 + B), pack=_gen_pack(100), w4=_gen_weights(100)[3])
            for li, c in enumerate((128, 64, 32)):
                v = _bn_vecs(c, 40 + li)
                inputs.update({f"gamma{li}": v["gamma"], f"beta{li}": v["beta"], f"rm{li}": v["rm"], f"rv{li}": v["rv"]})

            def fn(t):
                bns = [(t[f"gamma{li}"], t[f"beta{li}"], t[f"rm{li}"], t[f"rv{li}"]) for li in range(3)]
                return ops.simnn_gen_eval(t["noise"], t["pack"], t["w4"], bns, taps=taps)
            return dict(fn=fn, inputs=inputs)

# the row counts the generator's layers produce: y1 (16 B, 128), y2 (64 B, 64), y3 (256 B, 32)
for _B in (2, 5, 129):
    for _rows, _C in ((16 * _B, 128), (64 * _B, 64), (256 * _B, 32)):
        @case(f"bn_stats-{_rows}x{_C}", rows=_rows, C=_C)
        def _c(rows, C):
            v = _bn_vecs(C, rows)
            return dict(fn=lambda t: ops.bn_stats(t["y"], t["rm"], t["rv"], t["nbt"]),
                        inputs=dict(y=_randn(rows, C, seed=rows + C), rm=v["rm"], rv=v["rv"], nbt=v["nbt"]),
                        inout=("rm", "rv", "nbt"))

        @case(f"bn_partials-{_rows}x{_C}", rows=_rows, C=_C)
        def _c(rows, C):
            return dict(fn=lambda t: ops.bn_partials(t["y"]), inputs=dict(y=_randn(rows, C, seed=rows + C)))

        @case(f"bn_finalize-{_rows}x{_C}", rows=_rows, C=_C)
        def _c(rows, C):
            v = _bn_vecs(C, rows)
            part = ops.bn_partials(_randn(rows, C, seed=rows + C).to(DEV))
            return dict(fn=lambda t: ops.bn_finalize(t["part"], part.shape[0], rows, C, t["rm"], t["rv"], t["nbt"]),
                        inputs=dict(part=part, rm=v["rm"], rv=v["rv"], nbt=v["nbt"]), inout=("rm", "rv", "nbt"))


# ================================================================================= d. Linear + BatchNorm + activation
LB_KEYS = ("x", "w", "bias", "gamma", "beta", "running_mean", "running_var")


def _lb_block(K, N, M, seed, groups=1):
    from test_mmgan_batch_gpu import _block
    return _block(K, N, M, seed, groups=groups)


for _K, _N, _M in ((100, 256, 256), (64, 4096, 16), (64, 20, 33), (37, 33, 31), (37, 1, 2)):
    for _groups in (1, 3):
        for _save in (False, True):
            for _train in (True, False):
                @case(f"linear_bn-K{_K}-N{_N}-M{_M}-groups{_groups}-save_y{int(_save)}-{'train' if _train else 'eval'}",
                      K=_K, N=_N, M=_M, groups=_groups, save=_save, train=_train)
                def _c(K, N, M, groups, save, train):
                    c = _lb_block(K, N, M, 7 * K + N + M + groups, groups)
                    return dict(fn=lambda t: ops.linear_bn_act_fwd(*[t[k] for k in LB_KEYS], t["nbt"], act=ACT_SIGMOID,
                                                                   training=train, save_y=save, groups=groups),
                                inputs=dict(c, nbt=torch.full((), 3, dtype=torch.long)),
                                inout=("running_mean", "running_var", "nbt"))


@case("linear_bn_multi-two-jobs")
def _c():
    """the two-job launch of tests/test_mmgan_batch_gpu.py test_linear_bn_two_jobs_in_one_launch"""
    c1, c2 = _lb_block(100, 256, 256, 41, groups=2), _lb_block(64, 4096, 16, 42)
    inputs = {f"a_{k}": v for k, v in c1.items()}
    inputs.update({f"b_{k}": v for k, v in c2.items()})
    inputs.update(a_nbt=torch.zeros((), dtype=torch.long), b_nbt=torch.zeros((), dtype=torch.long))

    def fn(t):
        j1 = dict({k: t[f"a_{k}"] for k in LB_KEYS}, nbt=t["a_nbt"], groups=2)
        j2 = dict({k: t[f"b_{k}"] for k in LB_KEYS}, nbt=t["b_nbt"], stat_repeats=2)
        (o1, m1, i1), (o2, m2, i2) = ops.linear_bn_act_fwd_multi([j1, j2], act=ACT_SIGMOID)
        return dict(o1=o1, m1=m1, i1=i1, o2=o2, m2=m2, i2=i2)
    return dict(fn=fn, inputs=inputs, inout=tuple(f"{j}_{k}" for j in "ab" for k in ("running_mean", "running_var", "nbt")))


# ======================================================================================== e. lowering and pointwise
def _ops_kw(g):
    return dict(b=g["B"], h=g["H"], w=g["W"], c=g["C"], kh=g["KH"], kw=g["KW"], stride=g["stride"], pad=g["pad"])


for _g in LR.EDGE_GEOMS:
    _gid = _g["name"].replace(" ", "_")
    for _st in TYPES:
        for _ct in TYPES:
            _tt = f"{str(_st)[6:]}-{str(_ct)[6:]}"

            @case(f"im2col-{_gid}-{_tt}", g=_g, st=_st, ct=_ct)
            def _c(g, st, ct):
                src = _randn(g["B"] * g["H"] * g["W"] * g["C"], seed=g["H"] * g["C"], dtype=st)
                return dict(fn=lambda t: ops.im2col(t["src"], planar=g["planar"], out_dtype=GDT[ct], **_ops_kw(g))[0],
                            inputs=dict(src=src))

            @case(f"col2im-{_gid}-{_tt}", g=_g, st=_st, ct=_ct)
            def _c(g, st, ct):
                cols = _randn(g["B"] * g["OH"] * g["OW"], g["C"] * g["KH"] * g["KW"], seed=g["W"] * g["C"], dtype=st)
                return dict(fn=lambda t: ops.col2im(t["cols"], oh=g["OH"], ow=g["OW"], out_dtype=GDT[ct],
                                                    planar=g["planar"], **_ops_kw(g)), inputs=dict(cols=cols))

    for _st in TYPES:
        @case(f"maxpool2-{_gid}-{str(_st)[6:]}", g=_g, st=_st)
        def _c(g, st):
            B, H, W, C = g["B"], g["H"], g["W"], g["C"]
            x = LR.pool_input(B, H, W, C, st).reshape(-1, C)
            d = _randn(B * (H // 2) * (W // 2), C, seed=H, dtype=st)

            def fn(t):
                out, idx = ops.maxpool2_fwd(t["x"], B, H, W, C)
                out2, _ = ops.maxpool2_fwd(t["x"], B, H, W, C, want_idx=False)
                return dict(out=out, idx=idx, out2=out2, dx=ops.maxpool2_bwd(t["d"], idx, B, H, W, C))
            return dict(fn=fn, inputs=dict(x=x, d=d))

PERMUTE = LR.PERMUTE_SHAPES + [(g["B"], g["H"] * g["W"], g["C"]) for g in LR.EDGE_GEOMS[:3]]
assert {LR.permute_kernel(p) for _, p, _ in PERMUTE} == {"narrow", "wide"}
for _B, _P, _C in PERMUTE:
    for _st, _ct in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)):
        @case(f"permute_pc-{LR.permute_kernel(_P)}-{_B}x{_P}x{_C}-{str(_st)[6:]}-{str(_ct)[6:]}", B=_B, P=_P, C=_C, st=_st,
              ct=_ct)
        def _c(B, P, C, st, ct):
            return dict(fn=lambda t: ops.permute_pc(t["src"], B, P, C, out_dtype=GDT[ct]),
                        inputs=dict(src=_randn(B, P, C, seed=P + C, dtype=st)))

# one shape on each side of every boundary tests/test_pointwise_edges_gpu.py tabulates (lowering_ref's tables); the
# 65536-row pairs repeat the capped-chunks regime of the 16385-row ones
BN_PAIRS = [p for p in LR.BN_PAIRS if p[0] <= 16385]
assert {LR.row_chunks(r) for r, _ in BN_PAIRS} >= {1, 2, 3, 64} and any((r + 255) // 256 > 64 for r, _ in BN_PAIRS)
for _rows, _C in BN_PAIRS:
    for _ot in TYPES:
        _k = dict(rows=_rows, C=_C, ot=_ot)
        _id = f"{_rows}x{_C}-{str(_ot)[6:]}"
        for _train in (True, False):
            @case(f"bn_act_fwd-{'train' if _train else 'eval'}-{_id}", train=_train, **_k)
            def _c(rows, C, ot, train):
                v = _bn_vecs(C, rows + C)
                return dict(fn=lambda t: ops.bn_act_fwd(t["y"], t["gamma"], t["beta"], t["rm"], t["rv"], t["nbt"],
                                                        act=ACT_RELU, out_dtype=GDT[ot], training=train),
                            inputs=dict(v, y=_randn(rows, C, seed=rows * 131 + C, scale=2.0)), inout=("rm", "rv", "nbt"))

        @case(f"bn_apply-{_id}", **_k)
        def _c(rows, C, ot):
            v = _bn_vecs(C, rows + C)
            return dict(fn=lambda t: ops.bn_apply(t["y"], t["gamma"], t["beta"], t["rm"], t["rv"], act=ACT_SIGMOID,
                                                  out_dtype=GDT[ot]),
                        inputs=dict(y=_randn(rows, C, seed=rows + C), gamma=v["gamma"], beta=v["beta"], rm=v["rm"], rv=v["rv"]))

        @case(f"bn_act_bwd-{_id}", **_k)
        def _c(rows, C, ot):
            v = _bn_vecs(C, rows + C)
            y = _randn(rows, C, seed=rows + C)
            out = torch.relu(y * v["gamma"] + v["beta"]).to(ot)
            return dict(fn=lambda t: ops.bn_act_bwd(t["dout"], t["out"], t["y"], t["gamma"], t["rm"], t["rv"], act=ACT_RELU),
                        inputs=dict(dout=_randn(rows, C, seed=rows, dtype=ot), out=out, y=y, gamma=v["gamma"], rm=v["rm"],
                                    rv=v["rv"]))

for _rows in LR.COLSUM_ROWS:
    for _cols in LR.COLSUM_COLS:
        for _st in TYPES:
            @case(f"colsum-{_rows}x{_cols}-{str(_st)[6:]}", rows=_rows, cols=_cols, st=_st)
            def _c(rows, cols, st):
                return dict(fn=lambda t: ops.colsum(t["x"]), inputs=dict(x=_randn(rows, cols, seed=rows + cols, dtype=st)))

for _rows, _cols in LR.BIAS_ACT_SHAPES:
    for _act in (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID):
        for _ot in TYPES:
            @case(f"bias_act-{_rows}x{_cols}-act{_act}-{str(_ot)[6:]}", rows=_rows, cols=_cols, act=_act, ot=_ot)
            def _c(rows, cols, act, ot):
                def fn(t):
                    out = ops.bias_act_fwd(t["x"], t["bias"], act=act, slope=0.2, out_dtype=GDT[ot])
                    return dict(out=out, dx=ops.act_bwd(t["d"], out, act=act, slope=0.2))
                return dict(fn=fn, inputs=dict(x=_randn(rows, cols, seed=rows, scale=3.0), bias=_randn(cols, seed=cols),
                                               d=_randn(rows, cols, seed=act + 5, dtype=ot)))

for _n in LR.ADAM_N:
    for _st, _ct in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)):
        @case(f"cast-{_n}-{str(_st)[6:]}-{str(_ct)[6:]}", n=_n, st=_st, ct=_ct)
        def _c(n, st, ct):
            return dict(fn=lambda t: ops.cast(t["x"], GDT[ct]), inputs=dict(x=_randn(n, seed=n, scale=1e3, dtype=st)))

for _n in LR.ADAM_N:
    for _dev in (False, True):
        @case(f"adam_step{'_dev' if _dev else ''}-{_n}", n=_n, dev=_dev)
        def _c(n, dev):
            inputs = dict(p=_randn(n, seed=n % 100000), g=_randn(n, seed=n % 100000 + 1, scale=0.1),
                          m=_randn(n, seed=n % 100000 + 2, scale=1e-2), v=torch.rand(n, generator=_gen(3)) * 1e-4)
            if not dev:
                def fn(t):
                    ops.adam_step(t["p"], t["g"], t["m"], t["v"], 4, 2e-5, 0.5, 0.999, 1e-8, 0.125)
                    return {}
                return dict(fn=fn, inputs=inputs, inout=("p", "m", "v"))
            inputs["hyper"] = ops.adam_hyper("cpu", 2e-5, 0.5, 0.999, 1e-8, 0.125, step=3)

            def fn(t):
                ops.adam_step_dev(t["p"], t["g"], t["m"], t["v"], t["hyper"])
                return {}
            return dict(fn=fn, inputs=inputs, inout=("p", "m", "v", "hyper"))


def _logits(n, seed):
    x = _randn(n, seed=seed, scale=3.0)
    edge = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0])
    x[:min(n, 5)] = edge[:min(n, 5)]
    return x


for _n in LR.LOSS_N:
    for _want in (True, False):
        for _acc in (False, True):
            @case(f"bce_with_logits-{_n}-grad{int(_want)}-acc{int(_acc)}", n=_n, want=_want, acc=_acc)
            def _c(n, want, acc):
                def fn(t):
                    loss, dx = ops.bce_with_logits(t["x"], 0.9, grad_scale=0.5, want_grad=want, loss_out=t["loss"],
                                                   accumulate_loss=acc)
                    return dict(dx=dx, **({} if acc else {"loss_out": loss}))
                return dict(fn=fn, inputs=dict(x=_logits(n, n + 1), loss=torch.full((1,), 1.5) if acc else None),
                            inout=("loss",) if acc else ())

            for _crit in ("bce", "mse", "l1"):
                @case(f"criterion_loss-{_crit}-{_n}-grad{int(_want)}-acc{int(_acc)}", n=_n, want=_want, acc=_acc, crit=_crit)
                def _c(n, want, acc, crit):
                    def fn(t):
                        lo = t["loss"] if acc else ops.torch.empty(1, dtype=torch.float32, device=DEV)
                        _, dx = ops.criterion_loss(t["x"], 0.9, crit, loss_out=lo, accumulate_loss=acc, want_grad=want,
                                                   grad_scale=0.5)
                        return dict(dx=dx, **({} if acc else {"loss_out": lo}))
                    return dict(fn=fn, inputs=dict(x=_logits(n, n + 1), loss=torch.full((1,), 1.5) if acc else None),
                                inout=("loss",) if acc else ())

    @case(f"bce_with_logits-fused-sigmoid-{_n}", n=_n)
    def _c(n):
        return dict(fn=lambda t: ops.bce_with_logits(t["x"], 0.0, fuse_sigmoid_backward=True),
                    inputs=dict(x=torch.sigmoid(_logits(n, n))))

for _n, _n0 in LR.HEAD_N:
    for _dh in TYPES:
        for _want, _acc in ((True, True), (True, False), (False, False)):
            @case(f"simnn_head-{_n}-{_n0}-{str(_dh)[6:]}-grad{int(_want)}-acc{int(_acc)}", n=_n, n0=_n0, dh=_dh, want=_want,
                  acc=_acc)
            def _c(n, n0, dh, want, acc):
                g = _gen(n)
                inputs = dict(h1=torch.relu(torch.randn(n, 128, generator=g)), w2=torch.randn(1, 128, generator=g) * 0.2,
                              b2=torch.randn(1, generator=g), loss=torch.full((1,), 1.5) if acc else None)

                def fn(t):
                    lo = t["loss"] if acc else ops.torch.empty(1, dtype=torch.float32, device=DEV)
                    prob, dh1, grads = ops.simnn_head(t["h1"], t["w2"], t["b2"], n0, 0.9, 0.1, loss_out=lo,
                                                      accumulate_loss=acc, want_grad=want, dh_dtype=GDT[dh])
                    out = dict(prob=prob, dh1=dh1, **({} if acc else {"loss_out": lo}))
                    out.update(zip(("dw2", "db2", "db1"), grads or ()))
                    return out
                return dict(fn=fn, inputs=inputs, inout=("loss",) if acc else ())


@case("concat_cols_multi-three-pairs")
def _c():
    m = 33
    return dict(fn=lambda t: ops.concat_cols_multi([(t["a"], t["b"]), (t["b"], t["a"]), (t["a"], t["c"])]),
                inputs=dict(a=_randn(m, 50, seed=1), b=_randn(m, 50, seed=2), c=_randn(m, 7, seed=3)))


for _n in LR.LOSS_N:
    for _st in TYPES:
        @case(f"nonfinite_count-{_n}-{str(_st)[6:]}", n=_n, st=_st)
        def _c(n, st):
            x = _randn(n, seed=n)
            x[::7] = float("inf")
            x[n - 1] = float("nan")

            def fn(t):
                ops.nonfinite_count([t["x"]], t["counter"])
                return {}
            return dict(fn=fn, inputs=dict(x=x.to(st), counter=torch.full((1,), 2, dtype=torch.int32)), inout=("counter",))

# ops.gemm at the split-K cases of gemm_ref.GUARD_CASES (C already sits between sentinel rows there; the workspace is new)
for _gc in [c for c in GR.GUARD_CASES if "split" in c.name]:
    @case(f"gemm-{_gc.name}", c=_gc)
    def _c(c):
        t = GR.materialize(c, GR.inputs(c, "exact"), "cpu")
        assert GR.plan_of(c)["split_k"] > 1
        views = {k: (t[k].shape, t[k].stride(), t[k].storage_offset()) for k in ("a", "b", "out")}
        inputs = dict(a=t["a"]._base, b=t["b"]._base, cbuf=t["cbuf"],
                      bias_n=None if t["bias_n"] is None else t["bias_n"]._base, bias_m=t["bias_m"])
        bias_off = c.bias_off

        def fn(q):
            a, b, out = (torch.as_strided(q[k], views[n][0], views[n][1], q[k].storage_offset() + views[n][2])
                         for k, n in (("a", "a"), ("b", "b"), ("cbuf", "out")))
            ops.gemm(a, b, bias_n=None if q["bias_n"] is None else q["bias_n"][bias_off:], bias_m=q["bias_m"], act=c.act,
                     slope=c.slope, compute=c.comp, split_k=c.split, out=out)
            return {}
        return dict(fn=fn, inputs=inputs, inout=("cbuf",))


# ======================================================== f. device entries without a guarded test in another file
for _route, _b, _s, _dim, _kw in (("midi", 3, 64, 61, dict(note_mod=True)),
                                  ("wav", 3, 20, 15, dict(threshold=0.75, norm_aux=True))):
    def _matrices(b, s):
        r = np.random.RandomState(1000 + b + s)
        m = (1.0 / (1.0 + np.exp(-r.standard_normal((b, s, s))))).astype(np.float32)
        m[r.random_sample(m.shape) < 0.02] = 0.0
        return torch.from_numpy(m)

    @case(f"des_scan-{_route}", b=_b, s=_s, dim=_dim, kw=_kw)
    def _c(b, s, dim, kw):
        return dict(fn=lambda t: ops.des_scan(t["g"], s, dim, **kw), inputs=dict(g=_matrices(b, s)))

    @case(f"des_routing-{_route}", b=_b, s=_s, dim=_dim)
    def _c(b, s, dim):
        r = np.random.RandomState(b + dim)
        src = np.zeros((b, dim), np.uint8)
        src[:, 3] = 1
        cols = r.randint(0, dim, (b, dim)).astype(np.int32)
        return dict(fn=lambda t: ops.des_routing(t["g"], s, dim, t["src"], t["cols"]),
                    inputs=dict(g=_matrices(b, s), src=torch.from_numpy(src), cols=torch.from_numpy(cols)))


@case("des_pack-B300")
def _c():
    B, cap = 300, 7                      # more samples than one pass of the scan holds
    r = np.random.RandomState(4)
    n = B * cap
    inputs = dict(n_records=torch.from_numpy(r.randint(0, cap + 1, B).astype(np.int64)),
                  rec_ptr=torch.zeros(B + 1, dtype=torch.int64), value=torch.from_numpy(r.standard_normal(n)),
                  event_id=torch.arange(n, dtype=torch.int64), node=torch.from_numpy(r.randint(0, 9, n).astype(np.int32)),
                  kind=torch.from_numpy(r.randint(0, 3, n).astype(np.int32)))

    def fn(t):
        ops.des_pack(t["n_records"], t["rec_ptr"], t["value"], t["event_id"], t["node"], t["kind"], cap)
        return {}
    return dict(fn=fn, inputs=inputs, inout=("rec_ptr", "value", "event_id", "node", "kind"))


@case("piano_roll_raster-3-files")
def _c():
    files, width = 3, 50
    r = np.random.RandomState(9)
    counts = r.randint(0, 7, files * 128)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    steps = np.concatenate([np.sort(r.randint(0, width + 5, c)) for c in counts]).astype(np.int32)
    vel = np.where(r.random_sample(steps.size) < 0.5, r.randint(1, 128, steps.size), -1).astype(np.int32)
    return dict(fn=lambda t: ops.piano_roll_raster(t["row_ptr"], t["ev_step"], t["ev_vel"], files, width),
                inputs=dict(row_ptr=torch.from_numpy(row_ptr), ev_step=torch.from_numpy(steps), ev_vel=torch.from_numpy(vel)))


for _window in ((0, 50), (100, 150)):
    @case(f"des_log_to_roll-golden-{_window[0]}-{_window[1]}", window=_window)
    def _c(window):
        from gan_des_midi_music_gen_amd.sim_log_to_midi import MAX_LINES, _int_rows
        from test_des_midi_gpu import golden_batch
        logs, tails, inst, notes, save = golden_batch()
        heads = [lg[:MAX_LINES] for lg in logs]
        rec_ptr = np.zeros(len(logs) + 1, dtype=np.int64)
        np.cumsum([len(h) for h in heads], out=rec_ptr[1:])
        rec = np.concatenate(heads)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        names = ("value", "event_id", "node", "kind")
        inputs = dict({k: up(rec[k]) for k in names}, rec_ptr=up(rec_ptr), tails=up(np.asarray(tails, dtype=np.float32)),
                      inst=up(_int_rows(inst, "instruments")), notes=up(_int_rows(notes, "note_levels")),
                      save=up(np.asarray(save, dtype=np.int32)))
        return dict(fn=lambda t: ops.des_log_to_roll(*[t[k] for k in names], t["rec_ptr"], t["tails"], t["inst"], t["notes"],
                                                     t["save"], *window),
                    inputs=inputs)


@case("des_math_probe-edges")
def _c():
    from test_des_batch_gpu import edge_inputs
    return dict(fn=lambda t: ops.des_math_probe(t["x"]), inputs=dict(x=torch.from_numpy(edge_inputs(10000))))


for _label in ("edges-n513", "mixed"):
    @case(f"des_log_tracks-{_label}", label=_label)
    def _c(label):
        """gdm_des_log_tracks_count and gdm_des_log_tracks through the wrapper (its one read-back sizes ``tracks``)"""
        from gan_des_midi_music_gen_amd import simlog_to_vid as sl
        import test_simlog_to_vid_gpu as SV
        if label == "mixed":
            _l, logs, servers, dim, max_lines = next(g for g in SV.GROUPS if g[0] == "mixed dim 3")
        else:
            log, srv, dim, max_lines, _st = SV.EDGE_LOGS["n513"]
            logs, servers = [log], [srv]
        b = SV.batch_of(logs)
        col, n_cols = sl._columns(np.asarray(servers), len(logs), dim)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        return dict(fn=lambda t: ops.des_log_tracks(t["node"], t["kind"], t["rec_ptr"], t["col"], n_cols,
                                                    max_lines=max_lines),
                    inputs=dict(node=up(b.node), kind=up(b.kind), rec_ptr=up(b.rec_ptr), col=up(col)))


for _pc in (False, True):
    @case(f"des_log_to_notes{'_pc' if _pc else ''}-crafted-logs", pc=_pc)
    def _c(pc):
        """the crafted logs of tests/golden/des_notes.npz, all in one launch (tests/test_sim_to_wav_gpu.py)"""
        import os
        from helpers import GOLDEN
        fields = ("value", "event_id", "node", "kind")
        with np.load(os.path.join(GOLDEN, "des_notes.npz")) as z:
            names = [str(n) for n in z["names"] if f"{n}/value" in z.files]
            logs = [{k: z[f"{n}/{k}"] for k in fields} for n in names]
            inst = np.stack([z[f"{n}/instruments"] for n in names]).astype(np.int32)
            levels = np.stack([z[f"{n}/note_levels"] for n in names]).astype(np.int32)
        ptr = np.concatenate([[0], np.cumsum([len(lg["value"]) for lg in logs])]).astype(np.int64)
        dts = dict(value=np.float64, event_id=np.int64, node=np.int32, kind=np.int32)
        inputs = {k: torch.from_numpy(np.concatenate([lg[k] for lg in logs]).astype(dts[k])) for k in fields}
        inputs.update(rec_ptr=torch.from_numpy(ptr), inst=torch.from_numpy(inst), levels=torch.from_numpy(levels))
        if pc:
            return dict(fn=lambda t: ops.des_log_to_notes_pc(*[t[k] for k in fields], t["rec_ptr"], t["inst"], t["levels"]),
                        inputs=inputs)
        del inputs["inst"]
        return dict(fn=lambda t: ops.des_log_to_notes(*[t[k] for k in fields], t["rec_ptr"], t["levels"]), inputs=inputs)


def _gen_eval_names():
    import mmgan_gen_eval_ref as ER
    return sorted(ER.GEOMETRIES)


for _name in _gen_eval_names():
    @case(f"mmgan_gen_eval_pack-{_name}", name=_name)
    def _c(name):
        """the pointer arrays of the wrapper bypass ops._p; the 24 tensors they name are this case's inputs, so they
        lie in the arena all the same"""
        import mmgan_gen_eval_ref as ER
        keys = ("w",) + tuple(ER.VEC_NAMES)
        params = ER.make_params(name)
        inputs = {f"{k}{i}": p[k] for i, p in enumerate(params) for k in keys}
        return dict(fn=lambda t: ops.mmgan_gen_eval_pack([tuple(t[f"{k}{i}"] for k in keys) for i in range(4)],
                                                         eps=ER.EPS)[0], inputs=inputs)


def _db_cases():
    import mel_ref as MEL
    return MEL.DB_CASES + MEL.DB_MANY_WINDOWS + MEL.DB_LDS_FITS


for _dc in _db_cases():
    @case(f"power_to_db-{_dc.frames}x{_dc.n_mels}-B{_dc.B}-top{_dc.top_db}", c=_dc)
    def _c(c):
        import mel_ref as MEL
        return dict(fn=lambda t: ops.power_to_db(t["p"], c.B, c.frames, top_db=c.top_db), inputs=dict(p=MEL.db_input(c)))


# =========================================================================================================== the run
@pytest.mark.parametrize("cid,build", CASES, ids=[c[0] for c in CASES])
def test_guarded(cid, build):
    if _t0[0] is None:
        _t0[0] = time.perf_counter()
    assert not TR.plan_env_overrides(), TR.plan_env_overrides()
    spec = build()
    try:
        G.run_case(spec["fn"], spec["inputs"], spec.get("inout", ()), device=DEV, entry=spec.get("entry"))
    except RuntimeError as e:
        if "hip" in str(e).lower():          # a device fault is sticky: start nothing more on this device
            pytest.exit(f"{cid}: {e}", returncode=3)
        raise
    _ran.add(cid)


def test_the_harness_catches_the_four_faults_on_the_device_too():
    """tests/test_guarded.py's fake wrappers (plain torch, one element past a tensor inside the harness's own buffers)
    with the arena on the GPU: the device path of the harness fails when it should."""
    import test_guarded as TG
    want = [(TG.fake_stores_past_output, "wrote-outside", "_prologue:out"), (TG.fake_reads_past_input, "reads-outside-input", "x"),
            (TG.fake_leaves_one_unwritten, "unwritten", "out"), (TG.fake_reads_stale_workspace, "reads-stale-workspace", "workspace")]
    G.run_case(lambda t: TG.fake_ok(t["x"]), {"x": TG._x()}, mod=TG.NS, device=DEV)
    for fake, kind, tensor in want:
        with pytest.raises(G.GuardError) as e:
            G.run_case(lambda t: fake(t["x"]), {"x": TG._x()}, mod=TG.NS, device=DEV)
        assert (e.value.kind, e.value.tensor) == (kind, tensor), str(e.value)


def test_case_ids_are_unique():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))


def test_covered_is_what_the_cases_reached():
    """COVERED equals the library entries ``_call`` saw during the cases (when all of them ran in this session)."""
    seen = {n for n in G.CALLED if n.startswith("gdm_")}
    prep = seen - COVERED
    if len(_ran) == len(CASES):
        assert seen >= COVERED, sorted(COVERED - seen)
        seconds = time.perf_counter() - _t0[0]
        record("buffer_bounds", seconds=round(seconds, 1), cases=len(CASES))
    assert not prep, f"entries reached but not declared in COVERED: {sorted(prep)}"
