"""CPU: the shape table of tests/test_simnn_trunk_batch_gpu.py reaches every work-plan regime of the conv trunk kernels;
the float64 checker of tests/trunk_ref.py flags each kind of subtle kernel fault; the code decoders round-trip.

The fused / weight-gradient workgroup counts come from the library's host-only workspace functions (no GPU needed);
the other plans are Python mirrors that cite the C++ they restate (trunk_ref.py).
"""
import pytest
import torch

import trunk_ref as tr
from trunk_ref import SHAPES, gemm_path

from gan_des_midi_music_gen_amd.ops import BF16, F32


@pytest.fixture(scope="module")
def lib():
    assert not tr.plan_env_overrides(), (f"GDM_* plan overrides are set ({tr.plan_env_overrides()}): the kernels "
                                         "would not run the shipped plan")
    from gan_des_midi_music_gen_amd import build, _lib
    build.build()
    return _lib.load()


def _plans(lib, b, h, w):
    h1, w1 = (h + 1) // 2, (w + 1) // 2
    fused = tr.bd_plan(b, h1, w1, True)
    bw = tr.bw_plan(b, h1, w1)
    # the library's own plan: workgroups = workspace bytes / slab bytes - 65 (the *_workspace_bytes
    # functions of simnn_conv2_bwd_data.hip, simnn_conv2_bwd_weight.hip and simnn_conv1.hip)
    assert lib.gdm_simnn_conv2_bwd_fused_workspace_bytes(b, h1, w1) // 320 - 65 == fused["blocks"]
    assert lib.gdm_simnn_conv2_bwd_weight_workspace_bytes(b, h1, w1) // 18560 - 65 == bw["blocks"]
    assert lib.gdm_simnn_conv1_bwd_weight_workspace_bytes(b, h, w) // 320 - 65 == tr.conv1_slabs(b, h, w)
    return dict(fused=fused, bd=tr.bd_plan(b, h1, w1, False), bw=bw, c2f=tr.c2f_plan(b, h1, w1),
                c1=tr.conv1_fwd_blocks(b, h), slabs=tr.conv1_slabs(b, h, w), c1bd=tr.conv1_bwd_data_blocks(b, h, w),
                h1=h1, w1=w1)


def test_plan_environment_is_the_shipped_one():
    assert not tr.plan_env_overrides(), (f"GDM_* plan overrides are set ({tr.plan_env_overrides()}): the kernels "
                                         "would not run the shipped plan")


def test_shape_table_reaches_every_regime(lib):
    P = {(b, h, w): _plans(lib, b, h, w) for (b, h, w, _, _) in SHAPES}
    bsplit = {(b, h, w): bs for (b, h, w, bs, _) in SHAPES}
    # the two production launches
    assert P[(512, 128, 256)]["fused"]["n_items"] == 1024 and P[(512, 128, 256)]["fused"]["blocks"] == 512
    assert bsplit[(512, 128, 256)] == 256
    assert P[(256, 128, 256)]["bw"] == dict(P[(256, 128, 256)]["bw"], n_items=1024, nseg=2, blocks=768)
    assert P[(512, 128, 256)]["c2f"]["n_tiles"] == 16384 and P[(512, 128, 256)]["c2f"]["grid"] == 768
    # the reference geometry, B and B/2 per input tensor
    assert (256, 128, 216) in P and bsplit[(32, 128, 216)] == 16
    # items == cap exactly, and cap + 2
    assert P[(256, 128, 256)]["fused"]["n_items"] == tr.BD_CAP_FUSE
    assert P[(257, 128, 256)]["fused"]["n_items"] in (tr.BD_CAP_FUSE + 1, tr.BD_CAP_FUSE + 2)
    # >= 2 items per workgroup with an uneven tail (fused and weight-gradient plans)
    multi = [k for k, p in P.items() if p["fused"]["n_items"] >= 2 * p["fused"]["blocks"]
             and p["fused"]["n_items"] % p["fused"]["blocks"]]
    assert len(multi) >= 2, multi
    assert any(p["bw"]["n_items"] >= 2 * p["bw"]["blocks"] and p["bw"]["n_items"] % p["bw"]["blocks"]
               for p in P.values())
    # row segments together with wrap and a short last segment
    seg = [k for k, p in P.items() if p["fused"]["nseg"] > 1 and p["fused"]["n_items"] > p["fused"]["blocks"]
           and p["fused"]["last_seg_len"] < p["fused"]["seg_len"]]
    assert seg, "no shape has row segments + wrap + a short last segment"
    p = P[(130, 40, 130)]["fused"]
    assert (p["nrq"], p["seg_len"], p["last_seg_len"]) == (5, 3, 2) and p["n_items"] > 512, p
    # conv2 forward: tiles > 768, XCD remap, an odd tile left after the pair rounds
    assert any(p["c2f"]["n_tiles"] > tr.C2F_CAP and p["c2f"]["xcd_remap"] and p["c2f"]["odd_tail"] for p in P.values())
    assert any(p["c2f"]["grid"] % 8 for p in P.values()), "no shape keeps tile id = workgroup id"
    # conv1 forward rows beyond the grid (6144 = 1536 x 4), conv1_slabs at its cap, conv1 input-gradient blocks capped
    big = P[(512, 128, 256)]
    assert big["c1"]["n_rows"] > 4 * tr.C1_CAP and big["c1"]["blocks"] == tr.C1_CAP
    assert big["slabs"] == tr.C1_SLABS_CAP and big["c1bd"] == tr.C1BD_CAP
    # odd H1 and W1, a partial last column tile
    odd = [k for k, p in P.items() if p["h1"] % 2 and p["w1"] % 2 and p["w1"] % tr.BD_COLS]
    assert odd, "no shape with odd H1 and W1 and a partial column tile"
    assert any(p["w1"] % 2 and p["w1"] % tr.BD_COLS == 1 for p in P.values())
    # the fp32 backward (one register set, one step of look-ahead: AHEAD2 false) meets the multi-item and segmented
    # plans: the GPU file runs every shape of the table in every dtype of tr.DTYPES
    assert "fp32" in tr.DTYPES and "bf16" in tr.DTYPES


SWEEP_B = list(range(1, 41)) + [48, 64, 96, 100, 127, 128, 129, 192, 200, 255, 256, 257, 300, 384, 400, 511, 512, 513, 600]
SWEEP_HW = [(128, 256), (128, 216), (128, 64), (40, 130), (5, 7), (4, 4)]


def test_plan_sweep_library_equals_mirror(lib):
    """The one segment plan of csrc/simnn_trunk.h (seg_plan, behind the three host-only *_workspace_bytes functions) and
    conv1_slabs give the workgroup counts of trunk_ref's mirrors for every batch size up to 40, around 256 and 512 and
    up to 600, at the production, reference, narrow, segmented and tiny geometries."""
    for h, w in SWEEP_HW:
        h1, w1 = (h + 1) // 2, (w + 1) // 2
        for b in SWEEP_B:
            got = (lib.gdm_simnn_conv2_bwd_fused_workspace_bytes(b, h1, w1) // 320 - 65,
                   lib.gdm_simnn_conv2_bwd_weight_workspace_bytes(b, h1, w1) // 18560 - 65,
                   lib.gdm_simnn_conv1_bwd_weight_workspace_bytes(b, h, w) // 320 - 65)
            want = (tr.bd_plan(b, h1, w1, True)["blocks"], tr.bw_plan(b, h1, w1)["blocks"], tr.conv1_slabs(b, h, w))
            assert got == want, (b, h, w, got, want)


def test_fc1_gemm_paths():
    """The long-K fc1 products split K and take the deep variant; K = 55296 ends in a short slab (mirrors of
    ops.default_split_k, gemm.hip gemm_plan, gemm_bf16.hip gdm_gemm_bf16_fast_deep)."""
    for m, k in ((512, 65536), (256, 65536), (256, 55296), (32, 55296)):
        p = gemm_path(m, 128, k, BF16)
        assert p["split"] > 1 and p["fast"] and p["variant"] == 1, (m, k, p)
        assert gemm_path(m, 128, k, F32)["split"] > 1
    assert gemm_path(512, 128, 65536, BF16)["split"] == 64
    assert gemm_path(256, 128, 65536, BF16)["split"] == 128
    p = gemm_path(256, 128, 55296, BF16)
    assert p["last_tiles"] < p["per_tiles"], p


# ----------------------------------------------------------------------------------------- checker self-test
def _conv2_case(seed=3, b=3, h1=20, w1=70):
    g = torch.Generator().manual_seed(seed)
    p1 = torch.relu(torch.randn(b, h1, w1, 16, generator=g)).bfloat16()
    w2 = (torch.randn(32, 16, 3, 3, generator=g) * 0.05).bfloat16().float()
    b2 = torch.randn(32, generator=g) * 0.1
    vw, mw = tr.conv2_windows(p1, w2, b2)
    return p1, w2, b2, vw, mw


def _expect_flag(fn):
    with pytest.raises(tr.CheckError):
        fn()


def test_checker_flags_every_mutation():
    b, h1, w1 = 3, 20, 70
    p1, w2, b2, vw, mw = _conv2_case(b=b, h1=h1, w1=w1)
    ref, mag = tr.pool(vw, mw)
    got = ref.float().bfloat16()                                   # a kernel output rounded like the kernel's
    where = tr.where_c2f(b, h1, w1)
    chk = lambda t: tr.check_elementwise(t, ref, mag, rtol=tr.RTOL, out_dtype=torch.bfloat16, where=where)  # noqa
    assert chk(got) <= 1.0
    # one element moved by 4 bf16 ulps (at the largest element, where 4 ulps exceed rtol * M)
    i = tuple(int(v) for v in torch.unravel_index(ref.abs().argmax(), ref.shape))
    bad = got.float().clone()
    bad[i] += 4 * float(tr.ulp(ref[i], torch.bfloat16))
    _expect_flag(lambda: chk(bad))
    # one conv2 forward tile's outputs scaled by 1.01 (tile 1: image 0, pooled rows 0-1, pooled columns 32..)
    bad = got.float().clone()
    bad[0, 0:2, 32:64] *= 1.01
    with pytest.raises(tr.CheckError, match="tile 1 of"):
        chk(bad)

    # code checks: decoded kernel codes = the float64 argmax, encoded and decoded again
    pos = vw.argmax(-1)
    live = vw.max(-1).values > 0
    p_k, l_k, ok = tr.decode_code2(tr.encode_code2(pos, live))
    assert ok
    tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where, pos_when_dead=False)
    # one window's argmax moved to its second-largest position (a live window with a clear gap)
    top2 = vw.topk(2, dim=-1)
    gap = top2.values[..., 0] - top2.values[..., 1]
    j = tuple(int(v) for v in torch.unravel_index((gap * live).argmax(), gap.shape))
    p_bad = pos.clone()
    p_bad[j] = top2.indices[j][1]
    p_k, l_k, _ = tr.decode_code2(tr.encode_code2(p_bad, live))
    _expect_flag(lambda: tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where, pos_when_dead=False))
    # two channels' codes swapped in one pixel
    both = live[..., :, None] & live[..., None, :] & (pos[..., :, None] != pos[..., None, :])
    pix = both.flatten(3).any(-1).nonzero()[0]
    ca, cb = [int(v) for v in both[tuple(pix)].nonzero()[0]]
    p_bad = pos.clone()
    p_bad[tuple(pix) + (ca,)], p_bad[tuple(pix) + (cb,)] = pos[tuple(pix) + (cb,)], pos[tuple(pix) + (ca,)]
    p_k, l_k, _ = tr.decode_code2(tr.encode_code2(p_bad, live))
    _expect_flag(lambda: tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where, pos_when_dead=False))

    # data gradient: one whole plan item scaled by 1.01, the last row of the last segment zeroed
    g = torch.Generator().manual_seed(9)
    dp2 = (torch.randn(b, h1 // 2, w1 // 2, 32, generator=g) * 0.1).bfloat16()
    dref, dmag = tr.conv2_bwd_data_ref(dp2, pos, live, w2, h1, w1)
    dgot = dref.float().bfloat16()
    wbd = tr.where_bd(b, h1, w1, True)
    dchk = lambda t: tr.check_elementwise(t, dref, dmag, rtol=tr.RTOL_BD, out_dtype=torch.bfloat16, where=wbd)  # noqa
    assert dchk(dgot) <= 1.0
    pl = tr.bd_plan(b, h1, w1, True)
    assert pl["nseg"] > 1                                   # (3, 20, 70): 6 strips, 5 steps in segments of 3 + 2
    bad = dgot.float().clone()
    bad[1, 0:4 * pl["seg_len"], 64:] *= 1.01                 # item (image 1, segment 0, column tile 1)
    item = (1 * pl["nseg"] + 0) * pl["n_ctiles"] + 1
    with pytest.raises(tr.CheckError, match=f"item {item} "):
        dchk(bad)
    bad = dgot.float().clone()
    bad[b - 1, h1 - 1] = 0.0
    with pytest.raises(tr.CheckError, match=f"segment {pl['nseg'] - 1}"):
        dchk(bad)

    # weight gradient: one tap off by 1e-4 of its magnitude
    dw, db, mdw, mdb = tr.conv2_bwd_weight_ref(dp2, pos, live, p1)
    got_w = dw.float()
    wchk = lambda t: tr.check_elementwise(t, dw, mdw, rtol=tr.RTOL_DW, out_dtype=torch.float32,  # noqa
                                          where=tr.where_tap("dw2"))
    assert wchk(got_w) <= 1.0
    bad = got_w.clone()
    bad[5, 7, 1, 2] += 1e-4 * float(mdw[5, 7, 1, 2])
    with pytest.raises(tr.CheckError, match=r"dw2\[5, 7, 1, 2\]"):
        wchk(bad)


def test_conv1_code_check_flags_a_moved_argmax_and_a_wrong_live_bit():
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(2, 9, 13, generator=g) * 18 - 35).clamp(-80, 30)
    w1 = torch.randn(16, 1, 2, 2, generator=g) * 0.1
    b1 = torch.randn(16, generator=g) * 0.5 + 2.0
    vw, mw = tr.conv1_windows(x, w1, b1)
    pos, live = vw.argmax(-1), vw.max(-1).values > 0
    where = tr.where_rows(2, 5)
    p_k, l_k, ok = tr.decode_code1(tr.encode_code1(pos, live), 7)
    assert ok
    ties, n = tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where)
    assert n == 2 * 5 * 7 * 16
    top2 = vw.topk(2, dim=-1)
    gap = top2.values[..., 0] - top2.values[..., 1]
    j = tuple(int(v) for v in torch.unravel_index(gap.argmax(), gap.shape))
    p_bad = pos.clone()
    p_bad[j] = top2.indices[j][1]
    p_k, l_k, _ = tr.decode_code1(tr.encode_code1(p_bad, live), 7)
    _expect_flag(lambda: tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where))
    k = tuple(int(v) for v in torch.unravel_index(vw.max(-1).values.abs().argmax(), live.shape))
    l_bad = live.clone()
    l_bad[k] = ~l_bad[k]
    p_k, l_k, _ = tr.decode_code1(tr.encode_code1(pos, l_bad), 7)
    _expect_flag(lambda: tr.check_codes(p_k, l_k, vw, mw, rtol=tr.RTOL, where=where))


# ------------------------------------------------------------------------------------------ decoder round trips
@pytest.mark.parametrize("w1", [1, 4, 5, 7, 33, 65])
def test_code1_round_trip(w1):
    g = torch.Generator().manual_seed(w1)
    pos = torch.randint(0, 4, (3, 4, w1, 16), generator=g)
    live = torch.rand(3, 4, w1, 16, generator=g) < 0.5
    code = tr.encode_code1(pos, live)
    assert code.dtype == torch.int64 and code.shape == (3, 4, (w1 + 3) // 4 * 4)
    p, l, ok = tr.decode_code1(code, w1)
    assert ok and torch.equal(p, pos) and torch.equal(l, live)
    # a field written by hand from include/gdm.h: image 1, row 2, pixel w1-1, channel 4g+k at nibble k of field g
    f = code.view(torch.int16).view(3, 4, (w1 + 3) // 4, 4, 4).to(torch.int32) & 0xFFFF
    pw = w1 - 1
    for c in (0, 5, 15):
        nib = (int(f[1, 2, pw // 4, c // 4, pw % 4]) >> (4 * (c % 4))) & 0xF
        assert nib == int(pos[1, 2, pw, c]) | (4 * int(live[1, 2, pw, c]))
    # pixels >= W1 of the last quad decode as "not zero" -> flagged
    if w1 % 4:
        bad = f.clone()
        bad[0, 0, -1, 0, 3] = 1
        bad = torch.where(bad >= 0x8000, bad - 0x10000, bad).to(torch.int16).reshape(3, 4, -1).contiguous()
        assert not tr.decode_code1(bad.view(torch.int64), w1)[2]


def test_code2_round_trip():
    g = torch.Generator().manual_seed(2)
    pos = torch.randint(0, 4, (2, 3, 5, 32), generator=g)
    live = torch.rand(2, 3, 5, 32, generator=g) < 0.6
    code = tr.encode_code2(pos, live)
    assert code.dtype == torch.uint8 and code.shape == (2, 3, 5, 16) and int(code.max()) <= 8 * 24
    # byte j = 8 * (c_even + 5 * c_odd), 4 = dead (include/gdm.h)
    ce = 4 if not live[1, 2, 3, 6] else int(pos[1, 2, 3, 6])
    co = 4 if not live[1, 2, 3, 7] else int(pos[1, 2, 3, 7])
    assert int(code[1, 2, 3, 3]) == 8 * (ce + 5 * co)
    p, l, ok = tr.decode_code2(code)
    assert ok and torch.equal(l, live) and torch.equal(p[live], pos[live]) and not bool(p[~live].any())
    bad = code.clone()
    bad[0, 0, 0, 0] = 8 * 25
    assert not tr.decode_code2(bad)[2]
