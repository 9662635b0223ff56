"""CPU: the float64 references of tests/lowering_ref.py.  Each agrees with an independent torch float64 evaluation on
small shapes, each checker flags the fault planted for it at the bounds the GPU tests use, and the shape tables of lowering_ref.py reach every regime of the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lowering_ref as R

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nchw(x, g):
    return x.reshape(g["B"], g["C"], g["H"], g["W"]) if g["planar"] else \
        x.reshape(g["B"], g["H"], g["W"], g["C"]).permute(0, 3, 1, 2)


SMALL = [g for g in R.IM2COL_GEOMS + R.COL2IM_GEOMS if R.im2col_elements(g) < 400000]


# ------------------------------------------------------------------------------------------------- faithfulness
@pytest.mark.parametrize("g", SMALL, ids=lambda g: g["name"])
def test_im2col_and_col2im_references_are_unfold_and_fold(g):
    B, H, W, C, KH, KW, s, p, OH, OW = (g[k] for k in ("B", "H", "W", "C", "KH", "KW", "stride", "pad", "OH", "OW"))
    x = torch.randn(B * H * W * C, generator=_g(1), dtype=D)
    kw = dict(B=B, H=H, W=W, C=C, KH=KH, KW=KW, stride=s, pad=p, OH=OH, OW=OW)
    cols = R.im2col_ref(x, planar=g["planar"], **kw)
    want = F.unfold(_nchw(x, g), (KH, KW), padding=p, stride=s).permute(0, 2, 1).reshape(B * OH * OW, C * KH * KW)
    assert torch.equal(cols, want)
    c = torch.randn(B * OH * OW, C * KH * KW, generator=_g(2), dtype=D)
    for tap_major in (False, True):
        ct = c.reshape(-1, C, KH * KW).permute(0, 2, 1).reshape(c.shape).contiguous() if tap_major else c
        ref = R.col2im_ref(ct, planar=g["planar"], tap_major=tap_major, **kw)
        fold = lambda v: F.fold(v.reshape(B, OH * OW, -1).permute(0, 2, 1), (H, W), (KH, KW), padding=p, stride=s)
        for name, src in (("pre", c), ("mag", c.abs()), ("taps", torch.ones_like(c))):
            got = ref[name] if g["planar"] else ref[name].permute(0, 3, 1, 2)
            torch.testing.assert_close(got, fold(src), rtol=1e-13, atol=1e-13)
    if g["name"].startswith("edge uncovered"):
        assert float(ref["taps"][:, 9].max()) == 0 and float(ref["pre"][:, 9].abs().max()) == 0


@pytest.mark.parametrize("cin,cout,k,s,p,ih", [(100, 128, 4, 1, 0, 1), (128, 64, 4, 2, 1, 4), (64, 32, 4, 2, 1, 8),
                                               (32, 1, 5, 1, 0, 16)])
@pytest.mark.parametrize("tap_major", [False, True])
def test_conv_transpose_is_a_gemm_and_the_col2im_reference(cin, cout, k, s, p, ih, tap_major):
    """the four generator layers (GAN_DES/SIMNN.py:70-81): rows (B*IH*IW, Cin) @ W (Cin, Cout*k*k), then col2im"""
    B, oh = 2, (ih - 1) * s - 2 * p + k
    x = torch.randn(B, cin, ih, ih, generator=_g(3), dtype=D)
    w = torch.randn(cin, cout, k, k, generator=_g(4), dtype=D)
    wm = w.permute(0, 2, 3, 1).reshape(cin, -1) if tap_major else w.reshape(cin, -1)
    cols = x.permute(0, 2, 3, 1).reshape(B * ih * ih, cin) @ wm
    ref = R.col2im_ref(cols, B=B, H=oh, W=oh, C=cout, KH=k, KW=k, stride=s, pad=p, OH=ih, OW=ih, tap_major=tap_major,
                       act=R.ACT_SIGMOID)
    want = F.conv_transpose2d(x, w, stride=s, padding=p)
    torch.testing.assert_close(ref["pre"].permute(0, 3, 1, 2), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["out"].permute(0, 3, 1, 2), torch.sigmoid(want), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("B,H,W,C", R.POOL_SHAPES)
def test_maxpool_reference_is_torch_max_pool_and_its_autograd(B, H, W, C):
    x = R.pool_input(B, H, W, C, torch.float32).double()
    v, idx = R.maxpool2_ref(x, B, H, W, C)
    xn = x.reshape(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    want, flat = F.max_pool2d(xn, 2, 2, return_indices=True)
    assert not R.check_bits(v.permute(0, 3, 1, 2).contiguous(), want.detach().contiguous(), what="values")
    oh, ow = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    pos = (flat // W - 2 * oh) * 2 + (flat % W - 2 * ow)
    assert torch.equal(idx.permute(0, 3, 1, 2).long(), pos)
    d = torch.randn(B, H // 2, W // 2, C, generator=_g(5), dtype=D)
    (want * d.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(R.maxpool2_bwd_ref(d, idx, B, H, W, C), xn.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID])
def test_batchnorm_references_are_torch_batch_norm_in_double(act):
    rows, C = 37, 5
    y = (torch.randn(rows, C, generator=_g(6), dtype=D) * 2 + 3).requires_grad_(True)
    gamma, beta = (torch.randn(C, generator=_g(7), dtype=D).requires_grad_(True) for _ in range(2))
    rm, rv = torch.randn(C, generator=_g(8), dtype=D), torch.rand(C, generator=_g(9), dtype=D) + 0.5
    trm, trv = rm.clone(), rv.clone()
    for _ in range(2):
        pre = F.batch_norm(y, trm, trv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
    out = R.act_ref(pre, act)
    st = R.bn_stats_ref(y, rm, rv, 3, calls=2)
    torch.testing.assert_close(st["running_mean"], trm, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(st["running_var"], trv, rtol=1e-13, atol=1e-13)
    assert st["num_batches_tracked"] == 5
    ref, _ = R.bn_apply_ref(y, gamma, beta, st["mean"], st["invstd"], act, torch.float32)
    torch.testing.assert_close(ref, out.detach(), rtol=1e-12, atol=1e-13)
    d = torch.randn(rows, C, generator=_g(10), dtype=D)
    (out * d).sum().backward()
    bw = R.bn_bwd_ref(d, out, y, gamma, st["mean"], st["invstd"], act)
    for name, want in (("dy", y.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        torch.testing.assert_close(bw[name][0], want, rtol=1e-10, atol=1e-12)
    # eval mode is bn_apply_ref on the running statistics
    ev = F.batch_norm(y, rm, rv, gamma, beta, training=False, eps=1e-5)
    ref, _ = R.bn_apply_ref(y, gamma, beta, rm, 1 / torch.sqrt(rv + 1e-5), R.ACT_NONE, torch.float32)
    torch.testing.assert_close(ref, ev.detach(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("rows", [2, 255, 257, 513, 16385])
def test_partials_follow_the_chunk_map_and_merge_to_the_batch_statistics(rows):
    y = torch.randn(rows, 3, generator=_g(rows), dtype=D) + 5
    pr = R.partials_ref(y)
    assert torch.equal(torch.bincount(R.chunk_of_rows(rows), minlength=R.row_chunks(rows)).double(), pr["n"][:, 0])
    part = torch.stack([pr["n"], pr["mean"], pr["m2"]], -1)
    rm, rv = torch.zeros(3, dtype=D), torch.ones(3, dtype=D)
    got, ref = R.merge_partials_ref(part, rows, rm, rv, 0), R.bn_stats_ref(y, rm, rv, 0)
    for k in ("mean", "invstd", "running_mean", "running_var"):
        torch.testing.assert_close(got[k], ref[k], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.99)])
@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_adam_reference_is_torch_optim_adam_on_double_parameters(betas, gs):
    b1, b2 = (float(np.float32(b)) for b in betas)                  # what the C ABI receives
    lr, eps, n = float(np.float32(2e-3)), float(np.float32(1e-8)), 50
    p0 = torch.randn(n, generator=_g(11), dtype=D)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    for step in range(1, 6):
        g = torch.randn(n, generator=_g(step), dtype=D) * 10.0 ** -step
        par.grad = g * gs
        opt.step()
        r = R.adam_ref(p, g, m, v, step, lr, b1, b2, eps, gs)
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        torch.testing.assert_close(p, par.detach(), rtol=1e-13, atol=1e-15)
        assert bool((r["p"][1] > 0).all()) and bool((r["p"][1] < 4e-7).all())


def test_loss_terms_are_the_oracle():
    from oracle import steps
    x = torch.tensor([-100.0, -30.0, -1.5, 0.0, 0.3, 30.0, 100.0], dtype=D)
    for y in (0.0, 0.1, 0.9, 1.0):
        assert float(R.bce_terms(x, y).mean()) == pytest.approx(float(steps.bce_with_logits(x, y)), rel=1e-14)


# --------------------------------------------------------------------------------------------- planted faults
def _as_kernel(ref, dtype=torch.float32):
    """a reference result as an ideal kernel would store it"""
    return R.rnd(ref, dtype)


def _col2im_case(**over):
    g = dict(R.geom("t", False, 2, 8, 8, 6, 4, 4, 2, 1), **over)
    cols = torch.randn(g["B"] * g["OH"] * g["OW"], g["C"] * 16, generator=_g(12))
    kw = {k: g[k] for k in ("B", "H", "W", "C", "KH", "KW", "stride", "pad", "OH", "OW")}
    return cols, kw


def test_col2im_checker_flags_a_tap_range_short_by_one_at_the_high_edge():
    cols, kw = _col2im_case()
    ref = R.col2im_ref(cols, **kw)
    assert R.check_col2im(_as_kernel(ref["out"]), ref, torch.float32)[0] == []
    bad = R.col2im_ref(cols, faults=("short_tap",), **kw)
    assert R.check_col2im(_as_kernel(bad["out"]), ref, torch.float32)[0]
    assert R.check_col2im(_as_kernel(bad["out"], torch.bfloat16), ref, torch.bfloat16)[0]


def test_col2im_checker_flags_tap_major_columns_read_in_torch_order():
    cols, kw = _col2im_case()
    ref = R.col2im_ref(cols, tap_major=True, **kw)
    assert R.check_col2im(_as_kernel(ref["out"]), ref, torch.float32)[0] == []
    bad = R.col2im_ref(cols, tap_major=True, faults=("torch_order",), **kw)
    assert R.check_col2im(_as_kernel(bad["out"]), ref, torch.float32)[0]


def test_col2im_checker_demands_exact_zeros_where_no_window_reaches():
    g = R.geom("t", False, 2, 10, 10, 4, 3, 3, 2, 0)
    cols = torch.randn(2 * 16, 36, generator=_g(13))
    kw = {k: g[k] for k in ("B", "H", "W", "C", "KH", "KW", "stride", "pad", "OH", "OW")}
    ref = R.col2im_ref(cols, **kw)
    got = _as_kernel(ref["out"])
    assert R.check_col2im(got, ref, torch.float32)[0] == []
    got[0, 9, 3, 1] = 1e-30
    assert R.check_col2im(got, ref, torch.float32)[0]


@pytest.mark.parametrize("what", ["stats", "colsum", "im2col"])
def test_checkers_flag_a_dropped_tail_row(what):
    rows, C = 257, 5
    y = torch.randn(rows, C, generator=_g(14)) + 1
    if what == "stats":
        rm, rv = torch.zeros(C), torch.ones(C)
        ref, short = R.bn_stats_ref(y, rm, rv, 0), R.bn_stats_ref(y[:-1], rm, rv, 0)
        bounds = R.stats_bounds("standard")[0]
        ok = {k: _as_kernel(ref[k]) for k in bounds}
        assert R.check_stats(ok, ref, bounds)[0] == []
        assert R.check_stats({k: _as_kernel(short[k]) for k in bounds}, ref, bounds)[0]
    elif what == "colsum":
        ref, E = R.colsum_ref(y)
        assert R.check_bound(_as_kernel(ref), ref, E)[0] == []
        assert R.check_bound(_as_kernel(R.colsum_ref(y[:-1])[0]), ref, E)[0]
    else:
        kw = dict(B=1, H=9, W=7, C=2, KH=3, KW=3, stride=2, pad=1, OH=5, OW=4)
        x = torch.randn(9 * 7 * 2, generator=_g(15))
        want = _as_kernel(R.im2col_ref(x, planar=False, **kw))
        got = want.clone()
        got[-4:] = 0                                                # the last output row's windows never written
        assert R.check_bits(want, want.clone()) == [] and R.check_bits(got, want)


@pytest.mark.parametrize("k", [127, 128])
def test_stats_checker_flags_a_chunk_counted_twice_around_the_128_chunk_round(k):
    """check_stats notices one of 192 chunks counted twice, whichever side of chunk 128 it sits on.  The float64 merge
    here has no rounds of its own: bn_finalize's second round itself is run by the GPU merge case of 3 x 16384 rows."""
    rows, C = 3 * 16384, 4
    y = torch.randn(rows, C, generator=_g(16)) * 0.5 + 2
    parts = [R.partials_ref(y[i * 16384:(i + 1) * 16384]) for i in range(3)]
    part = torch.cat([torch.stack([p["n"], p["mean"], p["m2"]], -1) for p in parts])
    assert part.shape[0] == 192 > R.FINALIZE_ROUND
    rm, rv = torch.zeros(C), torch.ones(C)
    ref = R.bn_stats_ref(y, rm, rv, 0)
    bounds = R.stats_bounds("standard")[0]
    ok = R.merge_partials_ref(part, rows, rm, rv, 0)
    assert R.check_stats({n: _as_kernel(ok[n]) for n in bounds}, ref, bounds)[0] == []
    bad = R.merge_partials_ref(part, rows, rm, rv, 0, faults=(("twice", k),))
    assert R.check_stats({n: _as_kernel(bad[n]) for n in bounds}, ref, bounds)[0]


def test_pool_checks_flag_the_last_maximum_and_a_gradient_in_the_dropped_row():
    B, H, W, C = 2, 11, 15, 5
    x = R.pool_input(B, H, W, C, torch.float32)
    v, idx = R.maxpool2_ref(x, B, H, W, C)
    vb, idxb = R.maxpool2_ref(x, B, H, W, C, faults=("last_max",))
    assert torch.equal(v, vb) and not torch.equal(idx, idxb)          # only the index tells
    d = torch.randn(B, H // 2, W // 2, C, generator=_g(17))
    want = _as_kernel(R.maxpool2_bwd_ref(d, idx, B, H, W, C))
    assert float(want[:, H - 1].abs().max()) == 0 and float(want[:, :, W - 1].abs().max()) == 0
    assert R.check_bits(_as_kernel(R.maxpool2_bwd_ref(d, idxb, B, H, W, C)), want)
    assert R.check_bits(_as_kernel(R.maxpool2_bwd_ref(d, idx, B, H, W, C, faults=("odd_row",))), want)


def test_stats_checker_flags_a_biased_running_variance():
    rows, C = 513, 4
    y = torch.randn(rows, C, generator=_g(18))
    rm, rv = torch.zeros(C), torch.ones(C)
    ref = R.bn_stats_ref(y, rm, rv, 0, calls=2)
    bad = R.bn_stats_ref(y, rm, rv, 0, calls=2, faults=("biased_running",))
    bounds = R.stats_bounds("standard")[0]
    assert R.check_stats({n: _as_kernel(bad[n]) for n in bounds}, ref, bounds)[0]


@pytest.mark.parametrize("n", [5, 1027])
def test_adam_checker_flags_a_tail_left_alone(n):
    p, g = torch.randn(n, generator=_g(19)), torch.randn(n, generator=_g(20)) * 1e-2
    m, v = torch.randn(n, generator=_g(21)) * 1e-3, torch.rand(n, generator=_g(22)) * 1e-5
    args = (p, g, m, v, 3, float(np.float32(2e-5)), 0.5, float(np.float32(0.999)), float(np.float32(1e-8)), 0.125)
    ref = R.adam_ref(*args)
    assert R.check_adam({k: _as_kernel(ref[k][0]) for k in "pmv"}, ref)[0] == []
    bad = R.adam_ref(*args, faults=(("tail", n),))
    assert R.check_adam({k: _as_kernel(bad[k][0]) for k in "pmv"}, ref)[0]


@pytest.mark.parametrize("P,C", [(45, 70), (641, 70), (511, 33)])
def test_permute_check_flags_a_transposed_tile_edge(P, C):
    x = torch.randn(2, P, C, generator=_g(23))
    want = R.permute_ref(x, 2, P, C, torch.bfloat16)
    assert torch.equal(want.float(), x.permute(0, 2, 1).bfloat16().float())
    assert R.check_bits(R.permute_ref(x, 2, P, C, torch.bfloat16, faults=("tile_edge",)), want)


# ----------------------------------------------------------------------------------------------- regime table
def test_shape_tables_reach_every_regime():
    bn = {pair: R.bn_regimes(*pair) for pair in R.BN_PAIRS}
    assert {r for r, _ in R.BN_PAIRS} == set(R.BN_ROWS) and {c for _, c in R.BN_PAIRS} == set(R.BN_CHANNELS) | {9}
    assert (65536, 32) in bn and (16385, 3) in bn
    assert {b["cw"] for b in bn.values()} == {1, 2, 4, 8, 16, 32, 64}
    assert any(b["idle_lanes"] for b in bn.values()) and {b["column_blocks"] for b in bn.values()} == {1, 2}
    assert {b["capped"] for b in bn.values()} == {False, True}, "both sides of the 64-chunk cap"
    assert R.row_chunks(256) == 1 and R.row_chunks(257) == 2 and R.chunk_rows(257) == 129
    assert R.row_chunks(16384) == 64 and R.chunk_rows(16384) == 256 and R.chunk_rows(16385) == 257
    assert R.row_chunks(16385) == 64 and R.chunk_rows(65536) == 1024
    assert {R.permute_kernel(p) for _, p, _ in R.PERMUTE_SHAPES} == {"narrow", "wide"}
    assert R.permute_kernel(511) == "narrow" and R.permute_kernel(512) == "wide"
    wide = [(p, c) for _, p, c in R.PERMUTE_SHAPES if R.permute_kernel(p) == "wide"]
    assert any(p % 128 and c % 32 for p, c in wide) and any(p % 128 == 0 and c % 32 == 0 for p, c in wide)
    assert {R.grid_trips(R.im2col_elements(g)) for g in R.IM2COL_GEOMS} == {1, 2}
    assert {R.grid_trips(R.col2im_elements(g)) for g in R.COL2IM_GEOMS} == {1, 2}
    for table in (R.IM2COL_GEOMS, R.COL2IM_GEOMS):
        assert any(g["KH"] != g["KW"] for g in table) and any(g["stride"] == 3 for g in table)
        assert any(g["pad"] == 0 for g in table) and any(g["pad"] > g["stride"] for g in table)
        assert any(g["OH"] == 1 and g["OW"] == 1 for g in table) and {1, 33} <= {g["C"] for g in table}
        assert any((g["OH"] - 1) * g["stride"] + g["KH"] - g["pad"] < g["H"] for g in table), "uncovered last rows"
        assert {g["planar"] for g in table} == {False, True} and {g["B"] for g in table} == {1, 3}
    assert {g.get("act", 0) for g in R.COL2IM_GEOMS} == {R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID}
    assert any(g.get("tap_major") for g in R.COL2IM_GEOMS)
    assert [R.grid_trips(r * c, R.POINTWISE_GRID_CAP) for r, c in R.BIAS_ACT_SHAPES] == [1, 1, 2]
    assert R.BIAS_ACT_SHAPES[0] == (1, 1)
    assert {R.adam_trips(n) for n in R.ADAM_N} == {1, 2} and R.adam_trips(8388608) == 1
    assert {n % 4 for n in R.ADAM_N} == {0, 1, 3} and any(n < 4 for n in R.ADAM_N)
    assert {(n + 1023) // 1024 > 1 for n in R.LOSS_N} == {False, True} and max(R.LOSS_N) == 65536
    assert any(n > 1024 and n % 1024 for n in R.LOSS_N)
    chunks = [sum(R.row_chunks(r) for r in shards) for shards, _ in R.MERGE_CASES]
    assert max(chunks) == 192 > R.FINALIZE_ROUND and {len(s) for s, _ in R.MERGE_CASES} == {1, 2, 3, 8}
    assert ((5, 300), 8) in R.MERGE_CASES
    assert {R.row_chunks(r) for r in R.COLSUM_ROWS} == {1, 2, 64}


def test_chunk_entry_point_matches_the_mirror():
    from gan_des_midi_music_gen_amd import _lib
    lib = _lib.load()
    for rows in R.BN_ROWS + [1, 511, 512, 16383, 100000]:
        assert lib.gdm_bn_partial_chunks(rows) == R.row_chunks(rows)
        assert lib.gdm_bn_workspace_bytes(rows, 7) == R.row_chunks(rows) * 7 * 12
