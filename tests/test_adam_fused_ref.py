"""CPU: the host mirror and float64 references of tests/adam_fused_ref.py against torch.optim.Adam, an indexed loop and
planted faults -- every checker tests/test_simnn_adam_step_gpu.py relies on must flag the faulty reference and pass the
clean one on the same inputs -- and the regimes the case tables reach."""
import numpy as np
import pytest
import torch

import adam_fused_ref as A
import lowering_ref as R

D = torch.float64
HP = [A.hyper32(lr, betas, A.EPS, gs) for betas, lr, gs in A.HYPER_SETS]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _as_kernel(ref, dtype=torch.float32):
    """a reference result as an ideal kernel would store it"""
    return R.rnd(ref, dtype)


def _state(N, C, P, seed, step=3):
    n = N * C * P
    p = torch.randn(n, generator=_g(seed))
    m = torch.randn(n, generator=_g(seed + 1)) * 1e-3
    v = torch.rand(n, generator=_g(seed + 2)) * 1e-5 + 1e-12
    g_pc = torch.randn(N, P, C, generator=_g(seed + 3)) * 10.0 ** -step
    return p, g_pc, m, v


@pytest.mark.parametrize("hp", HP, ids=["b0.5", "b0.9"])
def test_pc_reference_is_torch_optim_adam_on_the_unpermuted_gradient(hp):
    N, C, P = 2, 5, 7
    lr, b1, b2, eps, gs = hp
    p0 = torch.randn(N, C, P, generator=_g(31), dtype=D)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 6):
        g = torch.randn(N, C, P, generator=_g(40 + step), dtype=D) * 10.0 ** -step
        par.grad = (g * gs).clone()
        opt.step()
        r = A.pc_step_ref(p, g.permute(0, 2, 1).contiguous(), m, v, N, C, P, step, hp, torch.float32)
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        torch.testing.assert_close(p, par.detach(), rtol=1e-12, atol=0)
        assert r["shadow"].shape == (N, P, C)
        assert torch.equal(r["shadow"], p.float().permute(0, 2, 1))


def test_group_sizes_count_every_workgroup_once():
    for grid in range(1, 5001):
        sizes = A.group_sizes(grid)
        assert sum(sizes) == grid and len(sizes) == min(grid, A.GROUPS), grid
        assert min(sizes) >= 1, grid
        # the members of group g are the workgroups with blk % 64 == g
        if grid in (1, 63, 64, 65, 130, 2080, 2113):
            assert sizes == [len(range(g, grid, A.GROUPS)) for g in range(len(sizes))], grid


def test_tile_plan():
    pl = A.tile_plan(3, 40, 300, True)
    assert (pl["tx"], pl["ty"], pl["grid"]) == (3, 2, 18)
    assert pl["vector"] == [[True, True, False], [False, False, False]] and pl["vector_tiles"] == 6
    assert A.tile_plan(3, 40, 300, False)["vector_tiles"] == 0 and A.tile_plan(2, 20, 130)["vector_tiles"] == 0
    assert A.tile_plan(128, 32, 80)["vector_tiles"] == 0                 # the trainer test's shape: never the vector path
    assert A.tile_plan(128, 32, 1728)["vector_tiles"] == 128 * 13 and A.tile_plan(128, 32, 1728)["scalar_tiles"] == 128
    assert (pl["groups"], pl["resident_slots"], A.REC_INTS) == (64, 2048, 1056)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=str)
def test_pack_model_against_an_indexed_loop(dtype):
    w = torch.randn(32, 16, 3, 3, generator=_g(5))
    kpf, kpb = A.KP[dtype]
    wf, wb = torch.zeros(32, kpf), torch.zeros(16, kpb)
    for o in range(32):
        for ci in range(16):
            for tap in range(9):
                wf[o, tap * 16 + ci] = w[o, ci, tap // 3, tap % 3]
                wb[ci, (8 - tap) * 32 + o] = w[o, ci, tap // 3, tap % 3]
    want = torch.cat([wf.reshape(-1), wb.reshape(-1)]).to(dtype)
    got = A.conv2_pack_ref(w, dtype)
    assert got.numel() == A.pack_elems(dtype) == 32 * kpf + 16 * kpb
    assert R.check_bits(got, want, what="pack") == []
    assert (kpf, kpb) == ((168, 296) if dtype == torch.bfloat16 else (146, 290))


def test_pack_checker_flags_images_of_the_weights_before_the_update():
    w0 = torch.randn(32, 16, 3, 3, generator=_g(6))
    w1 = w0 - 2e-5 * torch.sign(torch.randn(32, 16, 3, 3, generator=_g(7)))
    for dtype in (torch.float32, torch.bfloat16):
        w1r = w1 if dtype == torch.float32 else w1 + 0.05          # a change bf16 can see
        clean = A.conv2_pack_ref(w1r, dtype)
        assert R.check_bits(A.conv2_pack_ref(w1r, dtype, w_before=w0), clean) == []
        assert R.check_bits(A.conv2_pack_ref(w1r, dtype, w_before=w0, faults=("stale",)), clean)


PC_FAULT_SHAPE = (2, 40, 300)            # a partial c tile of 8 and a partial p tile of 44, like case C


@pytest.mark.parametrize("fault", ["c_tail", "p_tail", "no_transpose", "stale_shadow"])
@pytest.mark.parametrize("hp", HP, ids=["b0.5", "b0.9"])
def test_pc_checker_flags(fault, hp):
    N, C, P = PC_FAULT_SHAPE
    p, g_pc, m, v = _state(N, C, P, 50)
    ref = A.pc_step_ref(p, g_pc, m, v, N, C, P, 3, hp, torch.bfloat16)

    def as_kernel(r):
        return dict(p=_as_kernel(r["p"][0]), m=_as_kernel(r["m"][0]), v=_as_kernel(r["v"][0]), shadow=r["shadow"])

    assert A.check_pc(as_kernel(ref), ref)[0] == []
    bad = A.pc_step_ref(p, g_pc, m, v, N, C, P, 3, hp, torch.bfloat16, faults=(fault,))
    assert A.check_pc(as_kernel(bad), ref)[0], fault


@pytest.mark.parametrize("n", [4977, 4611])
def test_small_range_checker_flags_a_scalar_tail_left_alone(n):
    p, g = torch.randn(n, generator=_g(19)), torch.randn(n, generator=_g(20)) * 1e-2
    m, v = torch.randn(n, generator=_g(21)) * 1e-3, torch.rand(n, generator=_g(22)) * 1e-5
    for lr, b1, b2, eps, gs in HP:
        args = (p, g, m, v, 3, lr, b1, b2, eps, gs)
        ref = R.adam_ref(*args)
        assert R.check_adam({k: _as_kernel(ref[k][0]) for k in "pmv"}, ref)[0] == []
        bad = R.adam_ref(*args, faults=(("tail", n),))
        assert R.check_adam({k: _as_kernel(bad[k][0]) for k in "pmv"}, ref)[0]


@pytest.mark.parametrize("hp", HP, ids=["b0.5", "b0.9"])
@pytest.mark.parametrize("shape", [(1, 32, 128), (3, 40, 300)], ids=["A", "C"])
def test_float64_check_separates_a_stale_cached_step_size(hp, shape):
    """after the rewrite, step 4 with the step size cached under the OLD lr / beta1 must miss adam_ref's bound on p"""
    N, C, P = shape
    p, g_pc, m, v = _state(N, C, P, 60, step=4)
    new = A.rewritten(hp)
    ref = A.pc_step_ref(p, g_pc, m, v, N, C, P, 4, new, torch.float32)
    good = dict(p=_as_kernel(ref["p"][0]), m=_as_kernel(ref["m"][0]), v=_as_kernel(ref["v"][0]), shadow=ref["shadow"])
    assert A.check_pc(good, ref)[0] == []
    bad = A.pc_step_ref(p, g_pc, m, v, N, C, P, 4, new, torch.float32, faults=(("stale_slot", hp),))
    got = dict(p=_as_kernel(bad["p"][0]), m=_as_kernel(bad["m"][0]), v=_as_kernel(bad["v"][0]), shadow=bad["shadow"])
    fails = A.check_pc(got, ref)[0]
    assert fails and " p:" in fails[0], fails
    # the same on a small range
    n = 4977
    ps, gs_ = torch.randn(n, generator=_g(61)), torch.randn(n, generator=_g(62)) * 1e-4
    ms, vs = torch.randn(n, generator=_g(63)) * 1e-3, torch.rand(n, generator=_g(64)) * 1e-5 + 1e-12
    stale_lr = R.adam_corrections(4, hp[0], hp[1], hp[2])[0] * (1.0 - new[1] ** 4)
    r = R.adam_ref(ps, gs_, ms, vs, 4, new[0], new[1], new[2], new[3], new[4])
    b = R.adam_ref(ps, gs_, ms, vs, 4, stale_lr, new[1], new[2], new[3], new[4])
    assert R.check_adam({k: _as_kernel(b[k][0]) for k in "pmv"}, r)[0]


def test_record_reference_and_its_checker():
    hp = HP[0]
    for step in (1, 2, 8):
        rec, keep = A.record_ref(step, hp)
        assert int(rec[0]) == 0 and all(int(rec[A.REC_GROUP0 + 16 * g]) == 0 for g in range(A.GROUPS))
        nxt = A.REC_SLOT0 + 4 * ((step + 1) & 1)
        ss, bq = R.adam_corrections(step + 1, hp[0], hp[1], hp[2])
        assert int(rec[nxt]) == step + 1
        assert rec[nxt + 1:nxt + 3].view(torch.float32).tolist() == [float(np.float32(ss)), float(np.float32(bq))]
        other = set(range(A.REC_INTS)) - set(range(A.REC_SLOT0, A.REC_SLOT0 + 8))
        assert all(int(rec[i]) == 0 for i in other) and int(keep.sum()) == A.REC_INTS - 3
        assert A.check_record(rec, step, hp) == []
        # the slot the launch read may hold anything; one ulp of the cached floats is allowed, two are not
        ok = rec.clone()
        ok[A.REC_SLOT0 + 4 * (step & 1)] = step
        ok[nxt + 1] += 1
        assert A.check_record(ok, step, hp) == []
        for i, delta in ((0, 1), (A.REC_GROUP0 + 16 * 63, 1), (nxt, 1), (nxt + 1, 2), (nxt + 2, -2), (nxt + 3, 1), (5, 7),
                         (A.REC_GROUP0 + 17, 1)):
            bad = rec.clone()
            bad[i] += delta
            assert A.check_record(bad, step, hp), (step, i)
    assert A.check_record(A.record_ref(3, hp)[0], 4, hp)            # the record of another step


def test_case_tables_reach_every_regime():
    big = set().union(*(A.regimes(c) for c in A.BIG_CASES.values()))
    assert big == A.BIG_REGIMES, big ^ A.BIG_REGIMES
    small = set().union(*(A.regimes(c) for c in A.SMALL_CASES))
    assert small == A.SMALL_REGIMES, small ^ A.SMALL_REGIMES
    grids = {name: A.tile_plan(*c)["grid"] for name, c in A.BIG_CASES.items()}
    assert grids == dict(A=1, B63=63, B64=64, B65=65, C=18, D=4, E=10, F=2113, G=2080, H=18)
    # what the issue names per case
    assert "vector tiles" in A.regimes(A.BIG_CASES["A"]) and "scalar tiles" not in A.regimes(A.BIG_CASES["A"])
    assert {"vector and scalar tiles in one launch", "partial c tile", "partial p tile, P % 4 == 0", "C > 32"} <= \
        A.regimes(A.BIG_CASES["C"])
    assert "P % 4 != 0" in A.regimes(A.BIG_CASES["D"]) and "vector tiles" not in A.regimes(A.BIG_CASES["D"])
    assert "half p tile behind a full one" in A.regimes(A.BIG_CASES["E"])
    assert {"more workgroups than resident slots", "odd grid"} <= A.regimes(A.BIG_CASES["F"])
    assert "only vector tiles above the resident slots" in A.regimes(A.BIG_CASES["G"])
    assert "vector tiles" not in A.regimes(A.BIG_CASES["H"])
    # every small case rides on A and on C; every big case is run
    for b in ("A", "C"):
        assert {s for bb, s in A.STEP_PAIRS if bb == b} == set(A.SMALL_CASES)
    assert {b for b, _ in A.STEP_PAIRS} == set(A.BIG_CASES)
    # gdm_adam_step_dev_pc's own table: a partial channel tile above 32 channels, mixed tiles, two full channel tiles
    pc = set().union(*(A.regimes(c) for c in A.PC_CASES.values()))
    assert {"vector and scalar tiles in one launch", "partial c tile", "C > 32", "P % 4 != 0",
            "half p tile behind a full one", "misaligned p / m / v"} <= pc
    assert A.tile_plan(*A.PC_CASES["two-c-tiles"])["scalar_tiles"] == 0 and A.tile_plan(*A.PC_CASES["two-c-tiles"])["ty"] == 2
