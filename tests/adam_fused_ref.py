"""Host mirror and float64 references of model 1's one-launch optimizer step (csrc/simnn_adam.hip, gdm_simnn_adam_step)
and of the tile body it shares with gdm_adam_step_dev_pc (csrc/adam_pc.h).  A plain module next to lowering_ref.py,
whose Adam reference, checkers and rounding helper it reuses (R): tests/test_adam_fused_ref.py (CPU) checks it against
torch.optim.Adam, an indexed loop and planted faults; tests/test_simnn_adam_step_gpu.py (GPU) holds the kernels to it on
the case tables at the end of the file.

What is mirrored (from the kernel's comments, not from its output):
  tiles       a workgroup owns 128 p x 32 c of one row n of the (N, C, P) parameter; grid = ceil(P / 128) ceil(C / 32) N;
              a tile takes the 16-byte path when P % 4 == 0, p / m / v are 16-byte aligned and the tile is full both ways
  completion  group g = workgroup % 64 counts its (grid - g + 63) // 64 members, min(grid, 64) groups count themselves;
              the kernel's comments assume 8 x 256 = 2048 resident workgroup slots
  record      1056 ints: [0] finished groups, [32 + 16 g] finished members of group g, [16 + 4 s .. 16 + 4 s + 2] =
              {step, step_size, sqrt(bias_correction2)} of slot s = step & 1; a launch leaves every counter at zero
              and the NEXT step's terms in the slot it did not read
  small range Adam in rounds of 2 x 4 floats per thread (2048 elements a round) when the four arrays are 16-byte
              aligned, a scalar loop for the last n % 4 elements (for all of them when unaligned)
  pack        conv2's images (simnn_trunk.h): forward Wf[32][KPF] with k = tap * 16 + ci, backward Wb[16][KPB] with
              k = tap' * 32 + o and tap' = 8 - tap, each row zero padded behind 144 / 288
No tolerance is introduced here: p, m, v are held to lowering_ref.adam_ref's bounds, everything else to bit equality.
"""
import numpy as np
import torch

import lowering_ref as R

TILE_P, TILE_C = 128, 32
GROUPS = 64                                  # completion groups (REC_GROUPS)
RESIDENT_SLOTS = 2048                        # 256 CUs x 8 workgroups: the slots the kernel's comments count on
REC_SLOT0, REC_GROUP0 = 16, 32
REC_INTS = REC_GROUP0 + 16 * GROUPS          # GDM_SIMNN_ADAM_RECORD_INTS
SMALL_ROUND = 256 * 2 * 4                    # elements of the small range one round of the two-vector loop covers
W2_ELEMS = 32 * 16 * 9
KP = {torch.bfloat16: (168, 296), torch.float32: (146, 290)}        # (KPF, KPB)


def hyper32(lr, betas, eps, grad_scale):
    """(lr, beta1, beta2, eps, grad_scale) as the device record holds them: fp32 values, widened"""
    return tuple(float(np.float32(x)) for x in (lr, betas[0], betas[1], eps, grad_scale))


# ------------------------------------------------------------------------------------------------ plan mirrors
def tile_plan(N, C, P, aligned=True):
    tx, ty = (P + TILE_P - 1) // TILE_P, (C + TILE_C - 1) // TILE_C
    vec_ok = bool(aligned) and P % 4 == 0
    vector = [[vec_ok and (bx + 1) * TILE_P <= P and (by + 1) * TILE_C <= C for bx in range(tx)] for by in range(ty)]
    n_vec = N * sum(sum(row) for row in vector)
    grid = tx * ty * N
    return dict(tx=tx, ty=ty, grid=grid, vec_ok=vec_ok, vector=vector, vector_tiles=n_vec, scalar_tiles=grid - n_vec,
                groups=GROUPS, resident_slots=RESIDENT_SLOTS)


def group_sizes(grid):
    """members of every completion group: n_grp = min(grid, 64) groups, in_grp = (grid - g + 63) // 64"""
    return [(grid - g + GROUPS - 1) // GROUPS for g in range(min(grid, GROUPS))]


# -------------------------------------------------------------------------------------------------- references
def pc_step_ref(p, g_pc, m, v, N, C, P, step, hyper32, shadow_dtype, *, faults=()):
    """ONE float64 Adam step (R.adam_ref) of an (N, C, P) parameter whose gradient arrives as (N, P, C), from the given
    state.  hyper32 = (lr, beta1, beta2, eps, grad_scale).  Returns dict p, m, v -> (ref, bound), each (N, C, P), and
    shadow = rnd(p', shadow_dtype) permuted to (N, P, C).
    faults: "c_tail" / "p_tail" = the partial channel / pixel tile is left as it was; "no_transpose" = the gradient is
    read as if it were (N, C, P) already; "stale_shadow" = the operand copy is taken from the parameter before the
    update; ("stale_slot", old_hyper32) = step_size is the one cached for this step under the old lr / beta1."""
    lr, b1, b2, eps, gs = hyper32
    old = [t.detach().cpu().double().reshape(N, C, P) for t in (p, m, v)]
    g = g_pc.detach().cpu().double()
    g = g.reshape(N, C, P) if "no_transpose" in faults else g.reshape(N, P, C).permute(0, 2, 1)
    for f in faults:
        if isinstance(f, tuple) and f[0] == "stale_slot":
            lr = R.adam_corrections(step, f[1][0], f[1][1], b2)[0] * (1.0 - b1 ** step)
    res = R.adam_ref(old[0], g.contiguous(), old[1], old[2], step, lr, b1, b2, eps, gs)
    c_full, p_full = C // TILE_C * TILE_C, P // TILE_P * TILE_P
    for name, was in zip("pmv", old):
        if "c_tail" in faults:
            res[name][0][:, c_full:] = was[:, c_full:]
        if "p_tail" in faults:
            res[name][0][:, :, p_full:] = was[:, :, p_full:]
    src = old[0] if "stale_shadow" in faults else R.rnd(res["p"][0], torch.float32).double()
    res["shadow"] = R.rnd(src, shadow_dtype).permute(0, 2, 1).contiguous()
    return res


def check_pc(got, ref, *, what=""):
    """got: dict p, m, v (any shape, (N, C, P) order), shadow (N, P, C).  p, m, v within adam_ref's bounds; the operand
    copy bit-equal to the rounded parameter THE KERNEL wrote.  Returns (failures, worst ratios)."""
    fails, worst = R.check_adam(got, ref, what=what)
    N, C, P = ref["p"][0].shape
    want = R.rnd(got["p"].detach().cpu().reshape(N, C, P), got["shadow"].dtype).permute(0, 2, 1).contiguous()
    fails += R.check_bits(got["shadow"].detach().cpu().reshape(N, P, C), want, what=f"{what} operand copy")
    return fails, worst


def conv2_pack_ref(w, dtype, *, w_before=None, faults=()):
    """conv2's packed images from the (32, 16, 3, 3) weights: [Wf (32, KPF) | Wb (16, KPB)] flat, in dtype.
    fault "stale": built from w_before, the weights before the update."""
    if "stale" in faults:
        w = w_before
    w = w.detach().cpu().double().reshape(32, 16, 9)                    # (o, ci, tap)
    kpf, kpb = KP[dtype]
    wf = torch.zeros(32, kpf, dtype=torch.float64)
    wf[:, :144] = w.permute(0, 2, 1).reshape(32, 144)                   # k = tap * 16 + ci
    wb = torch.zeros(16, kpb, dtype=torch.float64)
    wb[:, :288] = w.flip(2).permute(1, 2, 0).reshape(16, 288)           # k = (8 - tap) * 32 + o
    return R.rnd(torch.cat([wf.reshape(-1), wb.reshape(-1)]), dtype)


def pack_elems(dtype):
    kpf, kpb = KP[dtype]
    return 32 * kpf + 16 * kpb


def _f32_bits(x):
    return int(np.float32(x).view(np.int32))


def record_ref(step, hyper32):
    """(record, compared) after a launch that performed `step`: all counters zero, slot (step + 1) & 1 = {step + 1,
    step_size, sqrt(bc2)} of step + 1 (the host's doubles rounded to fp32), zeros elsewhere.  `compared` leaves out the
    slot the launch read (it holds whatever the launch found: this step's terms, or zeros on a fresh record)."""
    rec = torch.zeros(REC_INTS, dtype=torch.int32)
    keep = torch.ones(REC_INTS, dtype=torch.bool)
    ss, bq = R.adam_corrections(step + 1, hyper32[0], hyper32[1], hyper32[2])
    nxt = REC_SLOT0 + 4 * ((step + 1) & 1)
    rec[nxt], rec[nxt + 1], rec[nxt + 2] = step + 1, _f32_bits(ss), _f32_bits(bq)
    cur = REC_SLOT0 + 4 * (step & 1)
    keep[cur:cur + 3] = False
    return rec, keep


def ulps_apart(a_bits, b_bits):
    """distance in fp32 ulps of two positive floats given as int32 bit patterns"""
    return abs(int(a_bits) - int(b_bits))


def check_record(rec, step, hyper32, *, what=""):
    """counters, tag and the zeros exactly; the two cached floats within one fp32 ulp of the host's (the device derives
    them in double too, so only the final rounding can differ)"""
    rec = rec.detach().cpu().to(torch.int32)
    want, keep = record_ref(step, hyper32)
    nxt = REC_SLOT0 + 4 * ((step + 1) & 1)
    exact = keep.clone()
    exact[nxt + 1:nxt + 3] = False
    fails = []
    if rec.numel() != REC_INTS:
        return [f"{what}: record of {rec.numel()} ints"]
    ne = (rec != want) & exact
    if bool(ne.any()):
        i = int(ne.nonzero()[0])
        fails.append(f"{what}: record[{i}] = {int(rec[i])}, want {int(want[i])} ({int(ne.sum())} ints differ)")
    for k, name in ((1, "step_size"), (2, "sqrt(bc2)")):
        if ulps_apart(rec[nxt + k], want[nxt + k]) > 1:
            fails.append(f"{what}: cached {name} of step {step + 1} is {ulps_apart(rec[nxt + k], want[nxt + k])} ulps "
                         "from the host's")
    return fails


# ------------------------------------------------------------------------------------------------- case tables
# big range: name -> (N, C, P, p / m / v aligned)
BIG_CASES = {
    "A": (1, 32, 128, True),
    "B63": (63, 32, 128, True), "B64": (64, 32, 128, True), "B65": (65, 32, 128, True),
    "C": (3, 40, 300, True),
    "D": (2, 20, 130, True),
    "E": (5, 32, 192, True),
    "F": (2113, 3, 5, True),
    "G": (130, 64, 1024, True),
    "H": (3, 40, 300, False),
}
BIG_STEPS = {name: 2 if name == "G" else 6 for name in BIG_CASES}
# small range: (n_small, offset of conv2.weight, the four arrays aligned)
SMALL_CASES = [(4608, 0, True), (4977, 80, True), (4980, 80, True), (4611, 3, True), (6660, 2049, True),
               (4977, 80, False)]
SMALL_DEFAULT = (4980, 80, True)
# (big case, small case) pairs of the one-launch step: every small case with A and C, the padded layout elsewhere
STEP_PAIRS = [(b, s) for b in ("A", "C") for s in SMALL_CASES] + \
             [(b, SMALL_DEFAULT) for b in ("B63", "B64", "B65", "D", "E", "F", "G", "H")]
# gdm_adam_step_dev_pc on its own
PC_CASES = {"C": BIG_CASES["C"], "D": BIG_CASES["D"], "E": BIG_CASES["E"], "H": BIG_CASES["H"],
            "two-c-tiles": (2, 64, 256, True)}
HYPER_SETS = [((0.5, 0.999), 2e-5, 0.125), ((0.9, 0.99), 1e-2, 1.0)]          # (betas, lr, grad_scale); eps = 1e-8
EPS = 1e-8
# the host rewrite of lr and beta1 the state-machine scenario performs after step 3: lr x 100, beta1 replaced -- large
# enough that adam_ref's bound on p rejects step 4 done with the step size cached under the old values
# (test_adam_fused_ref.py: test_float64_check_separates_a_stale_cached_step_size)
REWRITE = dict(lr=100.0, beta1=0.8)


def rewritten(hp):
    return hyper32(hp[0] * REWRITE["lr"], (REWRITE["beta1"], hp[2]), hp[3], hp[4])


BIG_REGIMES = {"grid of 1", "fewer groups than 64", "exactly 64 groups", "a group with two members",
               "groups of unequal size", "more workgroups than resident slots", "odd grid", "vector tiles",
               "scalar tiles", "vector and scalar tiles in one launch", "only vector tiles above the resident slots",
               "partial c tile", "partial p tile, P % 4 == 0", "P % 4 != 0", "half p tile behind a full one",
               "misaligned p / m / v", "C > 32"}
SMALL_REGIMES = {"no tail", "tail of 1", "tail of 3", "conv2.weight at 0", "conv2.weight offset % 4 != 0",
                 "conv2.weight behind the first round", "conv2.weight over three rounds", "model layout",
                 "padded layout", "scalar small range", "vector small range"}


def regimes(case):
    """what a case of BIG_CASES / PC_CASES ((N, C, P, aligned)) or of SMALL_CASES ((n, offset, aligned)) reaches"""
    out = set()
    if len(case) == 4:
        N, C, P, aligned = case
        pl = tile_plan(N, C, P, aligned)
        grid, sizes = pl["grid"], group_sizes(pl["grid"])
        out |= {"grid of 1"} if grid == 1 else set()
        out |= {"fewer groups than 64"} if len(sizes) < GROUPS else set()
        out |= {"exactly 64 groups"} if grid == GROUPS else set()
        out |= {"a group with two members"} if max(sizes) == 2 else set()
        out |= {"groups of unequal size"} if len(set(sizes)) > 1 else set()
        out |= {"more workgroups than resident slots"} if grid > RESIDENT_SLOTS else set()
        out |= {"odd grid"} if grid % 2 else set()
        out |= {"vector tiles"} if pl["vector_tiles"] else set()
        out |= {"scalar tiles"} if pl["scalar_tiles"] else set()
        out |= {"vector and scalar tiles in one launch"} if pl["vector_tiles"] and pl["scalar_tiles"] else set()
        out |= {"only vector tiles above the resident slots"} if grid > RESIDENT_SLOTS and not pl["scalar_tiles"] \
            else set()
        out |= {"partial c tile"} if C % TILE_C else set()
        out |= {"partial p tile, P % 4 == 0"} if P % TILE_P and P % 4 == 0 else set()
        out |= {"P % 4 != 0"} if P % 4 else set()
        out |= {"half p tile behind a full one"} if P > TILE_P and P % TILE_P == TILE_P // 2 else set()
        out |= {"misaligned p / m / v"} if not aligned else set()
        out |= {"C > 32"} if C > TILE_C else set()
        return out
    n, off, aligned = case
    assert 0 <= off and off + W2_ELEMS <= n
    out |= {"scalar small range"} if not aligned else {"vector small range"}
    out |= {{0: "no tail", 1: "tail of 1", 3: "tail of 3"}.get(n % 4, "tail of 2")}
    out |= {"conv2.weight at 0"} if off == 0 else set()
    out |= {"conv2.weight offset % 4 != 0"} if off % 4 else set()
    out |= {"conv2.weight behind the first round"} if off >= SMALL_ROUND else set()
    out |= {"conv2.weight over three rounds"} if (off + W2_ELEMS - 1) // SMALL_ROUND - off // SMALL_ROUND >= 2 else set()
    out |= {"model layout"} if (n, off) == (4977, 80) else set()
    out |= {"padded layout"} if (n, off) == (4980, 80) else set()
    return out
