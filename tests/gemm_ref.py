"""float64 reference, input families, checker and case tables for gdm_gemm (csrc/gemm.hip, csrc/gemm_bf16*.hip).
A plain module next to lowering_ref.py: tests/test_gemm_ref.py (CPU) proves that the checker rejects every planted
fault and -- through gdm_gemm_plan, the library's own dispatch -- that the tables reach the kernels they name;
tests/test_gemm_edges_gpu.py (GPU) holds the kernels to the reference.

Two input families.

  exact: integer-valued operands and biases, |v| <= 8, with K max|a| max|b| + max|bias_n| + max|bias_m| < 2^24
    (asserted for every case).  Every product and every partial sum is then an integer below 2^24: exact in fp32 in any
    summation order, inside the MFMA included, and the operands are exact in bf16.  The float64 result rounded once to
    the output type is the only correct answer for no activation, ReLU and leaky ReLU (slope 0.25, a power of two),
    with any bias, for both compute types, every kernel and every split-K order: the criterion is bit equality of
    every element, no tolerance.  With the sigmoid epilogue B and the biases are scaled by powers of two so that the
    pre-activations span about +-8 (still exact); what remains is the sigmoid's own error, lowering_ref.act_bound with
    an exact pre-activation.

  continuous: seeded normals handed to the library unrounded in fp32 (bf16 operands are rounded on the host, they
    cannot be otherwise); an eighth of the entries sit exactly on bf16 ties ((1 + 2^-8) 2^e rounds down to even,
    (1 + 3 2^-8) 2^e rounds up to even).  The reference is float64 on the operands rounded to bf16 to nearest even for
    bf16 compute, unrounded for fp32 compute.  Element bound: (K + split_k + 2) 2^-23 Mag with Mag = sum|a||b| + |bias|
    -- K products accumulated, split_k slab sums and two bias adds, each a faithful (not necessarily nearest) fp32
    operation, in the worst case of any order; derived, not measured -- then the activation (act_bound) and half an
    ulp of a bf16 output (store_bound).  Decisive at small K: at K = 8 an operand truncated instead of rounded moves an
    output by about 2^-9 of itself, over a thousand times the bound.

A Case describes one call completely: shape, operand types and layouts (la / lb: "k" = K-major, k stride 1; "r" =
row-major, m / n stride 1), leading dimensions, element offsets of the pointers, the view C is, the epilogue.
layout() turns it into strides and offsets; plan_of() asks the library with fake pointers of that alignment (no GPU);
materialize() builds the tensors with exactly those strides, C inside a sentinel-filled buffer.
"""
import dataclasses
import functools
import math

import torch

from lowering_ref import (ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, act_bound, act_ref, check_bits, check_bound, rnd,
                          store_bound)

F32, BF16 = 0, 1
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
GDT = {"f32": F32, "bf16": BF16}
ESZ = {"f32": 4, "bf16": 2}
KTILE = {"generic_f32": 32, "generic_bf16": 64, "fast_k32": 32, "fast_k64": 64}
GUARD = 8                    # sentinel rows above and below C (8 rows of any width keep C's 16-byte alignment)
SENTINEL = -12352.0          # exact in bf16; no case of the tables produces it
VMAX = 8                     # exact family: |a|, |b|, |bias| <= VMAX
LEAKY_SLOPE = 0.25
FAULTS = ("drop_product", "drop_chunk", "drop_last_tile", "slab_twice", "slab_missing", "swap_rows_16",
          "swap_cols_in_group", "transpose_block", "bias_last_col", "bias_shift_4", "truncate_operand",
          "leaky_on_positive")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    m: int
    n: int
    k: int
    ta: str = "f32"
    la: str = "k"
    tb: str = "f32"
    lb: str = "r"
    comp: int = BF16
    split: int = 1               # requested split_k
    act: int = ACT_NONE
    bias_n: bool = False
    bias_m: bool = False
    tc: str = "f32"
    a_ld: int = 0                # leading dimensions in elements (0: the natural one)
    b_ld: int = 0
    c_ld: int = 0
    a_off: int = 0               # element offsets of the pointers from a 16-byte aligned address
    b_off: int = 0
    c_off: int = 0
    bias_off: int = 0
    c_t: bool = False            # C is the transpose of an (N, c_ld) array: scn != 1
    expect: str = ""             # kernel the case is meant to run
    continuous: bool = False     # also run in the continuous family

    @property
    def slope(self):
        return LEAKY_SLOPE if self.act == ACT_LEAKY else 0.0

    def plain(self):
        """the same call with fp32 output and no epilogue"""
        return dataclasses.replace(self, act=ACT_NONE, bias_n=False, bias_m=False, tc="f32", bias_off=0)

    def setting(self):
        return (self.act, self.bias_n, self.bias_m, self.tc)


# (activation, bias_n, bias_m, C type): the further setting of a case, rotated over the tables
ROTATION = [(ACT_RELU, True, False, "f32"), (ACT_LEAKY, False, True, "bf16"), (ACT_SIGMOID, True, True, "f32"),
            (ACT_NONE, False, False, "bf16"), (ACT_RELU, True, True, "bf16"), (ACT_LEAKY, True, False, "f32"),
            (ACT_SIGMOID, False, True, "bf16"), (ACT_NONE, True, True, "bf16")]


def with_setting(c, i):
    act, bn, bm, tc = ROTATION[i % len(ROTATION)]
    return dataclasses.replace(c, act=act, bias_n=bn, bias_m=bm, tc=tc)


# ---------------------------------------------------------------------------------------------------- layout
def layout(c):
    """element strides, element offsets and buffer lengths of the call"""
    a_ld = c.a_ld or (c.k if c.la == "k" else c.m)
    b_ld = c.b_ld or (c.k if c.lb == "k" else c.n)
    c_rows, c_cols = (c.n, c.m) if c.c_t else (c.m, c.n)
    c_ld = c.c_ld or c_cols
    assert a_ld >= (c.k if c.la == "k" else c.m) and b_ld >= (c.k if c.lb == "k" else c.n) and c_ld >= c_cols
    sam, sak = (a_ld, 1) if c.la == "k" else (1, a_ld)
    sbk, sbn = (1, b_ld) if c.lb == "k" else (b_ld, 1)
    scm, scn = (1, c_ld) if c.c_t else (c_ld, 1)
    return dict(sam=sam, sak=sak, sbk=sbk, sbn=sbn, scm=scm, scn=scn, c_ld=c_ld, c_rows=c_rows, c_cols=c_cols,
                a_len=c.a_off + (c.m - 1) * sam + (c.k - 1) * sak + 1,
                b_len=c.b_off + (c.k - 1) * sbk + (c.n - 1) * sbn + 1,
                c_at=c.c_off + GUARD * c_ld, c_len=c.c_off + (c_rows + 2 * GUARD) * c_ld)


def plan_of(c):
    """the library's plan for the case (gdm_gemm_plan on fake pointers with the case's alignment: no GPU)"""
    from gan_des_midi_music_gen_amd import ops
    L = layout(c)
    base = 1 << 20
    return ops.gemm_plan_raw(base + c.a_off * ESZ[c.ta], GDT[c.ta], L["sam"], L["sak"],
                             2 * base + c.b_off * ESZ[c.tb], GDT[c.tb], L["sbk"], L["sbn"],
                             3 * base + L["c_at"] * ESZ[c.tc], GDT[c.tc], L["scm"], L["scn"], c.m, c.n, c.k,
                             4 * base + c.bias_off * 4 if c.bias_n else None, c.comp, c.split)


def materialize(c, inp, device):
    """the call's tensors with layout()'s strides: a, b, out (a view into the sentinel-filled cbuf), bias_n, bias_m,
    and outside (True where cbuf is not part of out)"""
    L = layout(c)

    def operand(vals, t, shape, strides, off, length):
        buf = torch.zeros(length, dtype=TDT[t], device=device)
        v = buf.as_strided(shape, strides, off)
        v.copy_(vals.to(TDT[t]))
        return v

    a = operand(inp["a"], c.ta, (c.m, c.k), (L["sam"], L["sak"]), c.a_off, L["a_len"])
    b = operand(inp["b"], c.tb, (c.k, c.n), (L["sbk"], L["sbn"]), c.b_off, L["b_len"])
    cbuf = torch.full((L["c_len"],), SENTINEL, dtype=TDT[c.tc], device=device)
    outside = torch.ones(L["c_len"], dtype=torch.bool, device=device)
    shape, strides = (L["c_rows"], L["c_cols"]), (L["c_ld"], 1)
    outside.as_strided(shape, strides, L["c_at"]).fill_(False)
    out = cbuf.as_strided(shape, strides, L["c_at"])
    bias_n = bias_m = None
    if c.bias_n:
        bias_n = torch.zeros(c.bias_off + c.n, device=device)[c.bias_off:]
        bias_n.copy_(inp["bias_n"])
    if c.bias_m:
        bias_m = inp["bias_m"].to(device)
    return dict(a=a, b=b, out=out.t() if c.c_t else out, cbuf=cbuf, outside=outside, bias_n=bias_n, bias_m=bias_m)


def untouched(t):
    """every sentinel of the buffer around C is still there"""
    return bool((t["cbuf"][t["outside"]] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- inputs
def _seed(c):
    return (c.m * 1000003 + c.n * 10007 + c.k * 101 + (7 if c.act == ACT_SIGMOID else 0)) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=8)
def _inputs(family, m, n, k, sigmoid, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "exact":
        a = torch.randint(-VMAX, VMAX + 1, (m, k), generator=g).float()
        b = torch.randint(-VMAX, VMAX + 1, (k, n), generator=g).float()
        bn = torch.randint(-VMAX, VMAX + 1, (n,), generator=g).float()
        bm = torch.randint(-VMAX, VMAX + 1, (m,), generator=g).float()
        if bn[-1] == 0:
            bn[-1] = VMAX       # a bias missing on the last column must show
        s = 0
        if sigmoid:       # the sum of K products of uniform integers in +-8 has deviation 24 sqrt(K): bring it to ~4
            s = max(2, round(math.log2(6.0 * math.sqrt(k))))
            b, bn, bm = b * 2.0 ** -s, bn * 0.25, bm * 0.25
        # exactness: every partial sum and the biased result are multiples of 2^-s below 2^24 2^-s
        assert k * VMAX * VMAX + 2 * VMAX * 2 ** s < 2 ** 24, (k, s)
        assert float(a.abs().max()) <= VMAX and float(b.abs().max()) * 2 ** s <= VMAX
    else:
        a = torch.randn(m, k, generator=g)
        b = torch.randn(k, n, generator=g)
        for t in (a, b):          # an eighth of the entries exactly on bf16 ties, both rounding directions
            tie = torch.rand(t.shape, generator=g) < 0.125
            frac = torch.where(torch.rand(t.shape, generator=g) < 0.5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8)
            e = torch.randint(-3, 3, t.shape, generator=g).float()
            sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
            t[tie] = (sign * frac * 2.0 ** e)[tie]
        bn, bm = torch.randn(n, generator=g), torch.randn(m, generator=g)
        if sigmoid:
            b = b * 2.0 ** round(math.log2(4.0 / math.sqrt(k)))       # a power of two: the ties stay ties
    return dict(family=family, a=a, b=b, bias_n=bn, bias_m=bm)


def inputs(c, family):
    """fp32 a (M,K), b (K,N), bias_n, bias_m of the case (shared between the settings of one shape; never modified)"""
    return _inputs(family, c.m, c.n, c.k, c.act == ACT_SIGMOID, _seed(c))


def crop(inp, c):
    """the corner of larger inputs that case c uses (two cases of different shapes on the same values)"""
    return dict(family=inp["family"], a=inp["a"][:c.m, :c.k], b=inp["b"][:c.k, :c.n], bias_n=inp["bias_n"][:c.n],
                bias_m=inp["bias_m"][:c.m])


# ------------------------------------------------------------------------------------------------- reference
def _truncate_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _seen(x, t, comp, truncate=False):
    """the value the MFMA sees: the operand as handed over (t), then rounded to bf16 for bf16 compute"""
    x = x.to(TDT[t]).float()
    if comp == BF16:
        x = _truncate_bf16(x) if truncate else x.bfloat16().float()
    return x.double()


def slab_ks(plan, K, z):
    """the k indices of split-K slab z: interleaved K tiles on the fast kernels, a contiguous range on the generic"""
    ks = torch.arange(K)
    if plan["kernel"].startswith("fast"):
        return ks[(ks // KTILE[plan["kernel"]]) % plan["split_k"] == z]
    return ks[ks // plan["k_per_split"] == z]


def fault_applies(fault, c, plan, family):
    return {"slab_twice": plan["split_k"] > 1, "slab_missing": plan["split_k"] > 1, "swap_rows_16": c.m > 16,
            "swap_cols_in_group": c.n >= 4, "transpose_block": c.m >= 16 and c.n >= 16,
            "drop_chunk": c.k >= 8, "drop_last_tile": True, "drop_product": True,
            "bias_last_col": c.bias_n, "bias_shift_4": c.bias_n and c.n > 4,
            "truncate_operand": family == "continuous" and c.comp == BF16 and c.ta == "f32",
            "leaky_on_positive": c.act == ACT_LEAKY}[fault]


def expected(c, inp, plan, *, faults=()):
    """-> dict(out = float64 result, and either want (exact family: the one correct answer in C's type, kind "bits") or
    E (the element bound, kind "bound")).  `faults` plants the named mistakes of a wrong kernel."""
    a = _seen(inp["a"], c.ta, c.comp, truncate="truncate_operand" in faults)
    b = _seen(inp["b"], c.tb, c.comp)
    pre, mag = a @ b, a.abs() @ b.abs()
    m0, n0 = divmod(int(pre.argmax()), c.n)          # the largest output: no ReLU hides what is taken from it
    if "drop_product" in faults:
        k0 = int((a[m0] * b[:, n0]).abs().argmax())
        pre[m0, n0] -= a[m0, k0] * b[k0, n0]
    if "drop_chunk" in faults:
        k8 = 8 * ((c.k // 8) // 2)
        pre[m0] -= a[m0, k8:k8 + 8] @ b[k8:k8 + 8]
    if "drop_last_tile" in faults:
        kl = ((c.k - 1) // KTILE[plan["kernel"]]) * KTILE[plan["kernel"]]
        pre -= a[:, kl:] @ b[kl:]
    for f, sgn in (("slab_twice", 1.0), ("slab_missing", -1.0)):
        if f in faults:
            ks = slab_ks(plan, c.k, plan["split_k"] - 1)
            pre += sgn * (a[:, ks] @ b[ks])
    if c.bias_n:
        bn = inp["bias_n"].double()
        mag = mag + bn.abs()
        if "bias_last_col" in faults:
            bn = bn.clone()
            bn[-1] = 0
        if "bias_shift_4" in faults:
            bn = torch.cat([bn[:4], bn[:-4]])
        pre = pre + bn
    if c.bias_m:
        pre = pre + inp["bias_m"].double()[:, None]
        mag = mag + inp["bias_m"].double().abs()[:, None]
    out = (pre * c.slope if "leaky_on_positive" in faults else act_ref(pre, c.act, c.slope)).clone()
    if "swap_rows_16" in faults:
        r = (c.m - 17) // 2
        out[[r, r + 16]] = out[[r + 16, r]]
    if "swap_cols_in_group" in faults:
        q = 4 * ((c.n // 4) // 2)
        out[:, [q + 1, q + 2]] = out[:, [q + 2, q + 1]]
    if "transpose_block" in faults:
        r0, q0 = 16 * ((c.m // 16) // 2), 16 * ((c.n // 16) // 2)
        out[r0:r0 + 16, q0:q0 + 16] = out[r0:r0 + 16, q0:q0 + 16].t().clone()
    dt = TDT[c.tc]
    if inp["family"] == "exact" and c.act != ACT_SIGMOID:
        return dict(kind="bits", out=out, want=rnd(out, dt))
    e_pre = torch.zeros_like(mag) if inp["family"] == "exact" else (c.k + plan["split_k"] + 2) * 2.0 ** -23 * mag
    return dict(kind="bound", out=out, E=store_bound(out, act_bound(pre, e_pre, c.act, c.slope), dt))


def check(got, exp, *, what=""):
    """-> (failures, worst err / bound or None): bit equality of every element for the exact family, the element bound
    otherwise"""
    if exp["kind"] == "bits":
        return check_bits(got, exp["want"], what=what), None
    return check_bound(got, exp["out"], exp["E"], what=what)


# ------------------------------------------------------------------------------------------------ case tables
_TL = [(t, lay) for t in ("bf16", "f32") for lay in ("k", "r")]
COMBOS = [(ta, la, tb, lb) for (ta, la) in _TL for (tb, lb) in _TL]
FAST_M, FAST_N, FAST_N_ODD = 200, 264, 262
# (K, requested split): what each reaches is in DESIGN.md's table; (392, 1) is the split_k = 1 neighbour of (392, 2)
FAST_K32 = [(8, 1), (40, 1), (136, 1), (136, 3), (384, 2), (392, 1)]
FAST_K64 = [(392, 2), (448, 2), (520, 2), (776, 3)]
FAST_CONTINUOUS = {(8, 1), (40, 1), (136, 1), (136, 3), (392, 2)}


def fast_cases():
    """all 16 operand combinations on every K row of both variants at 200 x 264, the further setting rotated so that
    each translation unit (variant, A type) sees every setting on every K row; K-major-B combinations also at
    N = 262 (scalar epilogue, scalar split store and scalar reduce)"""
    out = []
    for ci, (ta, la, tb, lb) in enumerate(COMBOS):
        wi = ci % 8                                          # index inside the (variant, A type) translation unit
        for ki, (k, split) in enumerate(FAST_K32 + FAST_K64):
            c = Case(f"fast-{ta}{la}-{tb}{lb}-k{k}s{split}", FAST_M, FAST_N, k, ta, la, tb, lb, BF16, split,
                     expect="fast_k32" if (k, split) in FAST_K32 else "fast_k64",
                     continuous=(k, split) in FAST_CONTINUOUS)
            out.append(with_setting(c, wi + ki))
        if lb == "k":
            for ki, (k, split, kern) in enumerate([(136, 1, "fast_k32"), (136, 3, "fast_k32"), (392, 2, "fast_k64")]):
                c = Case(f"fast-{ta}{la}-{tb}{lb}-n262-k{k}s{split}", FAST_M, FAST_N_ODD, k, ta, la, tb, lb, BF16,
                         split, expect=kern, continuous=ki == 0)
                # four combinations per (A type, row): consecutive settings, so each sees all four activations
                out.append(with_setting(c, wi // 2 + 3 * ki + (4 if ta == "f32" else 0)))
    return out


# outer * MT = 512 against 520 in the deep-variant rule (split 8, k_per_split 256 on both)
VARIANT_BOUNDARY = [
    with_setting(Case("fast-boundary-n8192", 128, 8192, 2048, "bf16", "k", "bf16", "k", BF16, 8, expect="fast_k64"), 1),
    with_setting(Case("fast-boundary-n8320", 128, 8320, 2048, "bf16", "k", "bf16", "k", BF16, 8, expect="fast_k32"), 4),
]

GENERIC_MN = (1, 63, 64, 65)
GENERIC_K = (1, 31, 32, 33, 63, 64, 65, 100)
GENERIC_GROUPS = [(comp, ta, tb, la, lb) for comp in (F32, BF16) for ta in ("f32", "bf16") for tb in ("f32", "bf16")
                  for la in ("k", "r") for lb in ("k", "r")]


def generic_cases(comp, ta, tb, la, lb):
    """every (M, N, K) of the grid for one compute type, operand type pair and pair of global -> LDS maps, plus the
    clamped (K = 33, 7 requested) and uneven (K = 100, 3 requested) splits.  C rotates through a plain array, a
    transposed view (scn != 1) and a column slice (scm > N); a case the fast kernel would take with a row-major C gets
    the transposed view."""
    shapes = [(m, n, k, 1) for m in GENERIC_MN for n in GENERIC_MN for k in GENERIC_K]
    shapes += [(m, n, k, s) for (m, n) in ((65, 63), (1, 65), (64, 64)) for (k, s) in ((33, 7), (100, 3), (65, 2))]
    out = []
    for i, (m, n, k, s) in enumerate(shapes):
        c = Case(f"generic-{'bf16' if comp == BF16 else 'f32'}-{ta}{la}-{tb}{lb}-{m}x{n}x{k}s{s}", m, n, k, ta, la, tb,
                 lb, comp, s, expect="generic_bf16" if comp == BF16 else "generic_f32", continuous=True)
        c = with_setting(c, i)
        view = i % 3
        if view == 2:
            c = dataclasses.replace(c, c_ld=n + 5)
        if view == 1 or plan_of(c)["kernel"].startswith("fast"):
            c = dataclasses.replace(c, c_t=True, c_ld=m + 3)
        out.append(c)
    return out


# split-K reduce: effective splits 2, 3, 5, 9, 17 in fp32 compute (K tile 32, K = 32 s), vector (N = 68) and scalar
# (N = 67) forms.  In the vector form each of 4 waves sums a quarter (ceil(s / 4) slabs) in an unrolled loop of four
# plus a tail: 2 and 3 leave waves without a slab, 17 gives 5 = 4 + 1 per quarter; the scalar form's loop of four
# plus tail sees 17 = 16 + 1.
REDUCE_CASES = [with_setting(Case(f"reduce-n{n}-s{s}", 65, n, 32 * s, "f32", "k", "f32", "r", F32, s,
                                  expect="generic_f32", continuous=True), i)
                for n in (68, 67) for i, s in enumerate((2, 3, 5, 9, 17), start=1 if n == 68 else 4)]


def _fb(name, **kw):
    base = dict(m=FAST_M, n=FAST_N, k=136, ta="f32", la="k", tb="f32", lb="k", comp=BF16)
    base.update(kw)
    return Case(f"fallback-{name}", **base)


# (reason, the neighbour that takes the fast path, the case that leaves it): the pair differs in the named property only
FALLBACKS = [
    ("A pointer 4 bytes off 16", _fb("a-ptr-fast"), _fb("a-ptr", a_off=1)),
    ("B pointer 4 bytes off 16", _fb("b-ptr-fast", tb="bf16"), _fb("b-ptr", tb="bf16", b_off=2)),
    ("K % 8 != 0 with a K-major bf16 operand", _fb("k8-fast", ta="bf16", a_ld=144, b_ld=144),
     _fb("k8", ta="bf16", k=132, a_ld=144, b_ld=144)),
    ("K % 4 != 0 with a K-major fp32 operand", _fb("k4-fast", k=132, a_ld=136, b_ld=136),
     _fb("k4", k=134, a_ld=136, b_ld=136)),
    ("row stride not a multiple of 16 bytes", _fb("ld-fast", a_ld=140), _fb("ld", a_ld=138)),
    ("rows % 8 != 0 with a row-major bf16 operand", _fb("rows8-fast", ta="bf16", la="r", a_ld=208),
     _fb("rows8", m=204, ta="bf16", la="r", a_ld=208)),
    ("scn != 1", _fb("scn-fast"), _fb("scn", c_t=True)),
    ("N % 4 == 0 with scm % 4 != 0", _fb("scm-fast", c_ld=268), _fb("scm", c_ld=266)),
    ("N % 4 == 0 with C off alignment", _fb("c-ptr-fast", c_ld=268, c_off=4), _fb("c-ptr", c_ld=268, c_off=1)),
    ("bias_n off 16 bytes", _fb("bias-fast", bias_n=True, bias_off=4), _fb("bias", bias_n=True, bias_off=1)),
    ("M N = 63 x 64 against 64 x 64", _fb("tiny-fast", m=64, n=64), _fb("tiny", m=63, n=64)),
]

# C inside a larger sentinel-filled buffer with spare columns right of N (the guard rows are on every case): the fast
# kernel's interior and edge tiles (one launch at 200 x 264 has both), its split store + reduce, the generic kernel
# with and without split, for both output types
GUARD_CASES = [dataclasses.replace(c, name=f"{c.name}-{tc}", tc=tc) for tc in ("f32", "bf16") for c in (
    Case("guard-fast", FAST_M, FAST_N, 136, "bf16", "k", "bf16", "r", BF16, 1, ACT_RELU, True, True, c_ld=272,
         expect="fast_k32"),
    Case("guard-fast-split", FAST_M, FAST_N, 392, "f32", "k", "f32", "k", BF16, 2, ACT_NONE, True, False, c_ld=272,
         expect="fast_k64"),
    Case("guard-fast-odd-n", FAST_M, FAST_N_ODD, 136, "f32", "k", "bf16", "k", BF16, 3, ACT_LEAKY, False, True,
         c_ld=267, expect="fast_k32"),
    Case("guard-generic", 65, 65, 33, "f32", "k", "f32", "r", F32, 1, ACT_LEAKY, True, True, c_ld=70,
         expect="generic_f32"),
    Case("guard-generic-bf16-split", 65, 68, 160, "bf16", "r", "f32", "k", BF16, 2, ACT_NONE, False, True, c_ld=72,
         expect="generic_bf16"),
    Case("guard-generic-transposed", 63, 65, 100, "f32", "r", "bf16", "r", F32, 3, ACT_RELU, True, False, c_t=True,
         c_ld=70, expect="generic_f32"))]
