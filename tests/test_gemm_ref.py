"""CPU: tests/gemm_ref.py checked before it is used -- the checker rejects every planted fault in both input families,
materialize() lays the operands out as layout() says, and the case tables of tests/test_gemm_edges_gpu.py reach the
kernels, variants, fall-backs and reduce forms they name.  The last is asked of the library itself (gdm_gemm_plan on
fake pointers of the cases' alignment), not of a mirror of its dispatch."""
import pytest
import torch

import gemm_ref as gr
from gemm_ref import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F32, Case

FAULT_CASES = [
    Case("faults-fast-k32", 200, 264, 136, "f32", "k", "f32", "r", BF16, 3, ACT_LEAKY, True, True, "f32"),
    Case("faults-fast-k64", 200, 264, 392, "f32", "r", "bf16", "k", BF16, 2, ACT_NONE, True, False, "bf16"),
    Case("faults-fast-k8", 200, 264, 8, "f32", "k", "f32", "k", BF16, 1, ACT_LEAKY, True, True, "f32"),
    Case("faults-generic-f32", 65, 68, 160, "f32", "k", "f32", "r", F32, 5, ACT_LEAKY, True, True, "f32"),
    Case("faults-generic-bf16", 65, 63, 100, "f32", "r", "f32", "k", BF16, 2, ACT_RELU, True, False, "bf16"),
]


@pytest.mark.parametrize("family", ["exact", "continuous"])
@pytest.mark.parametrize("c", FAULT_CASES, ids=lambda c: c.name)
def test_checker_rejects_every_planted_fault(c, family):
    plan, inp = gr.plan_of(c), gr.inputs(c, family)
    clean = gr.expected(c, inp, plan)
    assert clean["kind"] == ("bits" if family == "exact" else "bound")
    own = gr.rnd(clean["out"], gr.TDT[c.tc])
    fails, _ = gr.check(own, clean, what=c.name)
    assert fails == [], "the reference fails its own checker"
    for f in gr.FAULTS:
        if not gr.fault_applies(f, c, plan, family):
            continue
        wrong = gr.rnd(gr.expected(c, inp, plan, faults=(f,))["out"], gr.TDT[c.tc])
        fails, _ = gr.check(wrong, clean, what=f)
        assert fails, f"{c.name} / {family}: planted fault {f} passes the checker"


def test_every_fault_is_planted_in_every_family_it_applies_to():
    planted = {fam: {f for c in FAULT_CASES for f in gr.FAULTS if gr.fault_applies(f, c, gr.plan_of(c), fam)}
               for fam in ("exact", "continuous")}
    assert planted["continuous"] == set(gr.FAULTS)
    assert planted["exact"] == set(gr.FAULTS) - {"truncate_operand"}      # integers are exact in bf16


def test_truncation_is_far_outside_the_bound_at_k8_and_hides_at_k392():
    """why the continuous family is run at small K and the exact family carries the long ones"""
    def worst(c):
        plan, inp = gr.plan_of(c), gr.inputs(c, "continuous")
        clean = gr.expected(c, inp, plan)
        wrong = gr.expected(c, inp, plan, faults=("truncate_operand",))["out"]
        return float(((wrong - clean["out"]).abs() / clean["E"]).max())
    assert worst(Case("t8", 200, 264, 8)) > 1000
    assert worst(Case("t8", 200, 264, 8)) > 20 * worst(Case("t392", 200, 264, 392, split=2))


def test_sigmoid_on_exact_inputs_is_held_to_the_sigmoid_error_alone():
    c = Case("s", 200, 264, 136, act=ACT_SIGMOID, bias_n=True, bias_m=True)
    inp = gr.inputs(c, "exact")
    pre = inp["a"].double() @ inp["b"].double() + inp["bias_n"].double() + inp["bias_m"].double()[:, None]
    assert torch.equal(pre.float().double(), pre), "pre-activations are exact in fp32"
    assert 4 < float(pre.abs().max()) < 40 and float(pre.std()) > 1
    exp = gr.expected(c, inp, gr.plan_of(c))
    assert float((exp["E"] / exp["out"]).max()) < 8 * 2.0 ** -23


@pytest.mark.parametrize("c", [gr.FALLBACKS[1][2], gr.FALLBACKS[5][1], gr.FALLBACKS[8][2], gr.GUARD_CASES[5],
                               gr.GUARD_CASES[8], gr.generic_cases(F32, "bf16", "f32", "r", "k")[37]],
                         ids=lambda c: c.name)
def test_materialize_builds_the_views_layout_describes(c):
    inp = gr.inputs(c, "exact")
    t, L = gr.materialize(c, inp, "cpu"), gr.layout(c)
    assert t["a"].stride() == (L["sam"], L["sak"]) and t["b"].stride() == (L["sbk"], L["sbn"])
    assert t["out"].stride() == (L["scm"], L["scn"]) and t["out"].shape == (c.m, c.n)
    assert torch.equal(t["a"].float(), inp["a"]) and torch.equal(t["b"].float(), inp["b"])
    assert t["a"].data_ptr() % 16 == (c.a_off * gr.ESZ[c.ta]) % 16
    assert t["b"].data_ptr() % 16 == (c.b_off * gr.ESZ[c.tb]) % 16
    assert t["out"].data_ptr() % 16 == (L["c_at"] * gr.ESZ[c.tc]) % 16
    if c.bias_n:
        assert t["bias_n"].data_ptr() % 16 == (c.bias_off * 4) % 16
    assert int(t["outside"].sum()) == L["c_len"] - c.m * c.n and gr.untouched(t)
    t["out"][c.m - 1, c.n - 1] = 1.0
    assert gr.untouched(t)
    t["cbuf"][L["c_at"] - 1] = 1.0                     # the element in front of C
    assert not gr.untouched(t)


# ---------------------------------------------------------------------------------- what the tables reach
def _all_cases():
    cs = gr.fast_cases() + gr.VARIANT_BOUNDARY + gr.REDUCE_CASES + gr.GUARD_CASES
    for g in gr.GENERIC_GROUPS:
        cs += gr.generic_cases(*g)
    return cs


def test_every_case_runs_the_kernel_it_names():
    for c in _all_cases():
        for v in (c, c.plain()):
            p = gr.plan_of(v)
            assert p["kernel"] == c.expect, (v, p)
            if p["kernel"].startswith("fast"):
                assert (p["a_kmajor"], p["b_kmajor"]) == (c.la == "k", c.lb == "k"), (v, p)
            assert p["workspace_bytes"] == (p["split_k"] * c.m * c.n * 4 if p["split_k"] > 1 else 0)
            assert (p["reduce"] == "none") == (p["split_k"] == 1)


def test_all_32_fast_instances_and_every_setting_in_every_translation_unit():
    inst, settings = set(), {}
    for c in gr.fast_cases():
        p = gr.plan_of(c)
        inst.add((p["kernel"], c.ta, p["a_kmajor"], c.tb, p["b_kmajor"]))
        if c.n == gr.FAST_N:
            settings.setdefault((p["kernel"], c.ta, c.k, p["split_k"]), set()).add(c.setting())
    assert len(inst) == 32 and {i[0] for i in inst} == {"fast_k32", "fast_k64"}
    # each translation unit gemm_bf16_kt{32,64}_{bf16,f32}a.hip, on every K row: all four activations, all four bias
    # settings and both output types -- on the unsplit rows (interior and edge epilogues) and on the split ones
    assert len(settings) == 2 * len(gr.FAST_K32 + gr.FAST_K64)
    for key, s in settings.items():
        assert {x[0] for x in s} == {ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID}, key
        assert {(x[1], x[2]) for x in s} == {(False, False), (True, False), (False, True), (True, True)}, key
        assert {x[3] for x in s} == {"f32", "bf16"}, key
    # N = 262: scalar epilogue and scalar reduce on every (variant, A type, A layout, B type)
    odd = {(gr.plan_of(c)["kernel"], c.ta, c.la, c.tb, gr.plan_of(c)["reduce"]) for c in gr.fast_cases()
           if c.n == gr.FAST_N_ODD}
    assert len(odd) == 8 * 3 and {o[4] for o in odd} == {"none", "scalar"}
    acts = {}
    for c in gr.fast_cases():
        if c.n == gr.FAST_N_ODD:
            acts.setdefault((c.expect, c.ta, c.k, c.split), set()).add(c.act)
    assert len(acts) == 6 and all(len(a) == 4 for a in acts.values()), acts


def test_the_k_rows_split_as_the_table_says():
    def row(k, split):
        return gr.plan_of(Case("row", gr.FAST_M, gr.FAST_N, k, "bf16", "k", "bf16", "k", BF16, split))
    want = {(8, 1): ("fast_k32", 1, 64), (40, 1): ("fast_k32", 1, 64), (136, 1): ("fast_k32", 1, 192),
            (136, 3): ("fast_k32", 3, 64), (384, 2): ("fast_k32", 2, 192), (392, 1): ("fast_k32", 1, 448),
            (392, 2): ("fast_k64", 2, 256), (448, 2): ("fast_k64", 2, 256), (520, 2): ("fast_k64", 2, 320),
            (776, 3): ("fast_k64", 3, 320)}
    for (k, split), w in want.items():
        p = row(k, split)
        assert (p["kernel"], p["split_k"], p["k_per_split"]) == w, (k, split, p)
    # the slices of the deep variant are interleaved 64-wide tiles: 392 -> 4 + 3 tiles (the odd slice ends in the zero
    # pair-tail, the ragged 8-wide tile 6 falls in slice 0), 520 -> 5 + 4, 776 -> 5 + 4 + 4
    tiles = lambda k, s: [len(set((gr.slab_ks(row(k, s), k, z) // 64).tolist())) for z in range(s)]
    assert tiles(392, 2) == [4, 3] and tiles(448, 2) == [4, 3] and tiles(520, 2) == [5, 4]
    assert tiles(776, 3) == [5, 4, 4]
    assert gr.slab_ks(row(392, 2), 392, 0)[-8:].tolist() == list(range(384, 392))
    # K tile 32, split 3 at K = 136: 32-wide tiles 2 / 2 / 1
    assert [len(set((gr.slab_ks(row(136, 3), 136, z) // 32).tolist())) for z in range(3)] == [2, 2, 1]


def test_both_sides_of_each_term_of_the_variant_rule():
    """split_k > 1 && outer * MT <= 512 && k_per_split >= 256, each term flipped alone"""
    by = {c.name: gr.plan_of(c) for c in gr.fast_cases() + gr.VARIANT_BOUNDARY}
    deep, no_split, short = by["fast-bf16k-bf16k-k392s2"], by["fast-bf16k-bf16k-k392s1"], by["fast-bf16k-bf16k-k384s2"]
    assert deep["kernel"] == "fast_k64" and deep["split_k"] == 2 and deep["k_per_split"] == 256
    assert no_split["kernel"] == "fast_k32" and no_split["split_k"] == 1 and no_split["k_per_split"] >= 256
    assert short["kernel"] == "fast_k32" and short["split_k"] == 2 and short["k_per_split"] == 192
    at, over = by["fast-boundary-n8192"], by["fast-boundary-n8320"]
    assert (at["kernel"], at["split_k"], at["k_per_split"]) == ("fast_k64", 8, 256)          # 64 n tiles x 8 = 512
    assert (over["kernel"], over["split_k"], over["k_per_split"]) == ("fast_k32", 8, 256)    # 65 n tiles x 8 = 520


@pytest.mark.parametrize("reason,fast,fallen", gr.FALLBACKS, ids=[f[2].name for f in gr.FALLBACKS])
def test_each_fallback_reason_leaves_the_fast_path_beside_a_neighbour_that_takes_it(reason, fast, fallen):
    assert gr.plan_of(fast)["kernel"] == "fast_k32", reason
    assert gr.plan_of(fallen)["kernel"] == "generic_bf16", reason


def test_reduce_cases_reach_both_forms_at_every_split():
    got = {(c.n, gr.plan_of(c)["split_k"], gr.plan_of(c)["reduce"]) for c in gr.REDUCE_CASES}
    assert got == {(n, s, r) for n, r in ((68, "vector"), (67, "scalar")) for s in (2, 3, 5, 9, 17)}
    assert {(c.tc, c.bias_n, c.bias_m) for c in gr.REDUCE_CASES} >= {("bf16", True, True), ("f32", True, False),
                                                                      ("bf16", False, True)}


def test_generic_tables_cover_maps_views_and_clamped_splits():
    views, splits = set(), {}
    for g in gr.GENERIC_GROUPS:
        for c in gr.generic_cases(*g):
            L = gr.layout(c)
            views.add("transposed" if L["scn"] != 1 else "sliced" if L["scm"] > c.n else "plain")
            if c.split > 1:
                splits[(c.comp, c.k, c.split)] = gr.plan_of(c)["split_k"]
    assert views == {"plain", "transposed", "sliced"}
    # 7 requested at K = 33: clamped by the tile count (2 tiles of 32, 1 of 64); 3 requested at K = 100: 4 tiles of 32
    # in slabs of 2 (64 + 36), 2 tiles of 64 (64 + 36)
    assert splits == {(F32, 33, 7): 2, (BF16, 33, 7): 1, (F32, 100, 3): 2, (BF16, 100, 3): 2, (F32, 65, 2): 2,
                      (BF16, 65, 2): 2}
    assert len(gr.GENERIC_GROUPS) == 2 * 4 * 4
