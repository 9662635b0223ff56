"""GPU: every gdm_gemm kernel instance against float64 (tests/gemm_ref.py states the two input families, the bound
and the case tables; tests/test_gemm_ref.py proves on the CPU, through gdm_gemm_plan, what the tables reach).

Every call here first asserts the library's plan -- of the case's description and of the actual device tensors -- so
a case that did not run the kernel it names fails for that reason.  The exact family must match the float64 result
rounded once to C's type in every bit of every element; the continuous family must stay inside the derived bound
(K + split_k + 2) 2^-23 Mag (+ activation, + half a bf16 ulp).  Every call writes C inside a sentinel-filled buffer
whose other elements must be unchanged afterwards, and every split-K call is made twice with equal results.

Measured on MI355X (helpers.record has each test's figures): every exact-family element bit-equal; worst |err| / bound
of the continuous family with fp32 output 0.22 (generic kernel, fp32 compute; the fast kernels 0.10), with the sigmoid
epilogue 0.19; with bf16 output 0.995, which is the output's own half ulp (the bound's last term) and says nothing about
the sum; exact inputs through the sigmoid 0.27 of SIGMOID_ULPS.  The whole file -- 251 tests -- takes 8.8 s of wall
time, the slowest test 0.5 s.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402

import gemm_ref as gr  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"


def run(c, family, fails, ratios, inp=None):
    """one call of case c on inputs of `family`: plan, result, sentinels, repeatability.  Failures are collected."""
    plan = gr.plan_of(c)
    inp = gr.inputs(c, family) if inp is None else inp
    t = gr.materialize(c, inp, DEV)
    kw = dict(bias_n=t["bias_n"], bias_m=t["bias_m"], act=c.act, slope=c.slope, compute=c.comp, split_k=c.split,
              out=t["out"])
    live = ops.gemm_plan(t["a"], t["b"], **kw)
    assert live == plan, f"{c.name}: the device tensors' plan {live} is not the description's {plan}"
    assert plan["kernel"] == c.expect, f"{c.name}: runs {plan['kernel']}, meant for {c.expect}: {plan}"
    ops.gemm(t["a"], t["b"], **kw)
    got = t["out"].contiguous().cpu()
    if plan["split_k"] > 1:
        first = t["cbuf"].clone()
        ops.gemm(t["a"], t["b"], **kw)
        if not torch.equal(first, t["cbuf"]):
            fails.append(f"{c.name} {family}: two runs of the split-K call differ")
    if not gr.untouched(t):
        bad = ((t["cbuf"] != gr.SENTINEL) & t["outside"]).nonzero().flatten()[:4].tolist()
        fails.append(f"{c.name} {family}: wrote outside C, buffer elements {bad} (C starts at {gr.layout(c)['c_at']}, "
                     f"ld {gr.layout(c)['c_ld']})")
    what = f"{c.name} {family} [{plan['kernel']} split {plan['split_k']} x {plan['k_per_split']}, {plan['reduce']}]"
    f, ratio = gr.check(got, gr.expected(c, inp, plan), what=what)
    fails += f
    if ratio is not None:
        # the fp32-output ratios show the arithmetic; a bf16 output is dominated by its own half ulp (ratio near 1 by
        # construction), the exact family's sigmoid by SIGMOID_ULPS
        ratios[f"{c.name} {family}"] = (ratio, f"{family}_{c.tc}{'_sigmoid' if c.act == gr.ACT_SIGMOID else ''}")


def run_all(c, fails, ratios):
    """the exact family with fp32 output and no epilogue, the exact family with the case's own setting, and the
    continuous family (own setting) where the table asks for it"""
    if c.setting() != c.plain().setting():
        run(c.plain(), "exact", fails, ratios)
    run(c, "exact", fails, ratios)
    if c.continuous:
        run(c, "continuous", fails, ratios)


def finish(name, fails, ratios):
    worst = {}
    for ratio, kind in ratios.values():
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    record(f"gemm_edges {name}", calls=len(ratios), **worst)
    assert not fails, "\n".join(fails)


_FAST = gr.fast_cases()


@pytest.mark.parametrize("c", _FAST, ids=[c.name for c in _FAST])
def test_fast_kernel_instances(c):
    fails, ratios = [], {}
    run_all(c, fails, ratios)
    finish(c.name, fails, ratios)


@pytest.mark.parametrize("c", gr.VARIANT_BOUNDARY, ids=[c.name for c in gr.VARIANT_BOUNDARY])
def test_deep_variant_boundary_of_the_grid_term(c):
    torch.set_num_threads(16)
    fails, ratios = [], {}
    run_all(c, fails, ratios)
    finish(c.name, fails, ratios)


@pytest.mark.parametrize("comp,ta,tb,la,lb", gr.GENERIC_GROUPS,
                         ids=[f"{'bf16' if g[0] else 'f32'}-{g[1]}{g[3]}-{g[2]}{g[4]}" for g in gr.GENERIC_GROUPS])
def test_generic_kernel_grid(comp, ta, tb, la, lb):
    fails, ratios = [], {}
    for c in gr.generic_cases(comp, ta, tb, la, lb):
        run(c, "exact", fails, ratios)
        run(c, "continuous", fails, ratios)
    finish(f"generic {comp} {ta}{la} {tb}{lb}", fails, ratios)


@pytest.mark.parametrize("c", gr.REDUCE_CASES, ids=[c.name for c in gr.REDUCE_CASES])
def test_split_k_reduce(c):
    fails, ratios = [], {}
    run_all(c, fails, ratios)
    finish(c.name, fails, ratios)


@pytest.mark.parametrize("reason,fast,fallen", gr.FALLBACKS, ids=[f[2].name for f in gr.FALLBACKS])
def test_fallbacks_beside_their_fast_neighbours(reason, fast, fallen):
    """both of a pair on the same values (where their shapes differ, the smaller one's are a corner of the larger
    one's); both bit-exact"""
    fails, ratios = [], {}
    big = gr.inputs(dataclasses.replace(fast, m=max(fast.m, fallen.m), k=max(fast.k, fallen.k)), "exact")
    for c, kern in ((fast, "fast_k32"), (fallen, "generic_bf16")):
        run(dataclasses.replace(c, expect=kern), "exact", fails, ratios, inp=gr.crop(big, c))
    finish(fallen.name, fails, ratios)


@pytest.mark.parametrize("c", gr.GUARD_CASES, ids=[c.name for c in gr.GUARD_CASES])
def test_nothing_outside_c_is_written(c):
    """C is a view with spare columns right of N inside the sentinel-filled buffer (guard rows are on every case)"""
    assert gr.layout(c)["c_ld"] > gr.layout(c)["c_cols"]
    fails, ratios = [], {}
    run(c, "exact", fails, ratios)
    run(c, "continuous", fails, ratios)
    finish(c.name, fails, ratios)
