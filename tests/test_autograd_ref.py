"""CPU tests of tests/autograd_ref.py: the float64 mirrors equal torch autograd in float64 on every geometry of the
case tables; the end-to-end check, with its measured bound, rejects every planted fault in both modes and passes the
unfaulted float32 baseline; and the tables reach the regimes they are there for (proved through the library's own
gemm plan and lowering_ref's plan mirrors, from the shapes alone: nothing is launched)."""
import pytest
import torch
import torch.nn.functional as F

import autograd_ref as R
import lowering_ref as L
from gan_des_midi_music_gen_amd import ops
from oracle import mmgan as OM
from oracle import simnn as OS

NAMES = [c["name"] for c in R.CASES]


def _autograd(name):
    """out, parameter gradients, input gradient and running statistics by torch autograd in float64"""
    c, inp = R.CASE[name], R.inputs(name)
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in inp["sd"].items()}
    x = inp["x"].double().requires_grad_(True)
    Rr = inp["R"].double()
    comp = c["composite"]
    if comp == "simnn_net":
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        y = F.max_pool2d(F.relu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"], padding=1)), 2, 2)
        y = F.max_pool2d(F.relu(F.conv2d(y, p["conv2.weight"], p["conv2.bias"], padding=1)), 2, 2)
        out = F.linear(F.relu(F.linear(y.flatten(1), p["fc1.weight"], p["fc1.bias"])), p["fc2.weight"], p["fc2.bias"])
        (out * Rr).sum().backward()
        return dict(out=out.detach(), grads={k: v.grad for k, v in p.items()}, dx=x.grad, running={})
    if comp == "simnn_gen":
        mod = OS.Generator(c["channels"], c["noise_dim"], c["gen_dim"])
        args = (x,)
    elif comp == "mlp_bn_sigmoid":
        if c["cls"] == "Generator":
            mod = OM.Generator(c["z_dim"], hidden_dim=c["hidden"], input_dim=c["input_dim"], adj_size=c["adj"])
        else:
            mod = OM.BeatGenerator(c["z_dim"], hidden_dim=c["hidden"], input_dim=c["input_dim"], output_dim=c["out"])
        args = (x[:, :c["z_dim"]], x[:, c["z_dim"]:])
    else:
        mod = OM.Discriminator(roll_size=c["roll"])
        args = (x,)
    mod.double()
    mod.load_state_dict(sd, strict=True)
    mod.train()
    out = mod(*args)
    (out * Rr).sum().backward()
    running = {k: (int(v) if k.endswith("num_batches_tracked") else v) for k, v in mod.state_dict().items()
               if "running" in k or "num_batches" in k}
    return dict(out=out.detach(), grads={k: p.grad for k, p in mod.named_parameters()}, dx=x.grad, running=running)


@pytest.mark.parametrize("name", NAMES)
def test_mirror_equals_autograd_in_float64(name):
    ref = _autograd(name)
    kw = dict(slope=0.2) if R.CASE[name]["composite"] == "mlp_leaky" else {}
    got = R.mirror(name, dtype=torch.float64, bf16=False, **kw)
    assert set(got["grads"]) == set(ref["grads"]), "the mirror names every parameter"
    ratios = R.e2e_ratios(R.CASE[name]["composite"], got, ref)
    assert set(ratios) == set(R.tensors_of(ref)), "every tensor compared"
    bad = {k: v for k, v in ratios.items() if not v <= 1e-10}
    assert not bad, bad
    for k, v in ref["running"].items():
        if k.endswith("num_batches_tracked"):
            assert got["running"][k] == v, k


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_every_fault_is_rejected_and_the_baseline_passes(name, bf16):
    comp = R.CASE[name]["composite"]
    bounds = R.family_bounds(R.family_of(name), bf16)
    print(name, "bf16" if bf16 else "fp32", "bounds", {k: f"{v:.3g}" for k, v in bounds.items()})
    if not bf16:
        assert all(v < 2.0 ** -10 for v in bounds.values()), bounds
    sub = R.mirror(name, dtype=torch.float32, bf16=bf16)
    ref = R.mirror(name, dtype=torch.float64, bf16=bf16, sel=sub["sel"] or None)
    fails, _, _ = R.check_e2e(name, bf16, sub, ref, what=name)
    assert not fails, fails
    clean = R.mirror(name, dtype=torch.float64, bf16=bf16)
    missed = []
    for fault in R.FAULTS[comp]:
        if not R.fault_present(fault, R.CASE[name], bf16):
            continue
        bad = R.mirror(name, dtype=torch.float64, bf16=bf16, faults=(fault,))
        fails, ratios, _ = R.check_e2e(name, bf16, bad, clean, what=f"{name} {fault}")
        required = R.fault_applies(fault, R.CASE[name], bf16)
        worst = max(v / bounds[R.kind_of(k)] for k, v in ratios.items())
        print(f"  {fault}: worst ratio / bound {worst:.3g}", "" if required else "(listed in BF16_BELOW_BASELINE)")
        assert max(ratios.values()) > 0, f"{fault} changes nothing"
        if required and not fails:
            missed.append(fault)
        if not required:
            assert worst < R.LISTED_BELOW, f"{fault} exceeds the bound {worst:.3g} times on {name}: require it"
    assert not missed, f"faults the end-to-end check lets through: {missed}"


def test_per_call_check_rejects_an_unrounded_operand():
    """bf16 mode's "one operand left unrounded" on the cases of BF16_BELOW_BASELINE, where the end-to-end bound cannot
    separate it from a value crossing a rounding boundary: a gemm whose A operand went in unrounded misses the
    per-call element bound."""
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(33, 64, generator=g), torch.randn(64, 48, generator=g)
    call = dict(name="gemm", args=(R.Rec(a), R.Rec(b)), kwargs=dict(compute=R.BF16), after=None)
    good = (a.bfloat16().double() @ b.bfloat16().double()).float()
    bad = (a.double() @ b.bfloat16().double()).float()
    call["results"] = (R.Rec(good),)
    fails, worst = R.check_call(call, ops)
    assert not fails and worst < 1.0, fails
    call["results"] = (R.Rec(bad),)
    fails, worst = R.check_call(call, ops)
    assert fails and worst > 100.0, worst


def _plans(bf16):
    out = []
    for c in R.CASES:
        for s in R.gemm_sites(c["name"], bf16, ops.linear_bn_act_max_rows()):
            out.append((c["name"], s, R.site_plan(s, ops)))
    return out


def test_tables_reach_the_regimes():
    """split-K off / on, both reduce kinds, the generic fp32 / bf16 and the fast bf16 kernels, K-major and row-major A,
    both col2im orders, the fused and unfused model 2 block, both BatchNorm row regimes"""
    plans = {bf16: _plans(bf16) for bf16 in (False, True)}
    every = plans[False] + plans[True]
    kernels = {p["kernel"] for _, _, p in every}
    assert {"generic_f32", "generic_bf16"} <= kernels, kernels
    # the fast bf16 kernels are reached too: among others by the reference generator's forward GEMMs of layers 1-3,
    # model 2's weight gradients and SimNN's conv2 / fc1 products
    fast = {f"{n}:{s['site']}": p["kernel"] for n, s, p in plans[True] if p["kernel"].startswith("fast")}
    assert {"gen-ref-B65:fwd1", "g1-rows300:dw0", "simnn-3x22x30-dx:conv2", "mlpd-B33-dx:dw0"} <= set(fast), fast
    print("fast bf16 kernels:", sorted(set(fast.values())), "at", len(fast), "call sites")
    assert not any(p["kernel"].startswith("fast") for _, _, p in plans[False])
    assert {p["reduce"] for _, _, p in every} >= {"none", "vector", "scalar"}, "both reduce kinds"
    assert {p["a_kmajor"] for _, _, p in every} == {True, False}, "K-major and row-major A"
    # split-K off and on at the same call site: layer 4's weight gradient of the reference generator, K = B * 256
    for bf16 in (False, True):
        dw3 = {n: p["split_k"] for n, s, p in plans[bf16] if s["site"] == "dw3" and n.startswith("gen-ref")}
        ks = {n: s["k"] for n, s, p in plans[bf16] if s["site"] == "dw3" and n.startswith("gen-ref")}
        assert ks == {"gen-ref-B2": 512, "gen-ref-B5": 1280, "gen-ref-B33": 8448, "gen-ref-B65": 16640}
        assert dw3["gen-ref-B2"] == 1 and dw3["gen-ref-B5"] > 1 and dw3["gen-ref-B65"] > 1, dw3
    # K = 37: no vector operand path (K % 4 != 0) -- the generic kernel, whatever the mode
    k37 = [p for n, s, p in plans[True] if n == "gen-c3-n37-g8-B3" and s["k"] == 37]
    assert k37 and all(p["kernel"] == "generic_bf16" for p in k37)
    # col2im: tap-major and torch order, the latter on a stride-2 layer too
    c2 = [s for c in R.GEN_CASES for s in R.col2im_sites(c["name"])]
    assert any(s["tap_major"] and s["stride"] == 2 for s in c2)
    assert any(not s["tap_major"] and s["stride"] == 2 for s in c2), "cout < 16 on a stride-2 layer"
    assert any(not s["tap_major"] and s["stride"] == 1 for s in c2)
    assert R.CASE["gen-c3-n37-g8-B3"]["channels"] > 1 and R.CASE["gen-c3-n37-g8-B3"]["noise_dim"] % 4
    # model 2: the fused block up to its last row count, the unfused one beyond and in fp32
    mr = ops.linear_bn_act_max_rows()
    rows = {c["B"] for c in R.MLP_BN_CASES}
    assert mr in rows and mr + 1 in rows and min(rows) == 2
    assert not any(s["site"].startswith("fwd") for n, s, p in plans[True] if n.endswith(f"rows{mr}") and n[0] == "g")
    assert any(s["site"].startswith("fwd") for n, s, p in plans[True] if n.endswith(f"rows{mr + 1}"))
    assert any(s["site"].startswith("fwd") for n, s, p in plans[False] if n.endswith("rows2"))
    # both BatchNorm row regimes (row_chunks capped at 64 chunks from 16384 rows on)
    regs = [L.bn_regimes(r, c) for case in R.CASES for (r, c) in R.bn_sites(case["name"])]
    assert {r["capped"] for r in regs} == {True, False}
    assert max(r for case in R.GEN_CASES for (r, _) in R.bn_sites(case["name"])) == 65 * 256 > 16384
    assert {r["chunks"] for r in regs} >= {1, 2, 64}
