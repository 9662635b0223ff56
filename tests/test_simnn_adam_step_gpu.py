"""GPU: model 1's one-launch optimizer step (gdm_simnn_adam_step) and the transposing Adam it shares its tile body with
(gdm_adam_step_dev_pc), called directly on synthetic buffers at the edges of their launch plans -- tests/adam_fused_ref.py
holds the case tables and says what each case reaches (the 16-byte non-temporal path, grids of 1 / 63 / 64 / 65 / 2080 /
2113 workgroups, partial tiles, misaligned arrays, the scalar tail of the small range).

Every launch is held to
  float64     p, m, v of both ranges against ONE lowering_ref.adam_ref step from the kernel's own previous state, within
              the bounds adam_ref derives (ratio <= 1; the worst ratios go to helpers.record "simnn_adam_step");
  the chain   gdm_adam_step_dev(small) + gdm_adam_step_dev_pc(big, advance_step=False) + gdm_simnn_conv2_pack on cloned
              state with a `hyper` of its own: p, m, v, operand copy, pack and all 8 floats of `hyper`, bit for bit;
  the copies  operand copy = rnd(p') permuted to (N, P, C); pack = adam_fused_ref.conv2_pack_ref(updated conv2.weight);
  the record  adam_fused_ref.check_record, and the cached floats bit-equal to the hyper[6:8] adam_prep derives a step later;
  the guards  64 elements of a known pattern on both sides of every buffer the kernels write, bit-unchanged.
State: m small randn, v small positive, from step 2 on the kernel's own; gradients randn * 10^-step; a few elements of
both ranges have g == 0 in every step, some of them also m == v == 0 (the denominator at its eps floor).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import ops  # noqa: E402
from gan_des_midi_music_gen_amd.ops import BF16, F32  # noqa: E402

import adam_fused_ref as A  # noqa: E402
import lowering_ref as R  # noqa: E402
from helpers import record  # noqa: E402

DEV = "cuda"
DT = {torch.float32: F32, torch.bfloat16: BF16}
TYPES = (torch.float32, torch.bfloat16)
GUARD = 64
PATTERN = {torch.float32: -1234.5, torch.bfloat16: -1234.0, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """a device buffer of n elements with GUARD elements of PATTERN before and behind it; `offset` more elements in
    front move the view off its 16-byte alignment"""

    def __init__(self, n, dtype, offset=0, src=None, name=""):
        self.name, self.lo = name, GUARD + offset
        self.buf = torch.full((self.lo + n + GUARD,), PATTERN[dtype], dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == (offset * self.buf.element_size()) % 16 and self.t.is_contiguous()
        if src is None:
            self.t.zero_()
        else:
            self.t.copy_(src.reshape(-1))

    def check(self, what):
        lo, hi = self.buf[:self.lo].cpu(), self.buf[self.lo + self.t.numel():].cpu()
        want = torch.full((1,), PATTERN[self.buf.dtype], dtype=self.buf.dtype)
        bad = int((R.bits(lo) != R.bits(want)).sum()) + int((R.bits(hi) != R.bits(want)).sum())
        return [f"{what}: {bad} guard element(s) around {self.name} overwritten"] if bad else []


def _planted(n):
    """(indices with g == 0 in every step, those that also start with m == v == 0)"""
    z = sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n)))
    return z, z[1::2]


class Step:
    """the buffers of one optimizer (big range, small range, operand copy, pack, hyper, record), guarded, plus the
    chain's hyper; `launch` performs one step both ways and checks it"""

    def __init__(self, big, small, dtype, hp, seed, *, first_step=1, with_small=True):
        self.N, self.C, self.P, big_aligned = big
        self.dtype, self.hp, self.step = dtype, hp, first_step - 1
        self.what = f"big {big} small {small} {dtype} betas ({hp[1]:.3g}, {hp[2]:.3g})"
        g = _gen(seed)
        nb = self.nb = self.N * self.C * self.P
        off = 0 if big_aligned else 1
        self.zb, zb0 = _planted(nb)
        m0, v0 = torch.randn(nb, generator=g) * 1e-3, torch.rand(nb, generator=g) * 1e-5 + 1e-12
        m0[zb0], v0[zb0] = 0.0, 0.0
        self.p = Guarded(nb, torch.float32, off, torch.randn(nb, generator=g), "p")
        self.m, self.v = Guarded(nb, torch.float32, off, m0, "m"), Guarded(nb, torch.float32, off, v0, "v")
        self.shadow = Guarded(nb, dtype, 0, None, "operand copy")
        self.hyper = Guarded(8, torch.float32, 0, self._hyper(hp, self.step), "hyper")
        self.c_hyper = self._hyper(hp, self.step).to(DEV)
        self.guarded = [self.p, self.m, self.v, self.shadow, self.hyper]
        self.with_small = with_small
        if with_small:
            self.ns, self.w2_off, small_aligned = small
            ns, offs = self.ns, 0 if small_aligned else 1
            self.zs, zs0 = _planted(ns)
            ms0, vs0 = torch.randn(ns, generator=g) * 1e-3, torch.rand(ns, generator=g) * 1e-5 + 1e-12
            ms0[zs0], vs0[zs0] = 0.0, 0.0
            self.ps = Guarded(ns, torch.float32, offs, torch.randn(ns, generator=g) * 0.1, "small p")
            self.ms, self.vs = Guarded(ns, torch.float32, offs, ms0, "small m"), Guarded(ns, torch.float32, offs, vs0, "small v")
            self.gs = Guarded(ns, torch.float32, offs, None, "small g")
            self.pack = Guarded(A.pack_elems(dtype) * self.shadow.t.element_size(), torch.uint8, 0, None, "pack")
            self.rec = Guarded(A.REC_INTS, torch.int32, 0, None, "record")
            self.guarded += [self.ps, self.ms, self.vs, self.pack, self.rec]
        self.gen = g
        self.worst = {}
        self.cached = None                               # the record's floats for the coming step, from the last launch

    @staticmethod
    def _hyper(hp, step):
        h = torch.zeros(8)
        h[1:6] = torch.tensor(hp)
        h.view(torch.int32)[0] = step
        return h

    def rewrite(self, hp=None, step=None):
        """the host rewrites `hyper` (both optimizers') and zeroes the record, as include/gdm.h requires"""
        if hp is not None:
            self.hp = hp
        if step is not None:
            self.step = step
        for h in (self.hyper.t, self.c_hyper):
            h[1:6].copy_(torch.tensor(self.hp))
            h.view(torch.int32)[0:1].copy_(torch.tensor([self.step], dtype=torch.int32))
        self.rec.t.zero_()
        self.cached = None

    def gradients(self, step):
        gb = torch.randn(self.nb, generator=self.gen) * 10.0 ** -step            # in (N, C, P) order
        gb[self.zb] = 0.0
        g_pc = gb.view(self.N, self.C, self.P).permute(0, 2, 1).contiguous()
        gs = None
        if self.with_small:
            gs = torch.randn(self.ns, generator=self.gen) * 10.0 ** -step
            gs[self.zs] = 0.0
        return g_pc, gs

    def state(self):
        """bit-comparable copies of everything the step writes"""
        names = ("p", "m", "v", "shadow", "hyper") + (("ps", "ms", "vs", "pack") if self.with_small else ())
        return {k: getattr(self, k).t.cpu().clone() for k in names}

    def launch(self, rows=None):
        """one step: the one-launch kernel on the guarded buffers, the chain on clones.  rows: the rows n of the big
        range that are compared with float64 (all when None); the chain comparison always covers every element."""
        N, C, P, hp = self.N, self.C, self.P, self.hp
        self.step += 1
        step, what = self.step, f"{self.what} step {self.step}"
        g_pc, gs = self.gradients(step)
        g_dev = g_pc.to(DEV)
        self.gs.t.copy_(gs)
        before = self.state()
        # ---- the chain, on clones
        c = {k: getattr(self, k).t.clone() for k in ("p", "m", "v", "ps", "ms", "vs")}
        c_shadow = torch.empty(N * P * C, dtype=self.dtype, device=DEV)
        c_pack = torch.empty_like(self.pack.t)
        ops.adam_step_dev(c["ps"], self.gs.t.clone(), c["ms"], c["vs"], self.c_hyper)
        ops.adam_step_dev_pc(c["p"], g_dev.view(-1), c["m"], c["v"], N, C, P, c_shadow, self.c_hyper, advance_step=False)
        ops.simnn_conv2_pack(c["ps"][self.w2_off:self.w2_off + A.W2_ELEMS].view(32, 16, 3, 3), DT[self.dtype], out=c_pack)
        nxt_hyper = self.c_hyper.clone()                 # what adam_prep derives one step later
        dummy = torch.zeros(4, 4, device=DEV)
        ops.adam_step_dev(dummy[0], dummy[1], dummy[2], dummy[3], nxt_hyper)
        # ---- the one launch
        ops.simnn_adam_step(self.p.t, g_dev.view(-1), self.m.t, self.v.t, N, C, P, self.shadow.t, self.ps.t, self.gs.t,
                            self.ms.t, self.vs.t, self.ps.t[self.w2_off:self.w2_off + A.W2_ELEMS], self.pack.t,
                            self.hyper.t, self.rec.t)
        torch.cuda.synchronize()
        after = self.state()
        fails = []
        for b in self.guarded:
            fails += b.check(what)
        # 2. the chain, bit for bit
        chain = dict(c, shadow=c_shadow, pack=c_pack, hyper=self.c_hyper)
        for k, t in chain.items():
            fails += R.check_bits(after[k], t, what=f"{what} {k} vs the chain")
        # 1. float64, one step from the state before; 3. the operand copy
        sel = slice(None) if rows is None else rows

        def rows_of(t, shape):
            return t.view(*shape)[sel].contiguous()

        n_sel = rows_of(before["p"], (N, C, P)).shape[0]
        ref = A.pc_step_ref(rows_of(before["p"], (N, C, P)), rows_of(g_pc, (N, P, C)), rows_of(before["m"], (N, C, P)),
                            rows_of(before["v"], (N, C, P)), n_sel, C, P, step, hp, self.dtype)
        got = {k: rows_of(after[k], (N, C, P)) for k in "pmv"}
        got["shadow"] = rows_of(after["shadow"], (N, P, C))
        f, w = A.check_pc(got, ref, what=f"{what} big")
        fails += f
        self._worst("big", w)
        want = R.rnd(after["p"].view(N, C, P), self.dtype).permute(0, 2, 1).contiguous().view(-1)
        fails += R.check_bits(after["shadow"], want, what=f"{what} operand copy (all rows)")
        ref_s = R.adam_ref(before["ps"], gs, before["ms"], before["vs"], step, *hp)
        f, w = R.check_adam(dict(p=after["ps"], m=after["ms"], v=after["vs"]), ref_s, what=f"{what} small")
        fails += f
        self._worst("small", w)
        # 4. the pack
        w2 = after["ps"][self.w2_off:self.w2_off + A.W2_ELEMS]
        fails += R.check_bits(after["pack"].view(self.dtype), A.conv2_pack_ref(w2, self.dtype), what=f"{what} pack")
        # 5. the record
        rec = self.rec.t.cpu()
        fails += A.check_record(rec, step, hp, what=what)
        nxt = A.REC_SLOT0 + 4 * ((step + 1) & 1)
        fails += R.check_bits(rec[nxt + 1:nxt + 3].view(torch.float32), nxt_hyper[6:8], what=f"{what} cached terms vs "
                              "the next adam_prep")
        if self.cached is not None:                      # what the previous launch cached is what this one applied
            fails += R.check_bits(after["hyper"][6:8], self.cached, what=f"{what} hyper[6:8] vs the cached terms")
        self.cached = rec[nxt + 1:nxt + 3].view(torch.float32).clone()
        if int(after["hyper"].view(torch.int32)[0]) != step:
            fails.append(f"{what}: device step counter {int(after['hyper'].view(torch.int32)[0])}")
        return fails

    def _worst(self, rng, w):
        for k, x in w.items():
            self.worst[f"{rng}_{k}"] = max(self.worst.get(f"{rng}_{k}", 0.0), x)


HP = [A.hyper32(lr, betas, A.EPS, gs) for betas, lr, gs in A.HYPER_SETS]
_final = {}                                              # (big name, small, dtype, hyper set) -> final state


def _run(big_name, small, dtype, hi, *, fresh=False):
    key = (big_name, small, dtype, hi)
    if key in _final and not fresh:
        return [], _final[key]
    # the seed leaves out the alignment flags: a misaligned case starts from the state of its aligned twin
    s = Step(A.BIG_CASES[big_name], small, dtype, HP[hi], seed=sum(A.BIG_CASES[big_name][:3]) * 7 + small[0] + hi)
    rows = slice(0, None, 4) if big_name == "G" else None
    fails = []
    for _ in range(A.BIG_STEPS[big_name]):
        fails += s.launch(rows)
    record("simnn_adam_step", big=big_name, small=list(small), dtype=str(dtype), hyper=hi,
           **{k: round(x, 4) for k, x in s.worst.items()})
    assert all(x <= 1.0 for x in s.worst.values()) or fails, s.worst
    _final.setdefault(key, s.state())
    return fails, s.state()


def _twin(state_a, state_b, what):
    fails = []
    for k in state_a:
        fails += R.check_bits(state_a[k], state_b[k], what=f"{what} {k}")
    return fails


PAIRS = [(b, s) for b, s in A.STEP_PAIRS if b != "G"]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("big,small", PAIRS, ids=[f"{b}-{s[0]}+{s[1]}{'' if s[2] else 'u'}" for b, s in PAIRS])
def test_one_launch_step(big, small, dtype):
    """six steps under both hyper-parameter sets.  A misaligned case (big H; the small range one float into its
    buffers) must in addition end bit-equal to its aligned twin."""
    fails = []
    for hi in range(len(HP)):
        f, state = _run(big, small, dtype, hi)
        fails += f
        if big == "H":
            f, twin = _run("C", small, dtype, hi)
            fails += f + _twin(state, twin, "misaligned H vs aligned C")
        if not small[2]:
            f, twin = _run(big, small[:2] + (True,), dtype, hi)
            fails += f + _twin(state, twin, "misaligned small range vs aligned")
    assert not fails, fails[:8]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
def test_one_launch_step_above_the_resident_slots(dtype):
    """case G: 2080 workgroups, every tile on the 16-byte path, 34 MB per array; two steps, one hyper-parameter set per
    dtype (fp32: betas (0.5, 0.999), bf16: (0.9, 0.99)).  Every element is compared with the chain bit for bit; float64
    sees every fourth row n (3/4 of the rows are left out of the float64 comparison to keep its CPU time down)."""
    fails, _ = _run("G", A.SMALL_DEFAULT, dtype, TYPES.index(dtype))
    assert not fails, fails[:8]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
def test_one_launch_step_is_deterministic(dtype):
    fails, a = _run("C", (4977, 80, True), dtype, 0, fresh=True)
    f, b = _run("C", (4977, 80, True), dtype, 0, fresh=True)
    assert not fails + f + _twin(a, b, "second run"), (fails + f)[:8]


def _scenario(big, dtype, hi, first_step=1):
    return Step(A.BIG_CASES[big], A.SMALL_DEFAULT, dtype, HP[hi], seed=17 + hi, first_step=first_step)


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("big", ["A", "C"])
def test_first_launch_at_a_late_step(big, dtype):
    """a zeroed record and hyper's step at 7: every workgroup derives the terms of step 8 itself"""
    fails = []
    for hi in range(len(HP)):
        s = _scenario(big, dtype, hi, first_step=8)
        fails += s.launch() + s.launch()
        assert s.step == 9 and all(x <= 1.0 for x in s.worst.values()) or fails
    assert not fails, fails[:8]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("big", ["A", "C"])
def test_host_rewrite_of_lr_and_beta1(big, dtype):
    """after step 3 the host rewrites lr (x 100) and beta1 and zeroes the record: step 4 must use the new terms, not the
    step size cached for step 4 under the old ones (tests/test_adam_fused_ref.py shows the float64 bound tells them
    apart)"""
    fails = []
    for hi in range(len(HP)):
        s = _scenario(big, dtype, hi)
        for _ in range(3):
            fails += s.launch()
        s.rewrite(hp=A.rewritten(HP[hi]))
        for _ in range(3):
            fails += s.launch()
    assert not fails, fails[:8]


@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("big", ["A", "C"])
def test_host_rewrite_of_the_step_counter(big, dtype):
    """the step counter alone is rewritten, back by two and then forward by three, the record zeroed each time"""
    fails = []
    for hi in range(len(HP)):
        s = _scenario(big, dtype, hi)
        for _ in range(3):
            fails += s.launch()
        s.rewrite(step=s.step - 2)
        fails += s.launch() + s.launch()
        assert s.step == 3
        s.rewrite(step=s.step + 3)
        fails += s.launch() + s.launch()
        assert s.step == 8
    assert not fails, fails[:8]


def test_bad_arguments_are_refused_before_any_launch():
    s = _scenario("A", torch.float32, 0)
    before = s.state()
    g = torch.zeros(s.nb, device=DEV)
    outside = torch.zeros(A.W2_ELEMS, device=DEV)                    # a conv2.weight that is not inside the small range
    with pytest.raises(ops.GdmError):
        ops.simnn_adam_step(s.p.t, g, s.m.t, s.v.t, s.N, s.C, s.P, s.shadow.t, s.ps.t, s.gs.t, s.ms.t, s.vs.t, outside,
                            s.pack.t, s.hyper.t, s.rec.t)
    torch.cuda.synchronize()
    assert not _twin(s.state(), before, "after a refused call")


# ------------------------------------------------------------------------------------------ gdm_adam_step_dev_pc
@pytest.mark.parametrize("dtype", TYPES, ids=str)
@pytest.mark.parametrize("name", list(A.PC_CASES))
def test_adam_step_dev_pc(name, dtype):
    """three advance_step=True steps against float64 and, bit for bit, against gdm_adam_step_dev on the un-permuted
    gradient; then one advance_step=False call behind a gdm_adam_step_dev of another range, which must use the record
    as it is and leave `hyper` untouched (compared with gdm_adam_step at the same step).  Case H also ends bit-equal
    to case C."""
    fails, finals = [], {}
    for case in ([name, "C"] if name == "H" else [name]):
        for hi, hp in enumerate(HP):
            N, C, P, _ = big = A.PC_CASES[case]
            s = Step(big, None, dtype, hp, seed=sum(big[:3]) + hi, with_small=False)
            d = {k: getattr(s, k).t.clone() for k in "pmv"}
            d_hyper = s.c_hyper
            for step in range(1, 5):
                what = f"pc {case} {dtype} set {hi} step {step}"
                g_pc, _ = s.gradients(step)
                g_flat = g_pc.permute(0, 2, 1).contiguous().view(-1).to(DEV)
                before = s.state()
                if step < 4:
                    ops.adam_step_dev_pc(s.p.t, g_pc.to(DEV).view(-1), s.m.t, s.v.t, N, C, P, s.shadow.t, s.hyper.t,
                                         advance_step=True)
                    ops.adam_step_dev(d["p"], g_flat, d["m"], d["v"], d_hyper)
                else:
                    other = torch.zeros(4, 5, device=DEV)
                    ops.adam_step_dev(other[0], other[1], other[2], other[3], s.hyper.t)      # advances to step 4
                    held = s.hyper.t.cpu().clone()
                    ops.adam_step_dev_pc(s.p.t, g_pc.to(DEV).view(-1), s.m.t, s.v.t, N, C, P, s.shadow.t, s.hyper.t,
                                         advance_step=False)
                    ops.adam_step(d["p"], g_flat, d["m"], d["v"], 4, hp[0], hp[1], hp[2], hp[3], hp[4])
                    fails += R.check_bits(s.hyper.t, held, what=f"{what} hyper after advance_step=False")
                    d_hyper = held
                torch.cuda.synchronize()
                after = s.state()
                for b in s.guarded:
                    fails += b.check(what)
                ref = A.pc_step_ref(before["p"], g_pc, before["m"], before["v"], N, C, P, step, hp, dtype)
                f, w = A.check_pc(after, ref, what=what)
                fails += f
                s._worst("pc", w)
                for k in "pmv":
                    fails += R.check_bits(after[k], d[k], what=f"{what} {k} vs gdm_adam_step_dev")
                fails += R.check_bits(after["hyper"], d_hyper, what=f"{what} hyper vs gdm_adam_step_dev")
            record("adam_step_dev_pc", case=case, dtype=str(dtype), hyper=hi, **{k: round(x, 4) for k, x in s.worst.items()})
            assert all(x <= 1.0 for x in s.worst.values()) or fails, s.worst
            finals[case, hi] = after
    if name == "H":
        for hi in range(len(HP)):
            fails += _twin(finals["H", hi], finals["C", hi], "misaligned H vs aligned C")
    assert not fails, fails[:8]
