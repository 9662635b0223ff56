"""CPU: the guard-band harness of tests/guarded.py fails when it should, and every device entry point of the library
has a guarded test.

Fake "wrappers" written with torch on the CPU, shaped like those of gan_des_midi_music_gen_amd.ops (they allocate with
``NS.torch.empty``, take scratch from ``NS.workspace`` and hand pointers to ``NS._p`` / ``NS._call``), each with one
fault: a store past the output, a read past the input, an output element left unwritten, a read of workspace bytes
that were not written first.  Each is reported under its tensor's name with its cause; a correct fake passes.

The completeness pin: every name of _lib.SIGNATURES whose declaration in include/gdm.h takes a ``stream`` is either in
COVERED of tests/test_buffer_bounds_gpu.py (run through guarded.run_case there) or in GUARDED_ELSEWHERE, which names the
existing test file AND the function in it that launches the entry on caller-owned buffers between guard values and
asserts them: that one function's source must hold both the call and the guard assertion.  A new entry point cannot
land without one or the other.  The trunk cases' plan regimes are asserted here too (CPU arithmetic).
"""
import ast
import os
import re
import types

import pytest
import torch

import guarded as G

from gan_des_midi_music_gen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the fake module
class _SlackTorch:
    """torch whose ``empty`` hands out zeroed views of larger blocks, as a caching allocator's rounded blocks are: a
    fake may step one element past its tensor in the plain runs too"""

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def empty(shape, dtype=torch.float32, device=None):
        return G._plain(torch.zeros(shape, dtype=dtype), device or "cpu")


def _namespace():
    ns = types.SimpleNamespace(torch=_SlackTorch(), calls=[])
    ns.workspace = lambda nbytes, device: torch.zeros(max(int(nbytes), 1 << 12), dtype=torch.uint8, device=device)
    ns._p = lambda t: None if t is None else t.data_ptr()
    ns._call = lambda name, *args: ns.calls.append(name)
    return ns


NS = _namespace()


def _past(t, k=1):
    """the flat view of t with k more elements behind it"""
    return torch.as_strided(t, (t.numel() + k,), (1,))


def _prologue(x, name):
    out = NS.torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ws = NS.workspace(4 * x.numel(), x.device)
    for t in (x, out, ws):
        NS._p(t)
    NS._call(name)
    return out, ws[:4 * x.numel()].view(torch.float32)


def fake_ok(x):
    out, ws = _prologue(x, "fake_ok")
    ws.copy_(x.reshape(-1) * 2)
    out.copy_((ws + 1).view(x.shape))
    return out


def fake_stores_past_output(x):
    out, ws = _prologue(x, "fake_stores_past_output")
    ws.zero_()
    out.copy_(x)
    _past(out)[-1] = 1.0
    return out


def fake_reads_past_input(x):
    out, ws = _prologue(x, "fake_reads_past_input")
    ws.zero_()
    out.copy_(x)
    out.view(-1)[0] += _past(x)[-1]
    return out


def fake_leaves_one_unwritten(x):
    out, ws = _prologue(x, "fake_leaves_one_unwritten")
    ws.zero_()
    out.view(-1)[:-1] = x.reshape(-1)[:-1]
    return out


def fake_reads_stale_workspace(x):
    out, ws = _prologue(x, "fake_reads_stale_workspace")
    out.copy_(x + ws[0])
    return out


def fake_reads_stale_output(x):
    out, ws = _prologue(x, "fake_reads_stale_output")
    ws.zero_()
    out.view(-1)[1:] = x.reshape(-1)[1:]
    out.view(-1)[0] = out.view(-1)[0] * 0.5 + x.reshape(-1)[0]
    return out


_ticks = [0]


def fake_nondeterministic(x):
    out, ws = _prologue(x, "fake_nondeterministic")
    ws.zero_()
    _ticks[0] += 1
    out.copy_(x + _ticks[0])
    return out


def fake_allocates_on_the_side(x):
    out, ws = _prologue(x, "fake_allocates_on_the_side")
    ws.zero_()
    side = torch.zeros(3)                    # not through NS.torch: no arena, no guards
    NS._p(side)
    out.copy_(x)
    return out


def fake_writes_its_input(x):
    out, ws = _prologue(x, "fake_writes_its_input")
    ws.zero_()
    out.copy_(x)
    x.view(-1)[2] = 0.0
    return out


def _x(shape=(5, 7)):
    return torch.randn(shape, generator=torch.Generator().manual_seed(3)) + 3.0


def _run(fake, x=None, inout=()):
    return G.run_case(lambda t: fake(t["x"]), {"x": _x() if x is None else x}, inout, mod=NS, device="cpu")


def test_a_correct_fake_passes_and_its_entry_is_recorded():
    NS.calls.clear()
    R, log = _run(fake_ok)
    assert torch.equal(R["out"].view(torch.float32), (_x() * 2 + 1).reshape(-1))
    assert log.names == ["fake_ok"] and "fake_ok" in G.CALLED
    assert NS.calls == ["fake_ok"] * 4                                   # two plain runs, two guarded ones
    assert NS.torch.__class__ is _SlackTorch and NS._p(None) is None   # the patches are gone


def test_a_store_past_the_output_is_caught():
    with pytest.raises(G.GuardError) as e:
        _run(fake_stores_past_output)
    assert e.value.kind == "wrote-outside" and e.value.tensor == "_prologue:out", str(e.value)
    v = e.value.detail["violations"]
    assert v == [dict(tensor="_prologue:out", side="behind", distance=0, bytes=4)] or \
        v == [dict(tensor="_prologue:out", side="behind", distance=0, bytes=3)]      # 1.0f = 00 00 80 3F over 0x7F..


def test_a_read_past_the_input_is_caught():
    with pytest.raises(G.GuardError) as e:
        _run(fake_reads_past_input)
    assert e.value.kind == "reads-outside-input" and e.value.tensor == "x", str(e.value)
    assert e.value.detail["output"] == "out" and e.value.detail["first"] < 4


def test_an_unwritten_output_element_is_caught():
    with pytest.raises(G.GuardError) as e:
        _run(fake_leaves_one_unwritten)
    assert e.value.kind == "unwritten" and e.value.tensor == "out", str(e.value)
    assert e.value.detail["first"] == 4 * (5 * 7 - 1)


def test_a_read_of_unwritten_workspace_is_caught():
    with pytest.raises(G.GuardError) as e:
        _run(fake_reads_stale_workspace)
    assert e.value.kind == "reads-stale-workspace" and e.value.tensor == "workspace", str(e.value)


def test_a_read_of_earlier_output_content_is_caught():
    with pytest.raises(G.GuardError) as e:
        _run(fake_reads_stale_output)
    assert e.value.kind == "reads-stale-output" and e.value.tensor == "_prologue:out", str(e.value)


def test_nondeterminism_an_unguarded_buffer_and_a_written_input_are_told_apart():
    with pytest.raises(G.GuardError) as e:
        _run(fake_nondeterministic)
    assert e.value.kind == "nondeterministic" and e.value.tensor == "out"
    with pytest.raises(G.GuardError) as e:
        _run(fake_allocates_on_the_side)
    assert e.value.kind == "escaped" and "fake_allocates_on_the_side" in e.value.tensor, str(e.value)
    with pytest.raises(G.GuardError) as e:
        _run(fake_writes_its_input)
    assert e.value.kind == "input-modified" and e.value.tensor == "x" and e.value.detail["first"] == 8
    R, _ = _run(fake_writes_its_input, inout=("x",))                     # declared in-out: compared, not refused
    want = _x().reshape(-1)
    want[2] = 0.0
    assert torch.equal(R["x"].view(torch.float32), want)


def test_exempt_bytes_are_a_closed_list():
    for (entry, tensor), ((a, b), source) in G.EXEMPT.items():
        assert entry in _lib.SIGNATURES and isinstance(tensor, str)
        assert source.startswith("include/gdm.h") or source.startswith("gan_des_midi_music_gen_amd/csrc/"), source
        keep = G._keep(entry, tensor, torch.zeros(64, dtype=torch.uint8))
        assert int((~keep).sum()) == len(range(64)[slice(a, b)]) > 0
    assert bool(G._keep("gdm_cast", "out", torch.zeros(8, dtype=torch.uint8)).all())


def test_arena_layout():
    a = G.Arena("cpu", 0xFF, 1 << 20)
    x = a.take((3, 5), torch.float32, "x", init=torch.ones(3, 5))
    y = a.take((2, 4096), torch.bfloat16, "y")
    z = a.take(0, torch.uint8, "ws", role="ws")
    y2 = a.take((7,), torch.int64, "y")
    assert [s["name"] for s in a.slots] == ["x", "y", "ws", "y#2"]
    for t in (x, y, y2):
        assert t.data_ptr() % G.ALIGN == 0 and t.is_contiguous()
    assert z.numel() == 0
    sx, sy = a.slots[0], a.slots[1]
    assert sx["lo"] - sx["g0"] >= 4096 and sx["g1"] - sx["hi"] == 4096          # small tensors: 4 KiB either side
    assert sy["g1"] - sy["hi"] == 8192 and sy["lo"] - sy["g0"] >= 8192          # one outermost slice of y
    assert bool(torch.isnan(y.float()).all()) and int(y2[0]) == -1              # 0xFF: NaN, -1
    b = G.Arena("cpu", 0x7F, 1 << 16).take((4,), torch.float32, "b")
    assert float(b[0]) > 3.39e38 and bool(torch.isfinite(b).all())
    assert float(G.Arena("cpu", 0x7F, 1 << 16).take((4,), torch.bfloat16, "b")[0]) > 3.38e38
    assert a.owner(y.data_ptr()) == "y" and a.owner(y[1].data_ptr()) == "y" and a.owner(a.base) is None
    assert a.violations() == []
    a.buf[sx["lo"] - 3] = 0
    a.buf[sy["hi"] + 10:sy["hi"] + 12] = 1
    assert a.violations() == [dict(tensor="x", side="before", distance=2, bytes=1),
                              dict(tensor="y", side="behind", distance=10, bytes=2)]
    with pytest.raises(RuntimeError, match="the arena holds"):
        a.take((1 << 20,), torch.uint8, "big")


# ------------------------------------------------------------------------------------------------ completeness pin
# entry -> (test file, the function in it that launches the entry between guards, the call as that function writes it,
# the guard assertion as that function writes it, what is guarded).  Read from the files, function by function; where a
# file only guards the workspace (the DES simulators, whose outputs the host mirror pins element for element) the last
# field says so.
GUARDED_ELSEWHERE = {
    "gdm_adam_step_dev_pc": ("test_simnn_adam_step_gpu.py", "test_adam_step_dev_pc", "ops.adam_step_dev_pc(", "b.check(what)",
                             "p, m, v, operand copy, hyper"),
    "gdm_simnn_adam_step": ("test_simnn_adam_step_gpu.py", "launch", "ops.simnn_adam_step(", "b.check(what)",
                            "every buffer the kernel writes"),
    "gdm_mmgan_gen_eval": ("test_mmgan_gen_eval_gpu.py", "_launch", "ops.mmgan_gen_eval(", "== SENTINEL).all()",
                           "outputs and taps"),
    "gdm_stft_frames": ("test_mel_stages_gpu.py", "test_stft_frames_refusals_leave_the_output_untouched",
                        "lib.gdm_stft_frames(*ok", "== mr.SENTINEL).all()", "the output, behind"),
    "gdm_power_spectrum": ("test_mel_stages_gpu.py", "_run_power", "gdm_power_spectrum(", "== mr.SENTINEL).all()",
                           "the output"),
    "gdm_pcm_to_float": ("test_input_song_gpu.py", "test_pcm_to_float_bits", "ops.pcm_to_float(", "_guards_intact(buf)",
                         "the output"),
    "gdm_pcm_stft_frames": ("test_input_song_gpu.py", "_frames_case", "ops.pcm_stft_frames(", "_guards_intact(buf)",
                            "the output"),
    "gdm_des_draws": ("test_des_draws_gpu.py", "test_kernel_equals_host_mirror_bit_for_bit", "ops.des_draws(",
                      "== CANARY).all()", "every output"),
    "gdm_des_run_batch": ("test_des_batch_gpu.py", "device_run", "gdm_des_run_batch(", "== CANARY).all()",
                          "every output and the workspace"),
    "gdm_des_stats_batch": ("test_des_stats_gpu.py", "device_stats", "sv.run_stats_device(", "== GUARD).all()",
                            "the workspace"),
    "gdm_des_stats_batch_dist": ("test_des_dist_gpu.py", "device_stats", "sv.run_stats_device(", "== GUARD).all()",
                                 "the workspace"),
    "gdm_des_run_batch_dist": ("test_des_log_dist_gpu.py", "device_log", "sv.run_batch_device(", "== GUARD).all()",
                               "the workspace"),
    "gdm_des_stats_batch_net": ("test_des_net_gpu.py", "device_stats", "sv.run_stats_device(", "== GUARD).all()",
                                "the workspace"),
    "gdm_des_run_batch_net": ("test_des_net_gpu.py", "device_log", "sv.run_batch_device(", "== GUARD).all()",
                              "the workspace"),
    "gdm_piano_roll_windows": ("test_maestro_windows_gpu.py", "test_kernel_writes_its_windows_and_nothing_else",
                               "ops.piano_roll_windows(", "== sentinel).all()", "both outputs"),
    "gdm_synth_frames": ("test_des_bridge_gpu.py", "test_stage_b_equals_mirror", "ops.synth_frames(",
                         "guards_intact(buf, canary)", "the output"),
    "gdm_synth_pcm": ("test_des_bridge_gpu.py", "test_stage_c_equals_mirror_and_stage_b_through_the_pcm_front_end",
                      "ops.synth_pcm(", "guards_intact(buf, canary)", "the output"),
    "gdm_synth_windows": ("test_synth_windows_gpu.py", "test_windows_equal_the_mirror", "ops.synth_windows(",
                          "_guards_intact(buf)", "the output"),
    "gdm_synth_windows_gm": ("test_sim_to_wav_gpu.py", "_gm", "ops.synth_windows_gm(", "== 0x5A5A).all()", "the output"),
    "gdm_s2w_prologue": ("test_sim_to_wav_gpu.py", "test_s2w_prologue_equals_the_mirror", "ops.s2w_prologue(",
                         "== fill[dt]).all()", "every output"),
}
# the calls above that are not the entry or its ops wrapper: the package function behind them and the wrappers it picks
VIA = {"sv.run_stats_device(": ("simulation_v3.py", "run_stats_device",
                                {"gdm_des_stats_batch": "ops.des_run_stats(", "gdm_des_stats_batch_dist": "ops.des_run_stats_dist",
                                 "gdm_des_stats_batch_net": "ops.des_run_stats_net"}),
       "sv.run_batch_device(": ("simulation_v3.py", "run_batch_device",
                                {"gdm_des_run_batch_dist": "ops.des_run_batch_dist", "gdm_des_run_batch_net": "ops.des_run_batch_net"})}
NOT_DEVICE = re.compile(r"_host$|_bytes$|_chunks$|_supported$|_plan$|_max_rows$|^gdm_(last_error|version|arch|build_flavor)$")


def device_entries():
    """the names of _lib.SIGNATURES whose declaration in include/gdm.h has a ``stream`` parameter"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gdm.h")).read(), flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    out = []
    for name in _lib.SIGNATURES:
        m = re.search(r"\b%s\s*\(([^;{]*)\)\s*;" % re.escape(name), hdr)
        assert m, f"{name} is not declared in include/gdm.h"
        if re.search(r"\bstream\b", m.group(1)):
            out.append(name)
    return out


def ops_wrappers():
    """entry name -> the functions of ops.py whose source names it"""
    src = open(os.path.join(ROOT, "gan_des_midi_music_gen_amd", "ops.py")).read()
    out = {}
    for name, seg in functions_of(src).items():
        for n in re.findall(r'"(gdm_\w+)"', seg):
            out.setdefault(n, set()).add(name)
    return out


def functions_of(src):
    """name -> source of every function and method of a module (a later definition of the same name wins)"""
    return {f.name: ast.get_source_segment(src, f) for f in ast.walk(ast.parse(src)) if isinstance(f, ast.FunctionDef)}


def test_every_device_entry_point_has_a_guarded_test():
    import test_buffer_bounds_gpu as B
    dev = device_entries()
    assert len(dev) >= 70 and "gdm_gemm" in dev and "gdm_simnn_conv2_bwd_fused_finish" in dev
    left_out = [n for n in _lib.SIGNATURES if n not in dev]
    assert all(NOT_DEVICE.search(n) or n == "gdm_des_run" for n in left_out), \
        [n for n in left_out if not NOT_DEVICE.search(n)]
    covered, elsewhere = set(B.COVERED), set(GUARDED_ELSEWHERE)
    assert not covered & elsewhere, covered & elsewhere
    assert covered | elsewhere == set(dev), dict(missing=sorted(set(dev) - covered - elsewhere),
                                                 unknown=sorted((covered | elsewhere) - set(dev)))
    wrappers = ops_wrappers()
    for name, (fname, func, call, guard, _what) in GUARDED_ELSEWHERE.items():
        funcs = functions_of(open(os.path.join(ROOT, "tests", fname)).read())
        assert func in funcs, f"{fname} has no function {func}"
        body = funcs[func]
        assert call in body, f"{fname}:{func} does not call {call}"
        assert guard in body and re.search(r"assert|fails", body), f"{fname}:{func} asserts no guard ({guard})"
        if call in VIA:
            pkg_file, pkg_func, picks = VIA[call]
            seg = functions_of(open(os.path.join(ROOT, "gan_des_midi_music_gen_amd", pkg_file)).read())[pkg_func]
            assert picks[name] in seg, f"{pkg_file}:{pkg_func} does not reach {picks[name]}"
            wrapper = picks[name].split(".")[1].rstrip("(")
            reached = functions_of(open(os.path.join(ROOT, "gan_des_midi_music_gen_amd", "ops.py")).read())[wrapper]
            assert name in reached or any(w in reached for w in wrappers[name]), (name, wrapper)
        else:
            assert name in call or any(f".{w}(" in call for w in wrappers[name]), f"{call} is not a call of {name}"


def test_trunk_cases_reach_the_plan_regimes():
    """tests/test_trunk_plans.py's mirrors say which plan each row reaches; these regimes must be among the trunk cases
    of tests/test_buffer_bounds_gpu.py."""
    import test_buffer_bounds_gpu as B
    import trunk_ref as TR
    P = {}
    for kind, s in B.TRUNK:
        b, h, w, h1, w1 = B._geom(kind, s)
        P[(b, h, w)] = dict(fused=TR.bd_plan(b, h1, w1, True), bw=TR.bw_plan(b, h1, w1), h1=h1, w1=w1)
    f = [p["fused"] for p in P.values()]
    assert any(q["n_items"] == q["blocks"] for q in f), "one item per workgroup"
    assert any(q["n_items"] >= 2 * q["blocks"] and q["n_items"] % q["blocks"] for q in f), ">= 2 items, uneven tail"
    assert any(q["nseg"] > 1 and q["n_items"] > q["blocks"] for q in f), "row segments with wrap"
    assert any(p["w1"] % TR.BD_COLS and p["w1"] > TR.BD_COLS for p in P.values()), "a partial last column tile"
    assert any(p["h1"] % 2 and p["w1"] % 2 for p in P.values()), "odd H1 and W1"
    assert any(p["w1"] % 4 for p in P.values()), "code1 rows padded to a whole quad"
    ids = {c[0].split("-")[0] for c in B.CASES}
    assert {"conv1_fwd", "conv1_fwd_pair", "conv2_bwd_fused", "conv1_bwd_weight"} <= ids
