"""Cases, runner and recorded-bits format shared by tests/golden/make_gemm_ring_golden.py and test_gemm_ring_gpu.py.

The bf16 x bf16 instances of gemm_bf16_fast fetch their operand tiles through a ring of register stages (RING tiles
ahead, csrc/gemm_bf16_kernel.h).  How far ahead a tile is fetched must not move a bit: every output element receives
the same MFMAs in the same order.  tests/golden/gemm_ring_bits.npz holds what the library gave BEFORE the ring existed
(one tile ahead with K tile 32, two with K tile 64), on the continuous inputs of tests/gemm_ref.py -- its exact family
is independent of the summation order and test_gemm_edges_gpu.py covers it.

The shapes are the smallest that reach every place of a ring of up to 4 stages (the library ships 2): per-workgroup
k-tile counts 1 .. 9 (fewer tiles than stages, as many, one more, two trips, two trips and one -- for 2 stages that
is 1, 2, 3, 4, 5), a partial last tile, uneven split-K slabs, a full and an edge row tile.  Of every output the SHA-256 over all its bytes is recorded, and 256 four-byte words at
positions drawn from the output's name for the failure message.
"""
import hashlib

import numpy as np
import torch

import gemm_ref as gr

SAMPLE_WORDS = 256
GOLDEN_FILE = "gemm_ring_bits.npz"


def _deep(k):
    """K tile 64, split_k 2 (fc1 forward's layouts): K-major A x K-major B"""
    return gr.Case(f"ring-k64-k{k}", 130, 132, k, "bf16", "k", "bf16", "k", gr.BF16, 2, expect="fast_k64")


def _k32(kind, k, tc):
    """K tile 32: dX's layouts (K-major A x row-major B) and dW's (row-major A x row-major B)"""
    la, m = ("k", 130) if kind == "dx" else ("r", 128)
    return gr.Case(f"ring-k32-{kind}-k{k}-{tc}", m, 136, k, "bf16", la, "bf16", "r", gr.BF16, 1, tc=tc,
                   expect="fast_k32")


K32_KS = [32 * t for t in (1, 2, 3, 4, 5, 8, 9)] + [32 * 5 - 24]
CASES = ([_deep(k) for k in [2 * 64 * t for t in (4, 5, 7, 8, 9)] + [2 * 64 * 4 + 8]] +
         [_k32("dx", k, tc) for k in K32_KS for tc in ("bf16", "f32")] +
         [_k32("dw", k, "f32") for k in K32_KS])


def run(c, device="cuda"):
    """One call of case c on its continuous inputs, C inside a sentinel-filled buffer -> (out on the CPU, failures).
    The plan is asserted first: a case that does not run the kernel it names fails for that reason."""
    from gan_des_midi_music_gen_amd import ops
    plan = gr.plan_of(c)
    t = gr.materialize(c, gr.inputs(c, "continuous"), device)
    kw = dict(act=c.act, slope=c.slope, compute=c.comp, split_k=c.split, out=t["out"])
    live = ops.gemm_plan(t["a"], t["b"], **kw)
    assert live == plan, f"{c.name}: the device tensors' plan {live} is not the description's {plan}"
    assert plan["kernel"] == c.expect, f"{c.name}: runs {plan['kernel']}, meant for {c.expect}: {plan}"
    assert plan["split_k"] == c.split, f"{c.name}: split {plan['split_k']}, meant {c.split}"
    fails = []
    ops.gemm(t["a"], t["b"], **kw)
    out = t["out"].contiguous().cpu()
    if plan["split_k"] > 1:
        first = t["cbuf"].clone()
        ops.gemm(t["a"], t["b"], **kw)
        if not torch.equal(first, t["cbuf"]):
            fails.append(f"{c.name}: two runs of the split-K call differ")
    if not gr.untouched(t):
        bad = ((t["cbuf"] != gr.SENTINEL) & t["outside"]).nonzero().flatten()[:4].tolist()
        fails.append(f"{c.name}: wrote outside C, buffer elements {bad}")
    return out, fails


def _words(t):
    raw = t.contiguous().reshape(-1).view(torch.uint8).numpy()
    return raw, raw[:raw.size // 4 * 4].view(np.uint32)


def _positions(name, n_words):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    return np.sort(np.random.default_rng(seed).choice(n_words, SAMPLE_WORDS, replace=False))


def record(name, t):
    """What the golden file keeps of output ``name``: {key: array}."""
    raw, words = _words(t)
    return {f"{name}.sha256": np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), np.uint8),
            f"{name}.sample": words[_positions(name, words.size)]}


def mismatch(name, t, golden):
    """None when ``t`` has the recorded bits, else a message with the first differing sampled word."""
    raw, words = _words(t)
    if hashlib.sha256(raw.tobytes()).digest() == golden[f"{name}.sha256"].tobytes():
        return None
    idx = _positions(name, words.size)
    bad = np.flatnonzero(words[idx] != golden[f"{name}.sample"])
    where = f"first differing sampled 4-byte word {idx[bad[0]]}" if bad.size else "none of the sampled words differs"
    return f"{name}: SHA-256 differs from the recorded one; {where}"
