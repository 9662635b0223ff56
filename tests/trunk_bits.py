"""Inputs and recorded-bits format shared by tests/golden/make_trunk_bits_golden.py and test_trunk_fixed_cost_gpu.py.

The conv2 kernels' outputs are pinned BIT FOR BIT against tests/golden/trunk_bits.npz: changes to the part of a launch
that does not scale with work (prologue order, the weight gradient's cross-wave reduction) must not move a bit.

Inputs come from fixed CPU seeds and are realistic: x is a clamped dB-like spectrogram, p1 / code1 are what conv1's
forward kernel makes of it (ReLU-ed, rounded through bf16 in both modes), code2 is what conv2's forward kernel makes of
that p1, dp2 ~ 0.1 * randn.  The digests of p1 / code1 are recorded as well, so that a later change of conv1's forward
shows up as "inputs moved" and not as a conv2 failure.
"""
import hashlib

import numpy as np
import torch

from gan_des_midi_music_gen_amd import ops
from gan_des_midi_music_gen_amd.ops import BF16, F32

# (B, H1, W1): the geometry of p1; the spectrogram behind it is (B, 2 H1, 2 W1)
SHAPES = [(1, 4, 4), (2, 5, 7), (3, 40, 140), (130, 40, 130), (33, 128, 64)]
DTYPES = {"bf16": BF16, "fp32": F32}
WHOLE_BYTES = 64 * 1024          # outputs up to this size are recorded whole
SAMPLE_WORDS = 1024              # larger ones: SHA-256 + this many 4-byte words at fixed-seed positions (4 KB)


def case_key(dt_name, shape):
    return f"{dt_name}_{shape[0]}x{shape[1]}x{shape[2]}"


def make_inputs(shape, dt, device="cuda"):
    b, h1, w1 = shape
    g = torch.Generator().manual_seed(7919 * b + 131 * h1 + w1)
    x = (torch.randn(b, 2 * h1, 2 * w1, generator=g) * 18 - 35).clamp(-80, 30)
    cw1 = torch.randn(16, 1, 2, 2, generator=g) * 0.1
    cb1 = torch.randn(16, generator=g) * 0.5 + 2.0
    cw2 = torch.randn(32, 16, 3, 3, generator=g) * 0.05
    cb2 = torch.randn(32, generator=g) * 0.1
    dp2 = (torch.randn(b, h1 // 2, w1 // 2, 32, generator=g) * 0.1).to(ops.torch_dtype(dt))
    x = x.to(device)
    p1, code1 = ops.simnn_conv1_fwd(x, cw1.to(device), cb1.to(device), dt)
    if dt == F32:
        p1 = p1.to(torch.bfloat16).float()
    pack = ops.simnn_conv2_pack(cw2.to(device), dt)
    return {"x": x, "p1": p1.contiguous(), "code1": code1, "pack": pack, "b2": cb2.to(device), "dp2": dp2.to(device)}


def run_entry_points(inp):
    """The four entry points (the fused one in both its forms) -> {name: tensor}, inputs' digests first."""
    p1, pack = inp["p1"], inp["pack"]
    h1, w1 = p1.shape[1], p1.shape[2]
    out = {"in_p1": p1, "in_code1": inp["code1"]}
    out["fwd_p2"], out["fwd_code2"] = ops.simnn_conv2_fwd(p1, pack, inp["b2"])
    code2 = out["fwd_code2"]
    out["bwd_data_dp1"] = ops.simnn_conv2_bwd_data(inp["dp2"], code2, pack, h1, w1)
    out["fused_dw1"], out["fused_db1"], out["fused_dp1"] = ops.simnn_conv2_bwd_fused(
        inp["dp2"], code2, pack, inp["code1"], inp["x"], want_dp1=True)
    out["fused_nodp1_dw1"], out["fused_nodp1_db1"], _ = ops.simnn_conv2_bwd_fused(
        inp["dp2"], code2, pack, inp["code1"], inp["x"])
    out["bwd_weight_dw2"], out["bwd_weight_db2"] = ops.simnn_conv2_bwd_weight(inp["dp2"], code2, p1)
    return out


def raw_bytes(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy()


def sample_positions(name, n_words):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    return np.sort(np.random.default_rng(seed).choice(n_words, SAMPLE_WORDS, replace=False)).astype(np.int64)


def record(name, t):
    """What the golden file keeps of output ``name``: {suffix: array}."""
    raw = raw_bytes(t)
    if raw.size <= WHOLE_BYTES:
        return {"whole": raw}
    words = raw.view(np.uint32)
    idx = sample_positions(name, words.size)
    return {"sha256": np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), np.uint8), "idx": idx, "sample": words[idx]}


def mismatch(name, t, golden):
    """None when ``t`` has the recorded bits, else a message naming the array and the first differing index."""
    raw = raw_bytes(t)
    if f"{name}.whole" in golden:
        want = golden[f"{name}.whole"]
        if raw.size != want.size:
            return f"{name}: {raw.size} bytes, recorded {want.size}"
        item = t.element_size()
        bad = np.flatnonzero(raw != want)
        return None if bad.size == 0 else f"{name}: first differing element {bad[0] // item} (byte {bad[0]})"
    if hashlib.sha256(raw.tobytes()).digest() == golden[f"{name}.sha256"].tobytes():
        return None
    words, idx = raw.view(np.uint32), golden[f"{name}.idx"]
    if idx.max() >= words.size:
        return f"{name}: {raw.size} bytes, shorter than the recorded sample reaches"
    bad = np.flatnonzero(words[idx] != golden[f"{name}.sample"])
    where = f"first differing sampled 4-byte word {idx[bad[0]]}" if bad.size else "none of the sampled words differs"
    return f"{name}: SHA-256 differs from the recorded one; {where}"
