"""GPU: conv2's four entry points give the bits recorded in tests/golden/trunk_bits.npz (recorded before the kernels'
prologues and the weight gradient's epilogue were reordered; tests/golden/make_trunk_bits_golden.py), and the weight
gradient's workgroups still write their slabs in the layout the slab sum reads.

Shapes (B, H1, W1), see tests/trunk_bits.py -- the smallest that reach each path of the prologue / epilogue code:
  (1, 4, 4)       one workgroup, one real step; the forward's second prefetch clamps to the last tile
  (2, 5, 7)       odd H1 / W1, partial quad, scalar x-window loads in the fused kernel
  (3, 40, 140)    fewer items than the cap, row segments, three column tiles with a partial last one; forward grid (90)
                  not a multiple of 8, so no XCD remap
  (130, 40, 130)  more items than workgroups in the fused and weight plans: accumulators persist across items
  (33, 128, 64)   forward with more tiles (1056) than workgroups (768): remapped grid, one or two tiles per workgroup
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import trunk_bits as tb  # noqa: E402
from gan_des_midi_music_gen_amd import _lib, ops  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("shape", tb.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt_name", list(tb.DTYPES))
def test_conv2_entry_points_give_the_recorded_bits(golden, dt_name, shape):
    key = tb.case_key(dt_name, shape)
    outs = tb.run_entry_points(tb.make_inputs(shape, tb.DTYPES[dt_name]))
    torch.cuda.synchronize()
    moved = [m for m in (tb.mismatch(f"{key}/{n}", t, golden) for n, t in outs.items() if n.startswith("in_")) if m]
    assert not moved, f"the INPUTS moved (conv1's forward, not conv2): {moved}  [{golden['header']}]"
    bad = [m for m in (tb.mismatch(f"{key}/{n}", t, golden) for n, t in outs.items() if not n.startswith("in_")) if m]
    assert not bad, f"{bad}  [{golden['header']}]"


@pytest.mark.parametrize("dt_name", list(tb.DTYPES))
def test_weight_gradient_slab_layout(dt_name):
    """Slab k of the workspace = workgroup k's partial sums as [o 32][tap 9][ci 16], then 32 bias sums.  With at most 64
    workgroups the slab sum is one level (slab_groups in simnn_slab_sum.hip): wave w of 16 adds slabs w, w + 16, ... in
    ascending order starting from zero, then the 16 partials are added in wave order -- the same float32 sums on the host
    must reproduce dw2 / db2 exactly."""
    shape = (3, 40, 140)
    inp = tb.make_inputs(shape, tb.DTYPES[dt_name])
    _, code2 = ops.simnn_conv2_fwd(inp["p1"], inp["pack"], inp["b2"])
    dw2, db2 = ops.simnn_conv2_bwd_weight(inp["dp2"], code2, inp["p1"])
    nb = _lib.load().gdm_simnn_conv2_bwd_weight_workspace_bytes(*shape)
    nslabs = nb // (4640 * 4) - 65
    if nslabs > 64:
        pytest.skip("two-level slab sum: the one-level order does not apply")
    slabs = ops.workspace(nb, inp["p1"].device)[:nslabs * 4640 * 4].view(torch.float32).reshape(nslabs, 4640).cpu()
    parts = []
    for w in range(16):
        s = torch.zeros(4640)
        for k in range(w, nslabs, 16):
            s = s + slabs[k]
        parts.append(s)
    # ((s0 + s1) + (s2 + s3)) + ... of the kernel's eight partial sums: only s0 is non-zero here
    total = parts[0] + 0.0
    for w in range(1, 16):
        total = total + parts[w]
    want_dw = total[:4608].reshape(32, 9, 16).permute(0, 2, 1).reshape(32, 16, 3, 3)
    got_dw, got_db = dw2.cpu(), db2.cpu()
    bad = torch.nonzero((got_dw != want_dw).reshape(-1))
    assert bad.numel() == 0, f"dw2: first differing index {int(bad[0])}"
    bad = torch.nonzero(got_db != total[4608:])
    assert bad.numel() == 0, f"db2: first differing index {int(bad[0])}"
