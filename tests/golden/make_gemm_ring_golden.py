#!/usr/bin/env python
"""Record tests/golden/gemm_ring_bits.npz: the bits gdm_gemm produces on an MI355X for the cases of tests/gemm_ring.py
(bf16 x bf16 operands through both variants of gemm_bf16_fast, continuous inputs).

    python tests/golden/make_gemm_ring_golden.py [commit hash to note in the file] [output directory]

Run it at the commit whose bits are the yardstick (the library must be built) and commit the file: it was recorded
with the library of the commit before the register ring, whose kernels fetched one (K tile 32) or two (K tile 64)
tiles ahead.  ``header`` names the commit (the argument, else ``git rev-parse HEAD``) and the device.
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import gemm_ring as ring  # noqa: E402


def main():
    if len(sys.argv) > 1:
        commit = sys.argv[1]
    else:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    store = {}
    for c in ring.CASES:
        out, fails = ring.run(c)
        assert not fails, fails
        store.update(ring.record(c.name, out))
        print(c.name, tuple(out.shape), out.dtype, flush=True)
    store["header"] = np.array(f"gemm ring bits recorded at commit {commit or 'unknown'} on "
                               f"{torch.cuda.get_device_name(0)}")
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    path = os.path.join(out_dir, ring.GOLDEN_FILE)
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
