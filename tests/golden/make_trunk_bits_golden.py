#!/usr/bin/env python
"""Record tests/golden/trunk_bits.npz: the bits conv2's four entry points (gdm_simnn_conv2_fwd, _bwd_data, _bwd_fused +
_finish, _bwd_weight) produce on an MI355X for the inputs of tests/trunk_bits.py, in bf16 and exact-fp32 mode.

    python tests/golden/make_trunk_bits_golden.py [commit hash to note in the file]

Run it at the commit whose bits are the yardstick (the library must be built) and commit the file.  Outputs of up to
64 KB are kept whole; of larger ones the SHA-256 and 1024 four-byte words at fixed-seed positions, with the positions.
``header`` names the commit (the argument, else ``git rev-parse HEAD``) and the device.
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import trunk_bits as tb  # noqa: E402


def main():
    if len(sys.argv) > 1:
        commit = sys.argv[1]
    else:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    store = {}
    for dt_name, dt in tb.DTYPES.items():
        for shape in tb.SHAPES:
            key = tb.case_key(dt_name, shape)
            outs = tb.run_entry_points(tb.make_inputs(shape, dt))
            torch.cuda.synchronize()
            for name, t in outs.items():
                for suffix, arr in tb.record(f"{key}/{name}", t).items():
                    store[f"{key}/{name}.{suffix}"] = arr
            print(key, {n: tuple(t.shape) for n, t in outs.items()}, flush=True)
    store["header"] = np.array(f"conv2 trunk bits recorded at commit {commit or 'unknown'} on "
                               f"{torch.cuda.get_device_name(0)}")
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    path = os.path.join(out_dir, "trunk_bits.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
