""""des_device" against "des_batch" on the same build.

  bridge      matrix_to_midis (64x64, window 100..150, no files) and matrix_to_wav (20x20) alone, B = 30 and B = 256
  midis       generate_midis(256), files written
  songs       generate_songs(30), --max-seconds of audio each

The two back ends are alternated --rounds times in one process after a warm-up; every call ends in a synchronise and is
timed on the host.  One JSON line per item with the median, the minimum and the maximum of each back end
(--out, default profiles/des_device_timing.jsonl).  --resources writes the draws kernel's resource report (VGPRs, SGPRs,
LDS, scratch) read from the compiler's remarks to profiles/des_draws_resources.txt (needs no GPU).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BACK_ENDS = ("des_batch", "des_device")


def resources(path):
    from gan_des_midi_music_gen_amd import build
    src = os.path.join(build.CSRC, "des_draws.hip")
    cmd = [build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [re.sub(r"\s*\[-Rpass[^\]]*\]$", "", ln.split("remark: ", 1)[1]) for ln in (r.stdout + r.stderr).splitlines()
             if "remark: " in ln and re.search(r"Function Name|VGPRs|AGPRs|SGPRs|ScratchSize|Occupancy|LDS Size", ln)]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"no resource remarks from {' '.join(cmd)}\n{r.stdout}{r.stderr}")
    with open(path, "w") as f:
        f.write("des_draws.hip, gfx950 (-Rpass-analysis=kernel-resource-usage)\n" + "\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--items", default="bridge,midis,songs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "des_device_timing.jsonl"))
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        return resources(os.path.join(ROOT, "profiles", "des_draws_resources.txt"))

    import numpy as np
    import torch
    from gan_des_midi_music_gen_amd import SIMNN
    from gan_des_midi_music_gen_amd import matrix_sim_process as msp
    from gan_des_midi_music_gen_amd import network_tests as NT
    dev = torch.device("cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def compare(item, fn, **info):
        """fn(back_end) alternated: one warm-up each, then --rounds timed calls each.  A call that raises what the
        reference raises for a sample (the whole-batch bridges do) is timed all the same and reported."""
        raised = {}

        def call(be):
            try:
                fn(be)
            except (ValueError, IndexError) as e:
                raised[be] = f"{type(e).__name__}: {str(e)[:60]}"

        for be in BACK_ENDS:
            call(be)
        ms = {be: [] for be in BACK_ENDS}
        for _ in range(a.rounds):
            for be in BACK_ENDS:
                np.random.seed(1)
                ms[be].append(wall(lambda: call(be)))
        line = dict(item=item, rounds=a.rounds, **info)
        for be in BACK_ENDS:
            line[be] = dict(median_ms=round(statistics.median(ms[be]), 2), min_ms=round(min(ms[be]), 2),
                            max_ms=round(max(ms[be]), 2))
        if raised:
            line["raised"] = raised
        line["speedup"] = round(line["des_batch"]["median_ms"] / line["des_device"]["median_ms"], 2)
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    def model2():
        torch.manual_seed(3)
        mm = NT.MultiModalGAN(z_dim=50, adj_size=(64, 64), roll_size=(2, 128, 50), input_dim=50, output_dim=20,
                              instrument=0, start=100, end=150, device=dev).to(dev)
        g = torch.Generator().manual_seed(4)
        for gen in (mm.generator1, mm.generator2):
            for blk in gen.gen:
                blk[1].running_mean.copy_(torch.randn(blk[1].num_features, generator=g) * 0.1)
                blk[1].running_var.copy_(torch.rand(blk[1].num_features, generator=g) + 0.5)
        return mm.eval()

    items = a.items.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        mm = model2()
        gen1 = SIMNN.Generator().apply(SIMNN.weights_init).to(dev)
        if "bridge" in items:
            for b in (30, 256):
                g = torch.Generator().manual_seed(b)
                n1, n2 = (torch.randn(b, 50, generator=g).to(dev) for _ in range(2))
                beats = torch.cumsum(torch.rand(b, 50, generator=g) * 0.5 + 0.3, dim=1).to(dev)
                o1, o2 = mm.sample(noise1=n1, noise2=n2, input_tensor=beats)
                compare("matrix_to_midis", lambda be: msp.matrix_to_midis(o1, o2, (64, 64), 0, 100, 150, simulate=be), B=b)
                torch.manual_seed(b)
                mats = SIMNN.sample_matrices(gen1, b).reshape(b, 20, 20)
                compare("matrix_to_wav", lambda be: msp.matrix_to_wav(mats, size=20, start=0, end=216, device=dev,
                                                                       simulate=be), B=b)
        if "midis" in items:
            g = torch.Generator().manual_seed(7)
            n1, n2 = (torch.randn(256, 50, generator=g).to(dev) for _ in range(2))
            beats = torch.cumsum(torch.rand(256, 50, generator=g) * 0.5 + 0.3, dim=1).to(dev)
            compare("generate_midis", lambda be: mm.generate_midis(noise1=n1, noise2=n2, input_tensor=beats,
                                                                    out_dir=os.path.join(tmp, be), bridge=be), n=256)
        if "songs" in items:
            torch.manual_seed(21)
            ck = os.path.join(tmp, "gen_5_0.pt")
            torch.save(SIMNN.Generator().apply(SIMNN.weights_init).state_dict(), ck)
            compare("generate_songs", lambda be: SIMNN.generate_songs(ck, 30, out_dir=os.path.join(tmp, "s_" + be),
                                                                      max_seconds=a.max_seconds, device=dev, bridge=be),
                    n=30, max_seconds=a.max_seconds)


if __name__ == "__main__":
    main()
