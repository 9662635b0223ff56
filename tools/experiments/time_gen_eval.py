"""Time model 1's eval-mode generator forward gen(noise) in bf16 at B = 1, 16, 256, and the training-mode fused chain at
B = 256, with HIP events around back-to-back calls after a warm-up.

    python tools/experiments/time_gen_eval.py                      one measurement of the tree this file is in
    python tools/experiments/time_gen_eval.py --compare OTHER_ROOT --rounds 3 --out FILE.json
        alternates fresh child processes on OTHER_ROOT (a checkout of another commit with its library built) and on
        this tree, `rounds` times each, and writes every measurement plus the per-batch minima, maxima and the verdict
        "faster by more than the spread between alternations".
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BATCHES = (1, 16, 256)


def measure(root, calls, warmup):
    sys.path.insert(0, root)
    import torch
    from gan_des_midi_music_gen_amd import SIMNN, functional as Fn

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / calls          # us per call

    torch.manual_seed(0)
    gen = SIMNN.Generator().to("cuda").eval()
    gen.compute_dtype = "bf16"
    res = {"root": root, "eval_route": "one launch" if hasattr(Fn, "simnn_gen_forward_eval") else "layer-wise"}
    with torch.no_grad():
        for B in BATCHES:
            noise = SIMNN.get_noise(B, 100, device="cuda")
            res[f"eval_bf16_B{B}_us"] = round(timed(lambda: gen(noise)), 2)
        # the training-mode fused chain (six launches), as the trainers call it
        gen.train()
        ws = [m.weight.detach() for m in (gen.conv1, gen.conv2, gen.conv3, gen.conv4)]
        bns = [(m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var, m.num_batches_tracked)
               for m in (gen.batch_norm1, gen.batch_norm2, gen.batch_norm3)]
        noise, cache = SIMNN.get_noise(256, 100, device="cuda"), {}
        res["train_fused_B256_us"] = round(timed(lambda: Fn.simnn_gen_forward(noise, ws, bns, True, Fn.BF16, cache=cache,
                                                                              need_backward=False)), 2)
        if hasattr(Fn, "simnn_gen_forward_eval"):        # the kernel alone (pack cached), without the module's autograd shell
            for B in BATCHES:
                noise = SIMNN.get_noise(B, 100, device="cuda")
                res[f"eval_kernel_B{B}_us"] = round(timed(lambda: Fn.simnn_gen_forward(noise, ws, bns, False, Fn.BF16,
                                                                                       cache=cache)), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare is None:
        print(json.dumps(measure(args.root, args.calls, args.warmup)))
        return
    runs = {"other": [], "this": []}
    for _ in range(args.rounds):
        for name, root in (("other", os.path.abspath(args.compare)), ("this", ROOT)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--calls", str(args.calls),
                                "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"measurement of {root} failed (exit {r.returncode}): nothing more is started")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    summary = {}
    for B in BATCHES:
        k = f"eval_bf16_B{B}_us"
        o, t = [r[k] for r in runs["other"]], [r[k] for r in runs["this"]]
        spread = max(max(o) - min(o), max(t) - min(t))
        summary[k] = {"other": o, "this": t, "spread_us": round(spread, 2),
                      "faster_by_more_than_spread": min(o) - max(t) > spread}
    out = {"calls": args.calls, "warmup": args.warmup, "runs": runs, "summary": summary}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
