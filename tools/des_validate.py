"""Simulated M/M/1/K and M/M/c/N beside queueing theory (simulation_v3.mm1k_sweep / mmck_sweep, queueing_theory.mm1k /
mmck): the counterpart of the validation harness the reference's simulator ends in.

    python tools/des_validate.py [--device cuda] [--seeds 64] [--customers 4000] [--warmup N] [--waits]

For every configuration of the default grid (rho 0.5 .. 1.5, 1 .. 5 waiting places) the source -> server net is run once
per seed -- all configurations and seeds in ONE batch: the host mirror without --device, one kernel launch with it -- and
each compared quantity is printed as mean +- standard error over the seeds, the closed form, and z = (mean - theory) /
sem.  Then the same table for the multi-server grid: source -> queue node -> c servers (simulation_v3.mmck_spec), one
batch per c, beside M/M/c/N with N = c + max(cap, 1).  With --warmup N both tables are printed twice: for the whole runs,
which start from an empty system, and for the window between N and --customers customers of the same runs
(simulation_v3.window; with --device the warm-up run and the whole run of a seed are two waves of the one launch).  With
--waits a third table follows: the waiting-time LAW of the single-server grid, the fraction of accepted customers that
waited longer than t beside queueing_theory.mm1k_wait_tail (simulation_v3.mm1k_wait_sweep: the runs' logs walked customer
by customer on the host; the first --warmup customers of a run, or an eighth of it, are left out).  Reads nothing outside
the repository."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import simulation_v3 as sv  # noqa: E402

GRID = ((0.5, 1.0, 1), (0.8, 1.0, 3), (1.0, 1.0, 5), (1.5, 1.0, 2), (1.6, 2.0, 4), (0.75, 0.5, 5))      # lam, mu, cap
MMC_GRID = ((1, 0.8, 1.0, 0), (2, 1.5, 1.0, 2), (2, 1.0, 1.0, 1), (3, 2.0, 1.0, 3), (4, 6.0, 1.0, 2),
            (3, 1.5, 1.0, 0))                                                                           # c, lam, mu, cap


def table(sw, heads, widths, n_runs):
    """One sweep's result, a line per compared cell; heads: per configuration, the columns in front."""
    worst = 0.0
    for c, head in enumerate(heads):
        for name in sv.SWEEP_NAMES:
            cells = [()] if sw.theory[name].ndim == 1 else [(j,) for j in range(widths[c])]
            for j in cells:
                i = (c,) + j
                label = name + (f"[{j[0]}]" if j else "")
                print(f"{head}  {label:<30} {sw.mean[name][i]:10.5f} {sw.sem[name][i]:9.5f} {sw.theory[name][i]:10.5f} "
                      f"{sw.z[name][i]:+6.2f}  {sw.n[name][i]}")
                worst = max(worst, abs(float(sw.z[name][i])))
    events = np.asarray(sw.stats.events.cpu() if hasattr(sw.stats.events, "cpu") else sw.stats.events)
    print(f"{len(heads)} configurations x {n_runs} seeds, {events.mean():.0f} events per run; largest |z| {worst:.2f}")


WAIT_TS = (0.5, 1.0, 2.0, 4.0)


def wait_table(sw, heads, n_runs):
    """mm1k_wait_sweep's result, a line per configuration and time."""
    for c, head in enumerate(heads):
        for j, t in enumerate(sw.ts):
            label = f"P(wait > {t:g})"
            print(f"{head}  {label:<30} {sw.mean[c, j]:10.5f} {sw.sem[c, j]:9.5f} {sw.theory[c, j]:10.5f} {sw.z[c, j]:+6.2f}  "
                  f"{sw.n[c, j]}")
    visits = np.diff(sw.visits.visit_ptr)
    print(f"{len(heads)} configurations x {n_runs} seeds, {visits.mean():.0f} visits per run; largest |z| "
          f"{np.abs(sw.z).max():.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default=None, help="a HIP device, e.g. cuda (default: the host mirror)")
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--customers", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=0, help="customers left out at the start (0: the whole runs only)")
    ap.add_argument("--waits", action="store_true", help="also the waiting-time law of the single-server grid")
    a = ap.parse_args()
    seeds = np.arange(a.seeds) * 11 + 5
    for warmup in ((0, a.warmup) if a.warmup else (0,)):
        print(f"---- customers {warmup} .. {a.customers}" + (" (the whole runs)" if not warmup else " (the window)"))
        lam, mu, cap = (np.array(c) for c in zip(*GRID))
        sw = sv.mm1k_sweep(lam, mu, cap, seeds, customers=a.customers, device=a.device, warmup=warmup)
        print(f"{'lam':>5} {'mu':>5} {'cap':>3}  {'quantity':<30} {'simulated':>10} {'sem':>9} {'theory':>10} {'z':>6}  n")
        table(sw, [f"{lam[c]:5.2f} {mu[c]:5.2f} {cap[c]:3d}" for c in range(len(GRID))], [int(k) + 1 for k in cap],
              a.seeds)
        cs, lam, mu, cap = (np.array(c) for c in zip(*MMC_GRID))
        sw = sv.mmck_sweep(cs, lam, mu, cap, seeds, customers=a.customers, device=a.device, warmup=warmup)
        print(f"\n{'c':>2} {'lam':>5} {'mu':>5} {'cap':>3}  {'quantity':<30} {'simulated':>10} {'sem':>9} {'theory':>10} "
              f"{'z':>6}  n")
        table(sw, [f"{cs[c]:2d} {lam[c]:5.2f} {mu[c]:5.2f} {cap[c]:3d}" for c in range(len(MMC_GRID))],
              [max(int(k), 1) + 1 for k in cap], a.seeds)
    if a.waits:
        skip = a.warmup if a.warmup else a.customers // 8
        print(f"---- waiting times of the accepted customers, the first {skip} of a run left out")
        lam, mu, cap = (np.array(c) for c in zip(*GRID))
        sw = sv.mm1k_wait_sweep(lam, mu, cap, seeds, WAIT_TS, customers=a.customers, skip=skip, device=a.device)
        print(f"{'lam':>5} {'mu':>5} {'cap':>3}  {'quantity':<30} {'simulated':>10} {'sem':>9} {'theory':>10} {'z':>6}  n")
        wait_table(sw, [f"{lam[c]:5.2f} {mu[c]:5.2f} {cap[c]:3d}" for c in range(len(GRID))], a.seeds)


if __name__ == "__main__":
    main()
