#!/usr/bin/env python3
"""Wall time per evaluation of the device relaxation under FIRE and under L-BFGS (sgpr_md_relax_lbfgs, md_lbfgs.inc) at memory 8
and memory 100, and the evaluations each needs to a common fmax, on the headline frame of bench.py (LiPS 4096 atoms, 512
inducing, fp64, the model fitted to the pair teacher), taken in ONE process.
  Timing: fmax far below reach, so nothing converges; every path is warmed up by `--warmup` evaluations (more than the longest
memory: the window of memory 100 is full when the clock starts), then the paths alternate in `--rounds` rounds of `--steps`
evaluations, each window going on from where the path's last one stopped and closed by the call's own synchronise.  An L-BFGS
evaluation costs what a FIRE one costs plus two passes over 2 memory (3N + 9) doubles and a memory x memory solve: the
difference of the medians is that cost.
  Counting: each optimizer from the same start to `--fmax` (eV/A, the largest generalised force), at most `--cap` evaluations;
null: not converged within the cap.  Positions only, and positions and cell.
Prints one JSON line.

    python tools/lbfgs_step_time.py [--rounds 3] [--steps 400] [--fmax 0.05]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.workloads import fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--warmup", type=int, default=150)
ap.add_argument("--fmax", type=float, default=0.05)
ap.add_argument("--cap", type=int, default=1500)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
PATHS = {"fire": dict(), "lbfgs_memory_8": dict(optimizer="LBFGS", memory=8), "lbfgs_memory_100": dict(optimizer="LBFGS", memory=100)}


def advance(steps):
    """`steps` more evaluations of the run on the model; seconds per evaluation."""
    done, stalls = 0, 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(min(steps - done, 256), None)
        done += len(sc)
        stalls = stalls + 1 if not len(sc) else 0
        if code in (1, 3) or stalls > 4:
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
    return (time.perf_counter() - t0) / done


def to_fmax(kw, cell_relax):
    mdl.relax_begin(numbers, pos, cell, pbc, args.fmax, cell_relax=cell_relax, **kw)
    done = 0
    while done < args.cap:
        sc, code = mdl.md_run(min(args.cap - done, 256), None)
        done += len(sc)
        if code == 3:
            return done, float(sc[-1][0])
        if code == 1 or (code and not len(sc)):
            break
    return None, float(sc[-1][0]) if len(sc) else None


# (one handle, one run at a time: every path keeps its own walk by being timed in one stretch per round from a fresh start
# warmed up by `warmup` evaluations — the start is the same frame for all three)
times = {k: [] for k in PATHS}
for _ in range(args.rounds):
    for k, kw in PATHS.items():
        mdl.relax_begin(numbers, pos, cell, pbc, 1e-12, **kw)
        advance(args.warmup)
        times[k].append(1e6 * advance(args.steps))
        mdl.md_end()
med = {k: float(np.median(v)) for k, v in times.items()}
counts = {("cell" if c else "positions"): {k: to_fmax(kw, c) for k, kw in PATHS.items()} for c in (False, True)}
out = dict(atoms=N, inducing=512, rounds=args.rounds, steps=args.steps, warmup=args.warmup,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in PATHS},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           lbfgs_8_minus_fire_us=round(med["lbfgs_memory_8"] - med["fire"], 2),
           lbfgs_100_minus_fire_us=round(med["lbfgs_memory_100"] - med["fire"], 2),
           fmax=args.fmax, cap=args.cap,
           evaluations_to_fmax={c: {k: v[0] for k, v in d.items()} for c, d in counts.items()},
           final_energy={c: {k: v[1] for k, v in d.items()} for c, d in counts.items()})
print(json.dumps(out))
mdl.close()
