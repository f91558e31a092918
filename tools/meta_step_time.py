#!/usr/bin/env python3
"""Wall time per evaluation of the device MD loop with and without metadynamics (sgpr_md_meta) on the headline frame of bench.py
(LiPS 4096 atoms, 512 inducing, fp64), taken in ONE process: (a) the plain Langevin device loop (deviates drawn on the device);
the same loop biased on (b) a distance and (c) a posvar over all atoms (dense: every atom receives a bias force), each with 0,
1 000 and 100 000 hills preloaded — spread over +-10 sigma around the starting CV, so about half of them pass the block rule and
cost an exp —; and the path a biased run had before the bias reached the device: (d) workloads.langevin_nvt around calculate() of
the device calculator with the same Meta (distance, 1 000 hills), one synchronised call and one numpy bias per step — the twin
walks the hills in the kernel's order, in Python: a large part of that path's time —, and (e) the same host loop with a Meta that
starts without hills.  Every path
is warmed up first; then they alternate in `--rounds` rounds of `--steps` evaluations, every window starting from the same frame
and the same hills and closed by a device synchronise.  Prints one JSON line: the median and the spread (max - min over the
rounds) of the microseconds per evaluation of each path, and what the bias adds to the plain loop.

    python tools/meta_step_time.py [--rounds 3] [--steps 4000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.meta import Distance, Meta
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips, meta_bias

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--host-steps", type=int, default=400)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION, SIGMA, W = 300.0, 0.02, 0.1, 0.01
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
CVS = {"distance": [("distance", 0, N - 1)], "posvar": [("posvar", 0, None)]}
HILLS = (0, 1000, 100000)


def hills(kind, H):
    cv0 = meta_bias(CVS[kind], SIGMA, W, numbers, pos, cell, None, species=mdl.species)["cv"]
    return cv0 + SIGMA * np.random.default_rng(5).uniform(-10.0, 10.0, size=(H, len(cv0)))


def loop(steps):
    sc, code = mdl.md_run(8, None)
    assert code == 0, code
    done = 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(steps - done, None)
        done += len(sc)
        if code in (1, 3) or (code and not len(sc)):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
    return (time.perf_counter() - t0) / done


def device(steps, kind=None, H=0):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    if kind:
        mdl.md_meta(CVS[kind], SIGMA, W, hills=hills(kind, H) if H else None, capacity=H + steps + 16)
    return loop(steps)


def langevin_host(steps, H=1000):
    steps = min(steps, args.host_steps)
    meta = Meta(Distance(0, N - 1), sigma=SIGMA, w=W, hist=None)
    meta.species = list(mdl.species)
    meta.hills = list(hills("distance", H))
    calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None, meta=meta)
    it = langevin_nvt(calc, numbers, pos, cell, pbc, steps + 8, T, 1.0, FRICTION, seed=7, vel=vel)
    for _ in range(9):
        next(it)
        meta.update()
    t0 = time.perf_counter()
    for _ in it:                # (every evaluation ends in calculate()'s own synchronise; the bias is post_calculate's)
        meta.update()
    return (time.perf_counter() - t0) / steps


paths = {"plain": lambda s: device(s)}
for kind in CVS:
    for H in HILLS:
        paths[f"{kind}_{H}"] = (lambda s, kind=kind, H=H: device(s, kind, H))
paths["host_distance_1000"] = langevin_host
paths["host_distance_0"] = lambda s: langevin_host(s, 0)
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
med = {k: float(np.median(v)) for k, v in times.items()}
out = dict(atoms=N, inducing=512, sigma=SIGMA, rounds=args.rounds, steps=args.steps,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           added_us={k: round(med[k] - med["plain"], 2) for k in paths if not k.startswith(("plain", "host"))},
           host_over_device_distance_1000=round(med["host_distance_1000"] / med["distance_1000"], 3))
print(json.dumps(out))
mdl.close()
