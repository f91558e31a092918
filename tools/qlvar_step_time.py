#!/usr/bin/env python3
"""Wall time per evaluation of the device MD loop biased on the Steinhardt Q6 of one atom (kind 2 of sgpr_md_meta: Qlvar) on the
headline frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64), taken in ONE process, after tools/meta_step_time.py: (a) the plain
Langevin device loop (deviates drawn on the device); the same loop biased on (b) a distance, (c) a posvar over all atoms and (d)
Q6 of the first Li atom over its S neighbours inside 4.0 A, each with 1 000 hills preloaded — spread over +-10 sigma around the
starting CV, so about half of them pass the block rule and cost an exp —; and the path a Qlvar run had before: (e)
workloads.langevin_nvt around calculate() of the device calculator with the same Meta (Q6, 1 000 hills), one synchronised call
and one numpy bias per step.  Every path is warmed up first; then they alternate in `--rounds` rounds of `--steps` evaluations,
every window starting from the same frame and the same hills and closed by a device synchronise.  Prints one JSON line: the median
and the spread (max - min over the rounds) of the microseconds per evaluation of each path, and what each bias adds to the plain
loop.

    python tools/qlvar_step_time.py [--rounds 3] [--steps 4000]"""
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
from autoforce_amd.meta import Meta, Qlvar
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips, meta_bias, ql_environment

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
T, FRICTION, W, H = 300.0, 0.02, 0.01, 1000
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
LI = int(np.where(numbers == 3)[0][0])
CUTOFF = 4.0
CVS = {"distance": ([("distance", 0, N - 1)], 0.1), "posvar": ([("posvar", 0, None)], 0.1), "qlvar": ([("qlvar", LI, 16, CUTOFF, (6,))], 0.02)}
KW = dict(pbc=pbc, rc=mdl.cutoff)


def hills(kind):
    cvs, sigma = CVS[kind]
    cv0 = meta_bias(cvs, sigma, W, numbers, pos, cell, None, species=mdl.species, **KW)["cv"]
    return cv0 + sigma * np.random.default_rng(5).uniform(-10.0, 10.0, size=(H, len(cv0)))


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


def device(steps, kind=None):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    if kind:
        mdl.md_meta(CVS[kind][0], CVS[kind][1], W, hills=hills(kind), capacity=H + steps + 16)
    return loop(steps)


def langevin_host(steps):
    steps = min(steps, args.host_steps)
    meta = Meta(Qlvar(3, 16, index=LI, cutoff=CUTOFF, l=[6]), sigma=CVS["qlvar"][1], w=W, hist=None)
    meta.species, meta.rc = list(mdl.species), mdl.cutoff
    meta.hills = list(hills("qlvar"))
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
    paths[f"{kind}_{H}"] = (lambda s, kind=kind: device(s, kind))
paths[f"host_qlvar_{H}"] = langevin_host
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
med = {k: float(np.median(v)) for k, v in times.items()}
env = ql_environment(numbers, pos, cell, pbc, LI, 16, CUTOFF)
out = dict(atoms=N, inducing=512, hills=H, rounds=args.rounds, steps=args.steps, qlvar=dict(index=LI, j=16, cutoff=CUTOFF, l=[6], selected=len(env[0])),
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           added_us={k: round(med[k] - med["plain"], 2) for k in paths if not k.startswith(("plain", "host"))},
           host_over_device_qlvar=round(med[f"host_qlvar_{H}"] / med[f"qlvar_{H}"], 3))
print(json.dumps(out))
mdl.close()
