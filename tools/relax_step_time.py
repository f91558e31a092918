#!/usr/bin/env python3
"""Wall time per evaluation of a FIRE relaxation on the headline frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64), taken
in ONE process: (a) the device relaxation, positions only — sgpr_md_relax —, (b) the same with the cell, (c) cl/relax.py's FIRE
around calculate() of the device calculator, one synchronised call per step (what relax(algo="FIRE") ran before the device
loop), (d) the velocity-Verlet device loop as the floor (an MD step: the integrator inside the evaluation's last kernel).
Every path is warmed up first; then the four alternate in `--rounds` rounds of `--steps` evaluations, every window starting
from the same frame and closed by a device synchronise.  Prints one JSON line: the median and the spread (max - min over the
rounds) of the microseconds per evaluation of each path, (a) - (d), (b) - (a), (c) / (a) and the list rebuilds per 1000
evaluations.

    python tools/relax_step_time.py [--rounds 2] [--steps 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import Atoms
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.cl.relax import FIRE
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None)


def loop(steps):
    sc, code = mdl.md_run(8, None)
    assert code == 0, code
    r0, done = mdl.list_rebuilds(), 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(steps - done, None)
        done += len(sc)
        if code in (1, 3) or (code and not len(sc)):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
    return (time.perf_counter() - t0) / done, (mdl.list_rebuilds() - r0) * 1000.0 / done


def relax_device(steps, cell_relax=False):
    mdl.relax_begin(numbers, pos, cell, pbc, 1e-12, cell_relax=cell_relax)
    return loop(steps)


def verlet_device(steps):
    mdl.md_begin(numbers, pos, cell, pbc, mass, np.zeros((N, 3)), dt=FS, friction=0.0, kT=0.0)
    return loop(steps)


def fire_host(steps):
    at = Atoms(numbers, pos.copy(), cell.copy(), pbc)
    at.calc = calc
    opt = FIRE(at)
    for _ in range(8):
        opt.step(at.get_forces())
    r0 = mdl.list_rebuilds()
    t0 = time.perf_counter()
    for _ in range(steps):      # (every evaluation ends in calculate()'s own synchronise)
        opt.step(at.get_forces())
    return (time.perf_counter() - t0) / steps, (mdl.list_rebuilds() - r0) * 1000.0 / steps


paths = {"relax_device": relax_device, "relax_cell_device": lambda s: relax_device(s, True), "fire_host": fire_host,
         "verlet_device": verlet_device}
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
rebuilds = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        t, r = f(args.steps)
        times[k].append(1e6 * t)
        rebuilds[k].append(r)
med = {k: float(np.median(v)) for k, v in times.items()}
out = dict(atoms=N, inducing=512, rounds=args.rounds, steps=args.steps,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           relax_minus_verlet_us=round(med["relax_device"] - med["verlet_device"], 2),
           cell_minus_positions_us=round(med["relax_cell_device"] - med["relax_device"], 2),
           fire_host_over_relax_device=round(med["fire_host"] / med["relax_device"], 3),
           rebuilds_per_1000={k: round(float(np.median(rebuilds[k])), 1) for k in paths})
print(json.dumps(out))
mdl.close()
