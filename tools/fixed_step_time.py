#!/usr/bin/env python3
"""Wall time per evaluation of the device loops with and without held atoms (sgpr_md_fix) on the headline frame of bench.py
(LiPS 4096 atoms, 512 inducing, fp64), taken in ONE process: (a) the Langevin device loop (deviates drawn on the device) without
a mask, (b) the same with the lowest quarter of the atoms in z held, (c) the FIRE device loop without a mask, (d) the same with
the mask — and the paths a constrained user had before the mask reached the device: (e) workloads.langevin_nvt(fixed=) and (f)
cl/relax.py's FIRE on constrained atoms, each around calculate() of the device calculator, one synchronised call per step.
Every path is warmed up first; then they alternate in `--rounds` rounds of `--steps` evaluations, every window starting from
the same frame and closed by a device synchronise.  Prints one JSON line: the median and the spread (max - min over the rounds)
of the microseconds per evaluation of each path, the ratios (b) / (a), (d) / (c), (e) / (b), (f) / (d) and the list rebuilds per
1000 evaluations.

    python tools/fixed_step_time.py [--rounds 3] [--steps 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import Atoms, FixAtoms, kB
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.cl.relax import FIRE
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None)
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
held = np.zeros(N, bool)
held[np.argsort(pos[:, 2], kind="stable")[:N // 4]] = True


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


def langevin_device(steps, fixed=None):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7, fixed=fixed)
    return loop(steps)


def fire_device(steps, fixed=None):
    mdl.relax_begin(numbers, pos, cell, pbc, 1e-12, fixed=fixed)
    return loop(steps)


def langevin_host(steps):
    it = langevin_nvt(calc, numbers, pos, cell, pbc, steps + 8, T, 1.0, FRICTION, seed=7, vel=vel, fixed=held)
    for _ in range(9):
        next(it)
    r0 = mdl.list_rebuilds()
    t0 = time.perf_counter()
    for _ in it:                # (every evaluation ends in calculate()'s own synchronise)
        pass
    return (time.perf_counter() - t0) / steps, (mdl.list_rebuilds() - r0) * 1000.0 / steps


def fire_host(steps):
    at = Atoms(numbers, pos.copy(), cell.copy(), pbc, constraint=FixAtoms(mask=held))
    at.calc = calc
    opt = FIRE(at)
    for _ in range(8):
        opt.step(at.get_forces())
    r0 = mdl.list_rebuilds()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step(at.get_forces())
    return (time.perf_counter() - t0) / steps, (mdl.list_rebuilds() - r0) * 1000.0 / steps


paths = {"langevin_device": langevin_device, "langevin_device_masked": lambda s: langevin_device(s, held),
         "fire_device": fire_device, "fire_device_masked": lambda s: fire_device(s, held),
         "langevin_host_masked": langevin_host, "fire_host_masked": fire_host}
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
out = dict(atoms=N, inducing=512, held_atoms=int(held.sum()), rounds=args.rounds, steps=args.steps,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           langevin_masked_over_unmasked=round(med["langevin_device_masked"] / med["langevin_device"], 4),
           fire_masked_over_unmasked=round(med["fire_device_masked"] / med["fire_device"], 4),
           langevin_host_over_device_masked=round(med["langevin_host_masked"] / med["langevin_device_masked"], 3),
           fire_host_over_device_masked=round(med["fire_host_masked"] / med["fire_device_masked"], 3),
           rebuilds_per_1000={k: round(float(np.median(rebuilds[k])), 1) for k in paths})
print(json.dumps(out))
mdl.close()
