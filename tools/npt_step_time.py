#!/usr/bin/env python3
"""Wall time per MD step of the three thermostatted dynamics on the headline frame of bench.py (LiPS 4096 atoms, 512 inducing,
fp64), taken in ONE process: (a) the Nose-Hoover device loop, (b) the moving-cell (NPT) device loop — sgpr_md_barostat —,
(c) npt.NPT around calculate() of the device calculator, one synchronised call per step, as cl/md.py runs a bulk modulus today.
Every path is warmed up first; then the three alternate in `--rounds` rounds of `--steps` steps, every window starting from
the same frame and velocities and closed by a device synchronise (md_run and predict both end with one).  Prints one JSON
line: the median and the spread (max - min over the rounds) of the microseconds per step of each path, the ratios b/a and
c/b, and the list rebuilds per 1000 steps of (b) and (c).

    python tools/npt_step_time.py [--rounds 5] [--steps 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import Atoms, kB
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.npt import GPA, NPT
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
args = ap.parse_args()

T, TDAMP = 600.0, 25.0
BARO = dict(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
v0 = np.random.default_rng(0).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None)


def device(steps, **baro):
    mdl.md_begin(numbers, pos, cell, pbc, mass, v0, dt=FS, friction=0.0, kT=kB * T, ttime=TDAMP * FS, **baro)
    sc, code = mdl.md_run(8, None)     # (the start of the trajectory — a synchronised evaluation under a barostat — is not a step)
    assert code == 0, code
    r0, done = mdl.list_rebuilds(), 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(steps - done, None)
        done += len(sc)
        if code == 1 or (code and not len(sc)):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} steps")
    return (time.perf_counter() - t0) / done, (mdl.list_rebuilds() - r0) * 1000.0 / done


def host(steps):
    at = Atoms(numbers, pos.copy(), cell.copy(), pbc, velocities=v0, masses=mass)
    at.calc = calc
    dyn = NPT(at, FS, T, externalstress=BARO["externalstress"], ttime=TDAMP * FS, pfactor=BARO["pfactor"])
    run = dyn.run(steps + 8)
    for _ in range(9):
        next(run)
    r0 = mdl.list_rebuilds()
    t0 = time.perf_counter()
    n = sum(1 for _ in run)      # (every step ends in calculate()'s own synchronise)
    return (time.perf_counter() - t0) / n, (mdl.list_rebuilds() - r0) * 1000.0 / n


paths = {"nose_hoover_device": lambda s: device(s), "npt_device": lambda s: device(s, **BARO), "npt_host": host}
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
           us_per_step={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           npt_device_over_nose_hoover_device=round(med["npt_device"] / med["nose_hoover_device"], 3),
           npt_host_over_npt_device=round(med["npt_host"] / med["npt_device"], 3),
           rebuilds_per_1000_steps={k: round(float(np.median(rebuilds[k])), 1) for k in ("npt_device", "npt_host")})
print(json.dumps(out))
mdl.close()
