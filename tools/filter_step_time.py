#!/usr/bin/env python3
"""Wall time per evaluation of the device MD loop with and without the filter of model-update jumps (sgpr_md_filter) on the
headline frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64), taken in ONE process: (a) the Langevin device loop (deviates
drawn on the device) without a filter, (b) the same with a filter whose accumulators are non-zero (order 0.3 eV/A with a few
components beyond the clamp, pushed again at the start of every window: they decay by `shrink` per evaluation), (c) the
Nose-Hoover device loop without a filter, (d) the same with the filter — and the path a filtered run had before the filter reached
the device: (e) workloads.langevin_nvt(ml_filter=) around calculate() of the device calculator, one synchronised call per step.
Every path is warmed up first; then they alternate in `--rounds` rounds of `--steps` evaluations, every window starting from
the same frame and closed by a device synchronise.  Prints one JSON line: the median and the spread (max - min over the rounds)
of the microseconds per evaluation of each path, the ratios (b) / (a), (d) / (c), (e) / (b) and the list rebuilds per 1000
evaluations.

    python tools/filter_step_time.py [--rounds 3] [--steps 2000]"""
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
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--host-steps", type=int, default=300)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None)
T, FRICTION, TDAMP, SHRINK = 300.0, 0.02, 25.0, 0.8
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
rng = np.random.default_rng(2)
acc0 = 0.3 * rng.normal(size=(N, 3))
acc0[rng.permutation(N)[:32], rng.integers(0, 3, 32)] = 5.0
acc0[rng.permutation(N)[:32], rng.integers(0, 3, 32)] = -5.0


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


def device(steps, nh, filt):
    kw = dict(ml_filter=SHRINK, filter_init=(acc0, None)) if filt else {}
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=0.0 if nh else FRICTION, kT=kB * T, seed=0 if nh else 7,
                 ttime=TDAMP * FS if nh else None, **kw)
    return loop(steps)


class Jumps:
    """calculate() of the device calculator with `deltas` republished every 25 evaluations: the host filter's accumulators stay
    non-zero as an updating model would keep them."""

    def __init__(self, inner):
        self.inner, self.n, self.deltas = inner, 0, None

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def get_property(self, name, atoms=None):
        out = self.inner.get_property(name, atoms)
        if name == "forces":
            self.deltas = dict(energy=0.0, forces=acc0, stress=np.zeros(6)) if self.n % 25 == 0 else None
            self.n += 1
        return out


def langevin_host(steps):
    steps = min(steps, args.host_steps)
    it = langevin_nvt(Jumps(calc), numbers, pos, cell, pbc, steps + 8, T, 1.0, FRICTION, seed=7, vel=vel, ml_filter=SHRINK)
    for _ in range(9):
        next(it)
    r0 = mdl.list_rebuilds()
    t0 = time.perf_counter()
    for _ in it:                # (every evaluation ends in calculate()'s own synchronise)
        pass
    return (time.perf_counter() - t0) / steps, (mdl.list_rebuilds() - r0) * 1000.0 / steps


paths = {"langevin_device": lambda s: device(s, False, False), "langevin_device_filtered": lambda s: device(s, False, True),
         "nose_hoover_device": lambda s: device(s, True, False), "nose_hoover_device_filtered": lambda s: device(s, True, True),
         "langevin_host_filtered": langevin_host}
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
out = dict(atoms=N, inducing=512, shrink=SHRINK, rounds=args.rounds, steps=args.steps,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           langevin_filtered_over_unfiltered=round(med["langevin_device_filtered"] / med["langevin_device"], 4),
           nose_hoover_filtered_over_unfiltered=round(med["nose_hoover_device_filtered"] / med["nose_hoover_device"], 4),
           langevin_host_over_device_filtered=round(med["langevin_host_filtered"] / med["langevin_device_filtered"], 3),
           rebuilds_per_1000={k: round(float(np.median(rebuilds[k])), 1) for k in paths})
print(json.dumps(out))
mdl.close()
