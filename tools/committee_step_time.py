#!/usr/bin/env python3
"""Wall time per evaluation of MD with a Bayesian committee on the headline frame of bench.py (LiPS 4096 atoms, 512 inducing per
model, fp64), taken in ONE process, for K = 1 and K = 3 frozen members beside the live model: (a) the committee inside the
device loop (sgpr_md_committee: K + 1 plain steps and three small launches per evaluation), (b) the path such a run had
before — workloads.langevin_nvt around BCMActiveCalculator.calculate(), one synchronised predict per member and a numpy
combination per step — and (c) the plain single-model device loop for scale.  Every model has its own inducing set (drawn from
another frame) and is fitted to the pair teacher, so the trajectories hold together.  Every path is warmed up first; then they
alternate in `--rounds` rounds of `--steps` evaluations, every window starting from the same frame and closed by a device
synchronise.  Prints one JSON line: the median and the spread (max - min over the rounds) of the microseconds per evaluation of
each path and the ratios host / device per K.
--npt: the same comparison under a barostat (Nose-Hoover / Parrinello-Rahman, pfactor = (100 fs)^2 x 30 GPa, 1 GPa external,
tdamp = 25 fs): the committee inside the moving-cell device loop (sgpr_md_committee on a run with sgpr_md_barostat) against
workloads.npt_moving_cell around BCMActiveCalculator.calculate() with the same members, and the plain moving-cell loop for scale.

    python tools/committee_step_time.py [--npt] [--rounds 3] [--steps 1000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.calculator_bcm import BCMActiveCalculator
from autoforce_amd.posterior import PosteriorPotential
from autoforce_amd.npt import GPA
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips, npt_moving_cell

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--npt", action="store_true", help="under a barostat: the moving-cell loops")
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
models = []
for k in range(4):   # the live model, then three members
    mdl = bench.build_model(0, numbers, pos, cell, pbc, 512, workload_seed=1 + k)
    fit_to_teacher(mdl, numbers, pos, cell, pbc)
    models.append(mdl)
live, members = models[0], models[1:]
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION, TDAMP = 300.0, 0.02, 25.0
BARO = dict(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
calcs = {K: BCMActiveCalculator(covariance=PosteriorPotential(live), kernel_model_dict={f"m{k}": PosteriorPotential(members[k]) for k in range(K)},
                                logfile=None, pckl=None, tape=None) for K in (1, 3)}


def device(steps, K):
    if args.npt:
        live.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=0.0, kT=kB * T, ttime=TDAMP * FS, **BARO)
    else:
        live.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    if K:
        live.md_committee(members[:K], moving_cell=True if args.npt else None)
    sc, code = live.md_run(8, None)
    assert code == 0, code
    done = 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = live.md_run(steps - done, None)
        done += len(sc)
        if code == 1 or (code and not len(sc)):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
    dt = (time.perf_counter() - t0) / done
    info = [round(float(w), 4) for w in live.md_committee_info()[0]] if K else None
    live.md_end()
    return dt, info


def host(steps, K):
    if args.npt:
        it = npt_moving_cell(calcs[K], numbers, pos, cell, pbc, steps + 8, T, 1.0, TDAMP, vel=vel, species=live.species, **BARO)
    else:
        it = langevin_nvt(calcs[K], numbers, pos, cell, pbc, steps + 8, T, 1.0, FRICTION, seed=7, vel=vel)
    for _ in range(9):
        next(it)
    t0 = time.perf_counter()
    for _ in it:                # (every evaluation ends in the predicts' own synchronise)
        pass
    return (time.perf_counter() - t0) / steps, [round(float(w), 4) for w in calcs[K].bcm_weights.values()]


paths = {"device_plain": lambda s: device(s, 0), "device_committee_K1": lambda s: device(s, 1), "device_committee_K3": lambda s: device(s, 3),
         "host_committee_K1": lambda s: host(s, 1), "host_committee_K3": lambda s: host(s, 3)}
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
weights = {}
for _ in range(args.rounds):
    for k, f in paths.items():
        t, w = f(args.steps)
        times[k].append(1e6 * t)
        weights[k] = w
med = {k: float(np.median(v)) for k, v in times.items()}
out = dict(atoms=N, inducing=512, dynamics="npt" if args.npt else "langevin", rounds=args.rounds, steps=args.steps,
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           host_over_device_K1=round(med["host_committee_K1"] / med["device_committee_K1"], 3),
           host_over_device_K3=round(med["host_committee_K3"] / med["device_committee_K3"], 3),
           committee_K1_over_plain=round(med["device_committee_K1"] / med["device_plain"], 3),
           committee_K3_over_plain=round(med["device_committee_K3"] / med["device_plain"], 3),
           last_weights=weights)
print(json.dumps(out))
for mdl in models:
    mdl.close()
