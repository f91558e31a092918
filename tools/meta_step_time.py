#!/usr/bin/env python3
"""Wall time per evaluation of the device MD loop with and without metadynamics (sgpr_md_meta) on the headline frame of bench.py
(LiPS 4096 atoms, 512 inducing, fp64), taken in ONE process: (a) the plain Langevin device loop (deviates drawn on the device);
the same loop biased on (b) a distance and (c) a posvar over all atoms (dense: every atom receives a bias force), each with 0,
1 000 and 100 000 hills preloaded — spread over +-10 sigma around the starting CV, so about half of them pass the block rule and
cost an exp —; and the path a biased run had before the bias reached the device: (d) workloads.langevin_nvt around calculate() of
the device calculator with the same Meta (distance, 1 000 hills), one synchronised call and one numpy bias per step — the twin
walks the hills in the kernel's order, in Python: a large part of that path's time —, and (e) the same host loop with a Meta that
starts without hills; and (f) the merged form of the bias (md_meta(merge=1024)): the same frame, CVs and hill counts with the hills
drawn from a CONFINED walk around the starting CV (an Ornstein-Uhlenbeck walk 1.5 sigma wide per dimension, so that bins are
revisited as in a long run), every count both unmerged (`<cv>_<H>_walk`) and merged (`<cv>_<H>_walk_merged`) on the same hills,
the height w scaled by min(1, 1000 / H) so that the preloaded bias stays that of 1 000 hills (the cost of the sum does not depend
on w; the dynamics do), with the number of occupied bins (`bins`) and the time of one merge launch at the table sizes reached (`merge_launch_us`: a
synchronous sgpr_md_meta_merge of the preloaded hills with the buffers allocated, over its chunks).  Every path
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
from autoforce_amd import _lib
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, langevin_nvt, lips, meta_bias, meta_table

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
MERGE = 1024


def hills(kind, H):
    cv0 = meta_bias(CVS[kind], SIGMA, W, numbers, pos, cell, None, species=mdl.species)["cv"]
    return cv0 + SIGMA * np.random.default_rng(5).uniform(-10.0, 10.0, size=(H, len(cv0)))


def walk_hills(kind, H):
    """H deposits of a walk that stays where it has been: x <- x - 0.05 (x - cv0) + 0.47 sigma xi, 1.5 sigma wide per dimension"""
    cv0 = meta_bias(CVS[kind], SIGMA, W, numbers, pos, cell, None, species=mdl.species)["cv"]
    xi = 0.47 * SIGMA * np.random.default_rng(6).normal(size=(H, len(cv0)))
    out, x = np.empty((H, len(cv0))), np.zeros(len(cv0))
    for n in range(H):
        x = 0.95 * x + xi[n]
        out[n] = x
    return cv0 + out


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


def device(steps, kind=None, H=0, draw=hills, merge=None):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    if kind:
        # (the walk's hills stand in a handful of bins: their height is scaled so that 100 000 of them are the bias of 1 000 — at full
        # height they are thousands of eV/A on the CV's atoms, which then fly apart through a new bin every step)
        w = W if draw is hills else W * min(1.0, 1000.0 / max(H, 1))
        mdl.md_meta(CVS[kind], SIGMA, w, hills=draw(kind, H) if H else None, capacity=H + steps + 16, merge=merge)
    return loop(steps)


def merge_launch(kind, H):
    """(occupied bins of the H walk hills' whole chunks, microseconds per merge launch): the attach merges the uploaded chunks
    synchronously, one launch each; timed on the second call, when the table's buffers stand"""
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    h = walk_hills(kind, H)
    mdl.md_meta(CVS[kind], SIGMA, W, hills=h, capacity=H + 16, merge=MERGE)
    t0 = time.perf_counter()
    _lib.check(_lib.load().sgpr_md_meta_merge(mdl.handle, MERGE))
    dt = time.perf_counter() - t0
    bins = len(mdl.md_meta_table()[1])   # (of the preloaded hills; the run adds the bins it visits)
    assert bins == len(meta_table(h, SIGMA, MERGE)[2])
    return bins, 1e6 * dt / max(H // MERGE, 1)


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
        if H:
            paths[f"{kind}_{H}_walk"] = (lambda s, kind=kind, H=H: device(s, kind, H, draw=walk_hills))
        paths[f"{kind}_{H}_walk_merged"] = (lambda s, kind=kind, H=H: device(s, kind, H, draw=walk_hills, merge=MERGE))
paths["host_distance_1000"] = langevin_host
paths["host_distance_0"] = lambda s: langevin_host(s, 0)
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
med = {k: float(np.median(v)) for k, v in times.items()}
merges = {f"{kind}_{H}": merge_launch(kind, H) for kind in CVS for H in HILLS if H >= MERGE}
out = dict(atoms=N, inducing=512, sigma=SIGMA, rounds=args.rounds, steps=args.steps, merge=MERGE,
           bins={k: v[0] for k, v in merges.items()}, merge_launch_us={k: round(v[1], 2) for k, v in merges.items()},
           us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
           median_us={k: round(med[k], 2) for k in paths},
           spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
           added_us={k: round(med[k] - med["plain"], 2) for k in paths if not k.startswith(("plain", "host"))},
           host_over_device_distance_1000=round(med["host_distance_1000"] / med["distance_1000"], 3))
print(json.dumps(out))
mdl.close()
