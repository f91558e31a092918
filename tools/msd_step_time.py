#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without the displacement accumulator (sgpr_md_msd) on the headline
frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64, deviates drawn on the device), taken in ONE process: (a) the plain loop,
calls of `--call` evaluations; (b) the loop with the accumulator at every = 1, 16 levels; (c) at every = 10; (d) what a user had
before it: md_record(every, positions only), the frames of every call fetched behind it and fed to workloads.MsdBlocks on the
host, at every = 1; (e) the same at every = 10.  Every path is warmed up first; then they alternate in `--rounds` rounds of
`--steps` steps, every window starting from the same frame.  The table of (b) and (c) is read once at the end of a window, inside
the timing.  Prints one JSON line: microseconds per step of each path per round, medians and (b) - (a), (c) - (a) per round.

    python tools/msd_step_time.py [--rounds 2] [--steps 2048] [--call 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, MsdBlocks, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
ap.add_argument("--levels", type=int, default=16)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
tables = {}


def loop(steps, every=0, host=False):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    twin = None
    if every and host:
        mdl.md_record(every, velocities=False, results=False)
        twin = MsdBlocks(1, args.levels, False, mass, numbers, mdl.species)   # (fed the sampled configurations only)
    elif every:
        mdl.md_msd(every, args.levels)
    done = 0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(min(args.call, steps - done), None)
        if code or not len(sc):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
        done += len(sc)
        if twin is not None and mdl.md_frame_count():
            for x in mdl.md_frames(closed=False, reuse=True)["positions"]:
                twin.add(x)
    if every:
        tables[(every, host)] = twin.table() if host else mdl.md_msd_table()
    return (time.perf_counter() - t0) / done


paths = {"a_loop": lambda s: loop(s), "b_msd_every_step": lambda s: loop(s, 1), "c_msd_every_tenth": lambda s: loop(s, 10),
         "d_record_and_host_pass_every_step": lambda s: loop(s, 1, True), "e_record_and_host_pass_every_tenth": lambda s: loop(s, 10, True)}
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
same = all(np.array_equal(tables[(e, False)][k], tables[(e, True)][k]) for e in (1, 10) for k in ("count", "msd", "msd_sq", "smd", "smd_sq"))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, levels=args.levels, rounds=args.rounds, steps=args.steps, call=args.call,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()},
                      msd_every_step_minus_loop_us=[round(b - a, 2) for a, b in zip(times["a_loop"], times["b_msd_every_step"])],
                      msd_every_tenth_minus_loop_us=[round(c - a, 2) for a, c in zip(times["a_loop"], times["c_msd_every_tenth"])],
                      device_and_host_tables_equal=bool(same))))
mdl.close()
