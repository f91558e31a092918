#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without the bond-angle accumulator (sgpr_md_adf) on the headline frame
of bench.py (LiPS 4096 atoms, 512 inducing, fp64, deviates drawn on the device), taken in ONE process: (a) the plain loop, calls
of `--call` evaluations; (b) the loop with the accumulator at every = 1 and bond cutoffs (P-S 2.6, Li-S 3.0, the other pairs never
bond), `--bins` bins; (c) at every = 1 with all cutoffs at the model's rc (every list entry a neighbour); (d) (b) at every = 10;
(e) what a user had before it: md_record(1, positions only), the frames of every call fetched behind it and fed to
workloads.AdfCounts on the host, bond cutoffs.  The host pass takes about a second per configuration, so (e) runs `--host-steps`
steps per window (--host-steps 0 leaves it out: larger frames).  Every path is warmed up first; then they alternate in `--rounds`
rounds of `--steps` steps, every window starting from the same frame.  The tables are read once at the end of a window, inside the
timing.  Prints one JSON line: microseconds per step of each path per round, medians, (b) - (a), (c) - (a) and (d) - (a) per round,
and whether the device's tables equal the host's over the same `--host-steps` steps.

    python tools/adf_step_time.py [--rounds 2] [--steps 2048] [--call 256] [--dims 16 | --dims 32 32 16 --host-steps 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, AdfCounts, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
ap.add_argument("--host-steps", type=int, default=4)
ap.add_argument("--dims", type=int, nargs="+", default=[16])
ap.add_argument("--bins", type=int, default=180)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(args.dims[0] if len(args.dims) == 1 else tuple(args.dims), seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
BONDS = {(15, 16): 2.6, (3, 16): 3.0}
RC = float(mdl.cutoff)
tables = {}


def loop(steps, every=0, host=False, cut=BONDS, key=None):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    twin = None
    if every and host:
        mdl.md_record(every, velocities=False, results=False)
        twin = AdfCounts(1, args.bins, cut, numbers, mdl.species, cell, pbc)   # (fed the sampled configurations only)
    elif every:
        mdl.md_adf(every, args.bins, cut)
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
        tables[key] = twin.table() if host else mdl.md_adf_table()
    return (time.perf_counter() - t0) / done


paths = {"a_loop": lambda s: loop(s), "b_adf_bonds_every_step": lambda s: loop(s, 1), "c_adf_rc_every_step": lambda s: loop(s, 1, cut=RC),
         "d_adf_bonds_every_tenth": lambda s: loop(s, 10)}
if args.host_steps:
    paths["e_record_and_host_pass_every_step"] = lambda s: loop(args.host_steps, 1, True, key="host")
for k, f in paths.items():
    if not k.startswith("e_"):
        f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
same = None
if args.host_steps:
    loop(args.host_steps, 1, key="device")
    same = bool(all(np.array_equal(tables["device"][k], tables["host"][k]) for k in ("angles", "coord")) and
                tables["device"]["samples"] == tables["host"]["samples"])
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, rc=RC, bins=args.bins, rounds=args.rounds, steps=args.steps, call=args.call, host_steps=args.host_steps,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()},
                      adf_bonds_every_step_minus_loop_us=[round(b - a, 2) for a, b in zip(times["a_loop"], times["b_adf_bonds_every_step"])],
                      adf_rc_every_step_minus_loop_us=[round(b - a, 2) for a, b in zip(times["a_loop"], times["c_adf_rc_every_step"])],
                      adf_bonds_every_tenth_minus_loop_us=[round(c - a, 2) for a, c in zip(times["a_loop"], times["d_adf_bonds_every_tenth"])],
                      device_and_host_tables_equal=same)))
mdl.close()
