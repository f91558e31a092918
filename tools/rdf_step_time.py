#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without the pair-distance accumulator (sgpr_md_rdf) on the headline
frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64, deviates drawn on the device), taken in ONE process: (a) the plain loop,
calls of `--call` evaluations; (b) the loop with the accumulator at every = 1, rmax = 6, 120 bins (one image per pair); (c) at
every = 10; (d) at every = 10 with `--rmax-images` (default 24: beyond half the cell, the block of 27 images); (e) what a user
had before it: md_record(every, positions only), the frames of every call fetched behind it and fed to workloads.RdfCounts on the
host, at every = 1; (f) the same at every = 10.  The host pass is O(N^2) in numpy and takes seconds per configuration, so (e) and
(f) run `--host-steps` steps per window (--host-steps 0 leaves them out: larger frames).  Every path is warmed up first; then they
alternate in `--rounds` rounds of `--steps` steps, every window starting from the same frame.  The table is read once at the end
of a window, inside the timing.  Prints one JSON line: microseconds per step of each path per round, medians, (b) - (a) and
(c) - (a) per round, and whether the device's table equals the host's over the same `--host-steps` steps.

    python tools/rdf_step_time.py [--rounds 2] [--steps 2048] [--call 256] [--dims 16 | --dims 32 32 16 --host-steps 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, RdfCounts, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
ap.add_argument("--host-steps", type=int, default=10)
ap.add_argument("--dims", type=int, nargs="+", default=[16])
ap.add_argument("--rmax", type=float, default=6.0)
ap.add_argument("--bins", type=int, default=120)
ap.add_argument("--rmax-images", type=float, default=24.0)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(args.dims[0] if len(args.dims) == 1 else tuple(args.dims), seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
tables = {}


def loop(steps, every=0, host=False, rmax=args.rmax, key=None):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    twin = None
    if every and host:
        mdl.md_record(every, velocities=False, results=False)
        twin = RdfCounts(1, rmax, args.bins, 0.0, numbers, mdl.species, cell, pbc)   # (fed the sampled configurations only)
    elif every:
        mdl.md_rdf(every, rmax, args.bins)
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
        tables[key] = twin.table() if host else mdl.md_rdf_table()
    return (time.perf_counter() - t0) / done


paths = {"a_loop": lambda s: loop(s), "b_rdf_every_step": lambda s: loop(s, 1), "c_rdf_every_tenth": lambda s: loop(s, 10),
         "d_rdf_images_every_tenth": lambda s: loop(s, 10, rmax=args.rmax_images)}
if args.host_steps:
    paths["e_record_and_host_pass_every_step"] = lambda s: loop(args.host_steps, 1, True, key="host")
    paths["f_record_and_host_pass_every_tenth"] = lambda s: loop(10 * max(1, args.host_steps // 5), 10, True)
for k, f in paths.items():
    if not k.startswith(("e_", "f_")):
        f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
same = None
if args.host_steps:
    loop(args.host_steps, 1, key="device")
    same = bool(np.array_equal(tables["device"]["hist"], tables["host"]["hist"]) and tables["device"]["samples"] == tables["host"]["samples"])
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, rmax=args.rmax, bins=args.bins, rmax_images=args.rmax_images, rounds=args.rounds, steps=args.steps,
                      call=args.call, host_steps=args.host_steps,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()},
                      rdf_every_step_minus_loop_us=[round(b - a, 2) for a, b in zip(times["a_loop"], times["b_rdf_every_step"])],
                      rdf_every_tenth_minus_loop_us=[round(c - a, 2) for a, c in zip(times["a_loop"], times["c_rdf_every_tenth"])],
                      device_and_host_tables_equal=same)))
mdl.close()
