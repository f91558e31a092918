#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without the velocity-correlation accumulator (sgpr_md_vacf) on the
headline frame of bench.py (LiPS 4096 atoms, 512 inducing, fp64, deviates drawn on the device; --dims 32 32 16: 16384 atoms),
taken in ONE process: (a) the plain loop, calls of `--call` evaluations; (b) the loop with the accumulator at every = 1,
`--lags` lags, origin_every = 1; (c) the same at origin_every = 16; (d) at every = 10, origin_every = 1; (e) what a user had
before it: md_record(1, velocities and results), the frames of every call fetched behind it and fed to workloads.VacfRing
through observer_velocities on the host, for the table of (b) — `--host-steps` steps behind `--lags` untimed ones that fill the
ring, once: it is slow.  Every path is warmed up first; then they alternate in `--rounds` rounds of `--steps` steps, every window starting from the same frame.  The table is
read once at the end of a window, inside the timing.  Prints one JSON line: microseconds per step of each path per round, medians
and the differences to (a) per round, and whether the device's table equals the host pass's over the same steps.

    python tools/vacf_step_time.py [--rounds 2] [--steps 2048] [--call 256] [--lags 256] [--dims 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, VacfRing, fit_to_teacher, lips, observer_velocities

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
ap.add_argument("--host-steps", type=int, default=64)   # (timed once every lag has an origin)
ap.add_argument("--lags", type=int, default=256)
ap.add_argument("--dims", type=int, nargs="+", default=[16])
args = ap.parse_args()

numbers, pos, cell, pbc = lips(args.dims[0] if len(args.dims) == 1 else tuple(args.dims), seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
tables = {}


def loop(steps, every=0, origin_every=1, host=False, key=None, skip=0):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=FRICTION, kT=kB * T, seed=7)
    twin = None
    if every and host:
        mdl.md_record(every, velocities=True, results=True)
        twin = VacfRing(1, args.lags, origin_every, False, mass, numbers, mdl.species)   # (fed the sampled configurations only)
    elif every:
        mdl.md_vacf(every, args.lags, origin_every)
    done = timed_from = 0
    t0 = time.perf_counter()
    while done < steps:
        if skip and not timed_from and done >= skip:   # (the clock starts once every lag has an origin)
            timed_from, t0 = done, time.perf_counter()
        sc, code = mdl.md_run(min(args.call, (skip if done < skip else steps) - done), None)
        if code or not len(sc):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
        done += len(sc)
        if twin is not None and mdl.md_frame_count():
            f = mdl.md_frames(closed=False, reuse=True)
            for n, v, F in zip(f["index"], f["velocities_pre"], f["forces"]):
                twin.add(observer_velocities(v, F, mass, 0.5 * FS, 1 if n > 0 else 0))
    if key:
        tables[key] = twin.table() if host else mdl.md_vacf_table()
    return (time.perf_counter() - t0) / (done - timed_from)


paths = {"a_loop": lambda s: loop(s), "b_vacf_every_step": lambda s: loop(s, 1, 1),
         "c_vacf_every_step_origin_16": lambda s: loop(s, 1, 16), "d_vacf_every_tenth": lambda s: loop(s, 10, 1)}
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
host = [1e6 * loop(args.lags + args.host_steps, 1, 1, host=True, key="host", skip=args.lags)]
loop(args.lags + args.host_steps, 1, 1, key="device")
same = all(np.array_equal(tables["device"][k], tables["host"][k]) for k in ("tracer", "collective", "count", "samples", "pending", "next_due"))
times["e_record_and_host_pass_every_step"] = host
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, lags=args.lags, rounds=args.rounds, steps=args.steps, call=args.call, host_steps=args.host_steps,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()},
                      minus_loop_us={k: [round(b - a, 2) for a, b in zip(times["a_loop"], times[k])] for k in list(paths)[1:]},
                      device_and_host_tables_equal=bool(same))))
mdl.close()
