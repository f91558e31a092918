#!/usr/bin/env python3
"""Wall time per step of the Langevin device loop with and without the frame record (sgpr_md_record) on the headline frame of
bench.py (LiPS 4096 atoms, 512 inducing, fp64, deviates drawn on the device), taken in ONE process: (a) the loop without
recording, calls of `--call` evaluations; (b) recording every step, positions + velocities + packed results, the frames of
every call fetched behind it (md_frames: three device-to-host copies into buffers that are kept); (c) recording every tenth
step, fetched likewise; (d) the cut path a trajectory writer had before the record: md_run(1) + md_state(which=-1) per step;
and, as the yardstick for "one more small launch per step", (e) the Nose-Hoover loop (md_nh_kernel behind every evaluation)
without recording.  Every path is warmed up first; then they alternate in `--rounds` rounds of `--steps` steps, every window
starting from the same frame.  The fetch's share of (b) is timed inside it.  Prints one JSON line: microseconds per step of
each path per round, medians, (b) - (a), (e) - (a), the fetch's share and whether (b) < (d) held in every round.

    python tools/record_step_time.py [--rounds 2] [--steps 2048] [--call 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2048)
ap.add_argument("--call", type=int, default=256)
ap.add_argument("--warmup", type=int, default=256)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(16, seed=0)
N = len(numbers)
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
mass = np.array([MASS[int(z)] for z in numbers])
T, FRICTION = 300.0, 0.02
vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
fetch_s = []


def begin(nh=False):
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=0.0 if nh else FRICTION, kT=kB * T, seed=0 if nh else 7,
                 ttime=25.0 * FS if nh else None)


def loop(steps, every=0, nh=False):
    begin(nh)
    mdl.md_run(8, None)
    if every:
        mdl.md_record(every)
    done, fetch = 0, 0.0
    t0 = time.perf_counter()
    while done < steps:
        sc, code = mdl.md_run(min(args.call, steps - done), None)
        if code or not len(sc):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
        done += len(sc)
        if every:
            t1 = time.perf_counter()
            fr = mdl.md_frames(closed=False, reuse=True)
            fetch += time.perf_counter() - t1
            assert len(fr["index"]) >= len(sc) // every
    if every == 1:
        fetch_s.append(1e6 * fetch / done)
    return (time.perf_counter() - t0) / done


def cut(steps):
    begin()
    mdl.md_run(8, None)
    t0 = time.perf_counter()
    for _ in range(steps):
        sc, code = mdl.md_run(1, None)
        if code:
            raise RuntimeError(f"the device loop stopped with code {code}")
        mdl.md_state(which=-1)
    return (time.perf_counter() - t0) / steps


paths = {"a_loop": lambda s: loop(s), "b_record_every_step": lambda s: loop(s, 1), "c_record_every_tenth": lambda s: loop(s, 10),
         "d_cut_per_step": cut, "e_nose_hoover_loop": lambda s: loop(s, 0, True)}
for f in paths.values():
    f(args.warmup)
fetch_s.clear()
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.steps))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, rounds=args.rounds, steps=args.steps, call=args.call,
                      us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(v, 2) for k, v in med.items()},
                      record_minus_loop_us=[round(b - a, 2) for a, b in zip(times["a_loop"], times["b_record_every_step"])],
                      nose_hoover_minus_loop_us=[round(e - a, 2) for a, e in zip(times["a_loop"], times["e_nose_hoover_loop"])],
                      fetch_us_per_step_in_b=[round(t, 2) for t in fetch_s],
                      b_below_d_every_round=bool(all(b < d for b, d in zip(times["b_record_every_step"], times["d_cut_per_step"]))))))
mdl.close()
