#!/usr/bin/env python3
"""Wall time per evaluation of a ring polymer of P beads on LiPS 512 atoms / 512 inducing (fp64), taken in ONE process: (a) the
polymer inside the device loop (sgpr_md_pimd: P plain steps and three small launches per evaluation, deviates drawn on the
device, the host reads sixteen scalars per evaluation), (b) the path such a run had before — the host twin workloads.pimd_baoab
around the calculator surface, one synchronised predict per bead per evaluation and numpy in between —, (c) P times the step of
the plain Langevin device loop on that frame (md_begin + md_run: what P independent replicas cost; (a) - (c) is the price of the
three launches and of every bead rebuilding its lists) and (d) a nudged elastic band of K = P interior images in the device loop
for scale (its three launches behind the same P plain steps).  The model is fitted to the pair teacher, so the polymer holds
together.  Every path is warmed up first; then they alternate in `--rounds` rounds of `--evals` evaluations, every window starting
from the same polymer and closed by a device synchronise.  Prints one JSON line per P: the median and the spread (max - min over
the rounds) of the microseconds per evaluation of each path.

    python tools/pimd_step_time.py [--beads 8 16] [--rounds 5] [--evals 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.ase_shim import kB
from autoforce_amd.workloads import FS, MASS, fit_to_teacher, lips, pimd_baoab

ap = argparse.ArgumentParser()
ap.add_argument("--beads", type=int, nargs="+", default=[8, 16])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--evals", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()

T, DT_FS, FRICTION, LAMBDA = 300.0, 1.0, 1e-2, 0.5
numbers, pos, cell, pbc = lips(8, seed=0)
N = len(numbers)
mass = np.array([MASS[int(z)] for z in numbers])
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512, workload_seed=1)
fit_to_teacher(mdl, numbers, pos, cell, pbc)


class PredictCalc:
    """The library behind the getters of the twin: one synchronised predict per bead."""
    implemented_properties = ["energy", "forces"]

    def __init__(self):
        self._key, self.results, self.beta = None, {}, None

    def get_property(self, name, atoms=None):
        key = atoms.positions.tobytes()
        if key != self._key:
            out = mdl.predict(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc)
            self.results, self.beta, self._key = dict(energy=float(out["energy"]), forces=out["forces"]), out["beta"], key
        return self.results[name]

    def get_covloss(self):
        return self.beta


def run_through(evals):
    """`evals` evaluations of the run that has just begun, four unmeasured ones first; seconds per evaluation."""
    sc, code = mdl.md_run(4, None)
    assert code == 0, code
    done = 0
    t0 = time.perf_counter()
    while done < evals:
        sc, code = mdl.md_run(evals - done, None)
        done += len(sc)
        if code == 1 or (code and not len(sc)):
            raise RuntimeError(f"the device loop stopped with code {code} after {done} evaluations")
    dt = (time.perf_counter() - t0) / done
    mdl.md_end()
    return dt


def measure(P):
    rng = np.random.default_rng(5)
    beads = pos[None] + 0.02 * rng.normal(size=(P, N, 3))
    vel = rng.normal(size=(P, N, 3)) * np.sqrt(P * kB * T / mass)[None, :, None]
    band = np.concatenate([pos[None], beads[:min(P, 16)], pos[None]])

    def device(evals):
        mdl.pimd_begin(numbers, beads, cell, pbc, mass, vel, dt=DT_FS * FS, kT=kB * T, friction=FRICTION, pile_lambda=LAMBDA, seed=7)
        return run_through(evals)

    def host(evals):
        it = pimd_baoab(PredictCalc(), numbers, beads, cell, pbc, evals + 4, temperature=T, dt_fs=DT_FS, friction=FRICTION, pile_lambda=LAMBDA, vel=vel,
                        species=mdl.species, masses=mass)
        for _ in range(5):
            next(it)
        t0 = time.perf_counter()
        for _ in it:                # (every bead's evaluation ends in predict's own synchronise)
            pass
        return (time.perf_counter() - t0) / evals

    def langevin(evals):            # (P times the step of one replica)
        mdl.md_begin(numbers, beads[0], cell, pbc, mass, vel[0] / np.sqrt(P), dt=DT_FS * FS, friction=FRICTION, kT=kB * T, seed=7)
        return P * run_through(evals)

    def neb(evals):
        mdl.neb_begin(numbers, band, cell, pbc, 1e-9)
        return run_through(evals)

    paths = {"device_loop": device, "host_twin": host, "P_langevin_steps": langevin, "neb_device_loop": neb}
    for f in paths.values():
        f(args.warmup)
    times = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, f in paths.items():
            times[k].append(1e6 * f(args.evals))
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps(dict(atoms=N, inducing=512, beads=P, neb_images=min(P, 16), rounds=args.rounds, evals=args.evals,
                          us_per_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
                          median_us={k: round(med[k], 2) for k in paths},
                          spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
                          host_over_device=round(med["host_twin"] / med["device_loop"], 3),
                          device_minus_P_langevin_us=round(med["device_loop"] - med["P_langevin_steps"], 2),
                          neb_minus_P_langevin_us=round(med["neb_device_loop"] - med["P_langevin_steps"], 2))), flush=True)


for P in args.beads:
    measure(P)
mdl.close()
