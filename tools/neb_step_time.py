#!/usr/bin/env python3
"""Wall time per evaluation of a nudged elastic band of K = 5 interior images on LiPS 512 atoms / 512 inducing (fp64), taken in
ONE process: (a) the band inside the device loop (sgpr_md_neb: K plain steps and three small launches per evaluation, the host
reads sixteen scalars per evaluation), (b) the path such a run had before — the host twin workloads.neb_fire around the
calculator surface, one synchronised predict per image per evaluation and numpy in between — and (c) K plain synchronised
predicts alone for scale (what (b) cannot go below).  The model is fitted to the pair teacher, so the band holds together.
Every path is warmed up first; then they alternate in `--rounds` rounds of `--evals` evaluations, every window starting from the
same band and closed by a device synchronise.  Prints one JSON line: the median and the spread (max - min over the rounds) of
the microseconds per band evaluation of each path and the ratio host / device.

    python tools/neb_step_time.py [--rounds 5] [--evals 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from autoforce_amd.workloads import fit_to_teacher, lips, neb_fire

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--evals", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--images", type=int, default=5)
args = ap.parse_args()

numbers, pos, cell, pbc = lips(8, seed=0)
N, K = len(numbers), args.images
mdl = bench.build_model(0, numbers, pos, cell, pbc, 512, workload_seed=1)
fit_to_teacher(mdl, numbers, pos, cell, pbc)
rng = np.random.default_rng(5)
end = pos + np.clip(0.08 * rng.normal(size=pos.shape), -0.2, 0.2)
images = np.array([pos + (i / (K + 1.0)) * (end - pos) for i in range(K + 2)])
FMAX = 1e-9   # (never reached: every window runs its full count)


class PredictCalc:
    """The library behind the getters of the twin: one synchronised predict per image."""
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


def device(evals):
    mdl.neb_begin(numbers, images, cell, pbc, FMAX, climb=True)
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


def host(evals):
    it = neb_fire(PredictCalc(), numbers, images, cell, pbc, evals + 4, FMAX, climb=True, species=mdl.species)
    for _ in range(5):
        next(it)
    t0 = time.perf_counter()
    for _ in it:                # (every image's evaluation ends in predict's own synchronise)
        pass
    return (time.perf_counter() - t0) / evals


def predicts(evals):
    t0 = time.perf_counter()
    for _ in range(evals):
        for i in range(K):
            mdl.predict(numbers, images[1 + i], cell, pbc)
    return (time.perf_counter() - t0) / evals


paths = {"device_loop": device, "host_twin": host, "predicts_alone": predicts}
for f in paths.values():
    f(args.warmup)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, f in paths.items():
        times[k].append(1e6 * f(args.evals))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(atoms=N, inducing=512, images=K, rounds=args.rounds, evals=args.evals,
                      us_per_band_evaluation={k: [round(t, 2) for t in v] for k, v in times.items()},
                      median_us={k: round(med[k], 2) for k in paths},
                      spread_us={k: round(float(np.ptp(v)), 2) for k, v in times.items()},
                      host_over_device=round(med["host_twin"] / med["device_loop"], 3),
                      predicts_over_device=round(med["predicts_alone"] / med["device_loop"], 3))))
mdl.close()
