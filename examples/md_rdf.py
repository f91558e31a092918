#!/usr/bin/env python3
"""Radial distribution functions of a small lithium thiophosphate frame with on-the-fly SGPR learning on the MI355X: the pair
distances are counted INSIDE the device loop (ActiveCalculator.run_md(rdf=...) -> SGPRModel.md_rdf: a pair sweep behind a sampled
step, no trajectory leaves the device) and read once at the end — what the reference gets from a stored trajectory with
theforce/analysis/rdf.py (`rdf`).

    python examples/md_rdf.py --side 8 --steps 2000 --every 10 --rmax 8 --bins 160 [--temperature 900] [--thermostat nose-hoover]

* `every`: steps between samples; `rmax` may exceed the model's cutoff and half the cell (periodic images are enumerated, up to
  two cells either way); the counts are integers, the same however the run is cut or halted by a model update;
* the holder adds up the tables of several runs: call run_md again with the same holder to improve the statistics;
* radial_distribution(holder) returns the reference's axis and normalisation (its bin spacing (rmax - rmin) / (bins - 1));
  shells=True uses the true bins and shell volumes — printed here, with the first peak of every pair;
* teacher and integrator: those of examples/md_nvt_otf.py.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from md_nvt_otf import MASS, PairTeacher  # noqa: E402

from autoforce_amd.ase_shim import Atoms, kB  # noqa: E402
from autoforce_amd.calculator import ActiveCalculator  # noqa: E402
from autoforce_amd.transport import Rdf, radial_distribution  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=10, help="steps between samples")
    ap.add_argument("--rmax", type=float, default=8.0)
    ap.add_argument("--bins", type=int, default=160)
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--out", default="md_rdf_out")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    numbers, pos, cell, pbc = lips(args.side, seed=0)
    species = sorted(set(int(z) for z in numbers))
    N = len(numbers)
    calc = ActiveCalculator(calculator=PairTeacher(species), kernel_kw=dict(species=species), logfile=f"{args.out}/active.log",
                            tape=None, pckl=None, ediff=0.086, fdiff=0.129)
    np.random.seed(1)
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * args.temperature / mass)
    vel -= (mass * vel).sum(0) / mass.sum()
    at = Atoms(numbers, pos, cell, pbc, velocities=vel, masses=mass[:, 0])
    kw = dict(tdamp_fs=25.0) if args.thermostat == "nose-hoover" else dict(friction=1e-3, seed=1)
    rdf = Rdf(args.every, args.rmax, args.bins)                                                             # <- the holder
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, rdf=rdf, **kw):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}; "
          f"{rdf.samples} samples, {int(rdf.hist.sum())} pair distances below {args.rmax} A")
    r, g = radial_distribution(rdf, shells=True)
    np.savez(f"{args.out}/rdf.npz", r=r, pairs=np.array(list(g)), g=np.stack(list(g.values())), hist=rdf.hist, species=rdf.species, n=rdf.n)
    for (za, zb), gab in g.items():
        k = int(np.argmax(gab))
        print(f"# g({za:2d},{zb:2d}): first maximum {gab[k]:7.3f} at r = {r[k]:5.2f} A; mean over the last A: {gab[r > args.rmax - 1.0].mean():5.3f}")
    print(f"# written {args.out}/rdf.npz")


if __name__ == "__main__":
    main()
