#!/usr/bin/env python3
"""Bond angles and coordination of a small lithium thiophosphate frame with on-the-fly SGPR learning on the MI355X: the angles
between the bonds of every centre and its numbers of neighbours are counted INSIDE the device loop
(ActiveCalculator.run_md(adf=...) -> SGPRModel.md_adf: a pass over the step's own neighbour list behind a sampled step, no
trajectory leaves the device) and read once at the end — are the PS4 tetrahedra intact (S-P-S near 109.5 degrees), do they share
corners or edges (P-S-P), and how many S sit around a Li.

    python examples/md_adf.py --side 8 --steps 2000 --every 10 --bins 180 [--ps 2.6] [--lis 3.0] [--temperature 900]

* `every`: steps between samples; the bond cutoffs (--ps: P-S, --lis: Li-S; the other pairs never bond) must not exceed the
  model's cutoff; the counts are integers, the same however the run is cut or halted by a model update;
* the holder adds up the tables of several runs: call run_md again with the same holder to improve the statistics;
* angle_distribution(holder, centre, ends) returns P(theta) normalised to unit area (solid_angle=True divides by sin theta
  first); coordination(holder, centre, neighbour) the distribution of the number of neighbours and its mean;
* the frame is workloads.lips' rattled lattice, not a crystal structure: expect the angles of a simple-cubic lattice;
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
from autoforce_amd.transport import Adf, angle_distribution, coordination  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=10, help="steps between samples")
    ap.add_argument("--bins", type=int, default=180)
    ap.add_argument("--ps", type=float, default=2.6, help="P-S bond cutoff, A")
    ap.add_argument("--lis", type=float, default=3.0, help="Li-S bond cutoff, A")
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--out", default="md_adf_out")
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
    adf = Adf(args.every, args.bins, {(15, 16): args.ps, (3, 16): args.lis})                                # <- the holder
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, adf=adf, **kw):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}; "
          f"{adf.samples} samples, {int(adf.angles.sum())} angles")
    out = {}
    for name, centre, ends in (("S-P-S", 15, (16, 16)), ("P-S-P", 16, (15, 15)), ("S-Li-S", 3, (16, 16))):
        try:
            th, P = angle_distribution(adf, centre, ends)
        except ValueError:
            print(f"# {name}: no angle within the cutoffs")
            continue
        out[name] = P
        out["theta"] = th
        print(f"# {name}: most likely {th[int(np.argmax(P))]:6.1f} degrees, mean {np.sum(th * P) * 180.0 / args.bins:6.1f}")
    for name, centre, nb in (("S around Li", 3, 16), ("S around P", 15, 16), ("P around S", 16, 15)):
        n, P, mean = coordination(adf, centre, nb)
        print(f"# {name}: mean {mean:5.2f}, most likely {int(np.argmax(P))}, P(n) = " + " ".join(f"{n_}:{p:.3f}" for n_, p in zip(n, P) if p > 0.0005))
    np.savez(f"{args.out}/adf.npz", angles=adf.angles, coord=adf.coord, species=adf.species, n=adf.n, cut=adf.cut, **out)
    print(f"# written {args.out}/adf.npz")


if __name__ == "__main__":
    main()
