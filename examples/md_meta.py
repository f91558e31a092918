#!/usr/bin/env python3
"""Metadynamics with on-the-fly SGPR learning on the MI355X, after the reference's examples/meta-dyn/md.py: a Meta potential
is handed to ActiveCalculator(meta=...) and a hill is deposited per configuration.

    python examples/md_meta.py --side 6 6 6 --steps 400 --sigma 0.1 --w 0.01 [--tem 2000] [--thermostat nose-hoover]

* collective variables: the position of atom 0 relative to the mean of the other atoms of its species (Posvar) and its distance
  from atom 1 (Distance), concatenated (Catvar) — built in, as is the Steinhardt Qlvar (a commented variant below), so the bias runs inside the device loop (ActiveCalculator.run_md ->
  SGPRModel.md_meta: one small launch per step, no crossing into the host).  A colvar of your own, a function
  (numbers, xyz, cell, pbc, nl) -> 1-d torch tensor as in the reference, works too: the run then takes the host loop around
  calculate(), where the bias is added to energy, forces and stress;
* the reference attaches meta.update to its ASE dynamics; here run_md deposits per configuration on either path and writes
  meta.hist in the reference's format (a header `# sigma`, one line of CV values per deposit);
* merge=1024: the hills are merged by bin, 1024 at a time, as the reference's Gaussian_kde counts them — the cost of the bias
  grows with the bins the walk has visited, not with the length of the run (meta.histogram() returns the bins and their counts);
* teacher, system and integrator: those of examples/md_nvt_otf.py.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from md_nvt_otf import MASS, PairTeacher, rocksalt  # noqa: E402

from autoforce_amd.ase_shim import Atoms, kB  # noqa: E402
from autoforce_amd.calculator import ActiveCalculator  # noqa: E402
from autoforce_amd.meta import Catvar, Distance, Meta, Posvar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, nargs=3, default=[6, 6, 6], help="lattice sites per direction (even numbers)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=600.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--sigma", type=float, default=0.1, help="band width of the deposited Gaussians (A)")
    ap.add_argument("--w", type=float, default=0.01, help="their height (eV)")
    ap.add_argument("--tem", type=float, default=None, help="well-tempered metadynamics at this temperature (K)")
    ap.add_argument("--out", default="md_meta_out")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    species = [3, 9]
    numbers, pos, cell, pbc = rocksalt(args.side, species=species)
    N = len(numbers)
    meta = Meta(Catvar(Posvar(0, select=int(numbers[0])), Distance(0, 1)), sigma=args.sigma, w=args.w, tem=args.tem,
                hist=f"{args.out}/meta.hist", merge=1024)
    # The Steinhardt Q6 of atom 0 over its neighbours of the other species inside 4 A — the reference's Qlvar, the colvar of melting
    # and nucleation — runs inside the device loop too (cutoff <= the model's cutoff; sigma of order 0.01: Q6 lives in [0, 1]):
    # from autoforce_amd.meta import Qlvar
    # meta = Meta(Qlvar(int(numbers[0]), int(numbers[1]), index=0, cutoff=4.0, l=[6]), sigma=0.01, w=args.w, tem=args.tem,
    #             hist=f"{args.out}/meta.hist", merge=1024)
    teacher = PairTeacher(species)
    calc = ActiveCalculator(calculator=teacher, kernel_kw=dict(species=species), meta=meta, logfile=f"{args.out}/active.log",   # <- meta
                            tape=None, pckl=None, ediff=0.086, fdiff=0.129)
    np.random.seed(1)
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * args.temperature / mass)
    vel -= (mass * vel).sum(0) / mass.sum()
    at = Atoms(numbers, pos, cell, pbc, velocities=vel, masses=mass[:, 0])
    kw = dict(tdamp_fs=25.0) if args.thermostat == "nose-hoover" else dict(friction=1e-3, seed=1)
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=64, **kw):
        if step % 20 == 0 or updated:
            print(f"{step:5d} E={E:14.6f} T={T:7.1f} size={calc.size} hills={len(meta.hills)} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; "
          f"{len(meta.hills)} hills in {args.out}/meta.hist; final model {calc.size}")


if __name__ == "__main__":
    main()
