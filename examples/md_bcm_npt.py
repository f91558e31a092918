#!/usr/bin/env python3
"""NPT molecular dynamics with a Bayesian committee on the MI355X: a BCMActiveCalculator with one frozen member and a live
model that keeps learning, under the Nose-Hoover / Parrinello-Rahman barostat, all of it inside the device loop.

    python examples/md_bcm_npt.py --side 7 --steps 40

* a first model learns a rattled LiPS-like frame from a stand-in teacher (a smooth pair potential in numpy; a real run passes
  any ASE calculator) and is frozen as a member (initiate_bcm); a fresh live model takes over;
* run_md(tdamp_fs=, pfactor=, externalstress=) then integrates the committee's weighted forces in a cell that follows the
  committee's stress — pfactor = ptime^2 x bulk modulus —, halts where the committee's covloss asks for sampling, lets
  calculate() update the live model, and goes on (SGPRModel.md_begin(pfactor=) + md_committee(moving_cell=True) on the device);
* every `--sync` steps atoms.positions and atoms.cell are current, and the script prints the volume.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autoforce_amd import SGPRModel  # noqa: E402
from autoforce_amd.ase_shim import Atoms, kB  # noqa: E402
from autoforce_amd.calculator_bcm import BCMActiveCalculator  # noqa: E402
from autoforce_amd.npt import GPA  # noqa: E402
from autoforce_amd.workloads import FS, MASS, PairTeacher, lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=7, help="lattice sites per edge (7 -> 343 atoms)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--temperature", type=float, default=600.0)
    ap.add_argument("--tdamp", type=float, default=25.0, help="thermostat time, fs")
    ap.add_argument("--ptime", type=float, default=100.0, help="barostat time, fs")
    ap.add_argument("--bulk-modulus", type=float, default=30.0, help="GPa")
    ap.add_argument("--pressure", type=float, default=1.0, help="external pressure, GPa")
    ap.add_argument("--ediff", type=float, default=0.06)
    ap.add_argument("--sync", type=int, default=10)
    args = ap.parse_args()

    numbers, pos, cell, pbc = lips(args.side, seed=0)
    species = sorted(set(int(z) for z in numbers))
    np.random.seed(1)
    calc = BCMActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=species), calculator=PairTeacher(species, rc=4.0, eps=0.4, a=1.3, r0=2.6), logfile=None, pckl=None,
                               tape=None, ediff=args.ediff, ediff_tot=2 * args.ediff, fdiff=2 * args.ediff, noise_f=0.02)
    # the first model: seeded from another frame of the same lattice, then frozen as a member
    n1, p1, c1, b1 = lips(args.side, seed=1)
    first = Atoms(n1, p1, c1, b1)
    first.calc = calc
    first.get_forces()
    calc.initiate_bcm()
    print(f"# {len(numbers)} atoms; frozen members: {len(calc.model_dict)}; the live model starts empty")

    mass = np.array([MASS[int(z)] for z in numbers])
    rng = np.random.default_rng(2)
    vel = rng.normal(size=(len(numbers), 3)) * np.sqrt(kB * args.temperature / mass)[:, None]
    vel -= (mass[:, None] * vel).sum(0) / mass.sum()
    atoms = Atoms(numbers, pos, cell, pbc, velocities=vel)
    pfactor = (args.ptime * FS) ** 2 * args.bulk_modulus * GPA
    print(f"# committee on the device loop: {calc.md_on_device_ok()}")
    for step, E, T, updated, wall in calc.run_md(atoms, args.steps, args.temperature, dt_fs=1.0, tdamp_fs=args.tdamp, pfactor=pfactor,
                                                 externalstress=args.pressure * GPA, sync_every=args.sync):
        note = "  model updated" if updated else ""
        if step % args.sync == 0:
            vol = abs(np.linalg.det(np.asarray(getattr(atoms.cell, "array", atoms.cell), float)))
            note += f"  V = {vol:.3f} A^3"
        print(f"{step:5d} E = {E:14.6f} eV  T = {T:7.1f} K  live model {calc.size}{note}", flush=True)
    print("# weights of the last evaluation:", {k: round(w, 4) for k, w in calc.bcm_weights.items()})


if __name__ == "__main__":
    main()
