#!/usr/bin/env python3
"""Lithium diffusivity of a small lithium thiophosphate frame with on-the-fly SGPR learning on the MI355X: the mean-square
displacements are accumulated INSIDE the device loop (ActiveCalculator.run_md(msd=...) -> SGPRModel.md_msd: two small launches
behind a sampled step, no trajectory leaves the device) and read once at the end — what the reference gets from a stored
trajectory with theforce/analysis/analysis.py (`displacements`, `diffusion_constants`).

    python examples/md_msd.py --side 8 --steps 4000 --every 4 --levels 8 [--temperature 900] [--thermostat nose-hoover]

* `every`: steps between samples; `levels`: lags of 1, 2, 4, ... 2^(levels - 1) samples, each with its own origin and windows
  that do not overlap — so the scatter of a level's windows is an honest error bar;
* com: displacements are taken relative to the frame's centre of mass (a Langevin thermostat does not conserve momentum);
* the holder adds up the tables of several runs: call run_md again with the same holder to improve the statistics;
* D_t (tracer) and D_j (collective, "charge") are slopes / 6 of msd and smd against time, with the bounds the reference's
  get_slopes forms; their ratio is the Haven ratio;
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
from autoforce_amd.transport import Msd, diffusion_constants  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=4, help="steps between samples")
    ap.add_argument("--levels", type=int, default=8, help="lags of 2^l samples, l < levels")
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--out", default="md_msd_out")
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
    msd = Msd(args.every, args.levels, com=True)                                                            # <- the holder
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, msd=msd, **kw):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}")
    mean, err = msd.mean(), msd.stderr()
    k = list(msd.species).index(3)
    print("# lithium:  lag (fs)   windows   msd (A^2)   +/-        smd (A^2)   +/-")
    for l, lag in enumerate(msd.lags):
        print(f"          {lag * args.dt:9.1f} {msd.count[l]:9d} {mean['msd'][l, k]:11.5f} {err['msd'][l, k]:10.5f} {mean['smd'][l, k]:11.5f} {err['smd'][l, k]:10.5f}")
    D = diffusion_constants(msd, args.dt)[3]
    to_cm2_s = 1e-16 / 1e-15   # A^2 / fs -> cm^2 / s
    print("# D_t = {:.3e} ({:.3e} ... {:.3e}) cm^2/s".format(*(d * to_cm2_s for d in D["Dt"])))
    print("# D_j = {:.3e} ({:.3e} ... {:.3e}) cm^2/s".format(*(d * to_cm2_s for d in D["Dj"])))
    print("# (a run this short measures mostly vibration: the slope is a diffusivity once the msd passes a few A^2)")


if __name__ == "__main__":
    main()
