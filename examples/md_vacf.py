#!/usr/bin/env python3
"""Vibrational density of states and Green-Kubo diffusivity of a small lithium thiophosphate frame with on-the-fly SGPR learning on
the MI355X: the velocity autocorrelations are accumulated INSIDE the device loop (ActiveCalculator.run_md(vacf=...) ->
SGPRModel.md_vacf: a store and a correlation behind a sampled step, no velocity leaves the device) and read once at the end.  The
mean-square displacements of the SAME run are accumulated beside them (msd=...), so the Green-Kubo D stands next to the Einstein one.

    python examples/md_vacf.py --side 8 --steps 4000 --every 2 --lags 256 [--origin-every 4] [--temperature 900] [--thermostat nose-hoover]

* `every`: steps between samples — the highest frequency resolved is 1 / (2 every dt); `lags`: the correlation is kept up to
  (lags - 1) every dt, which sets the frequency resolution 1 / (2 lags every dt); `origin_every`: every how many samples a new time
  origin is taken (1: all of them; more: cheaper, noisier);
* com: velocities are taken relative to the frame's centre of mass (a Langevin thermostat does not conserve momentum);
* the holder adds up the tables of several runs: call run_md again with the same holder to improve the statistics;
* the last sample of a run is pending — it is correlated when the next one arrives —, so a run of S samples counts S - 1;
* D_GK = (1/3) int C(t) dt against D_t, the slope / 6 of the msd; the Onsager block L_ab of the species' currents;
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
from autoforce_amd.transport import Msd, Vacf, diffusion_constants, green_kubo, onsager, vibrational_dos  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=2, help="steps between samples")
    ap.add_argument("--lags", type=int, default=256, help="lags of 0 ... lags - 1 samples")
    ap.add_argument("--origin-every", type=int, default=1, help="samples between time origins")
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--out", default="md_vacf_out")
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
    vacf = Vacf(args.every, args.lags, args.origin_every, com=True)                                         # <- the holders
    msd = Msd(max(1, args.every), 8, com=True)
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, vacf=vacf, msd=msd, **kw):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}; "
          f"{vacf.samples} samples correlated")
    f, dos = vibrational_dos(vacf, args.dt)
    np.savetxt(f"{args.out}/dos.dat", np.column_stack([f] + [dos[z] for z in sorted(dos)]), header="f (THz)  " + "  ".join(f"Z={z}" for z in sorted(dos)))
    for z in sorted(dos):
        print(f"# Z = {z:2d}: the density of states peaks at {f[int(np.argmax(dos[z]))]:7.2f} THz (resolution {f[1]:.2f} THz; {args.out}/dos.dat)")
    to_cm2_s = 1e-16 / 1e-15   # A^2 / fs -> cm^2 / s
    gk = green_kubo(vacf, args.dt)
    try:
        ein = diffusion_constants(msd, args.dt)
    except ValueError:   # (a run too short for two lags with two windows)
        ein = {}
    for z in sorted(gk):
        line = f"# Z = {z:2d}: D_GK({gk[z]['t'][-1]:.0f} fs) = {gk[z]['value'] * to_cm2_s:.3e} cm^2/s"
        if z in ein:
            line += "   D_t (Einstein) = {:.3e} ({:.3e} ... {:.3e}) cm^2/s".format(*(d * to_cm2_s for d in ein[z]["Dt"]))
        print(line)
    t, L = onsager(vacf, args.dt)
    present = [k for k, n in enumerate(vacf.n) if n > 0]
    print(f"# Onsager block L_ab({t[-1]:.0f} fs), cm^2/s, species {[int(vacf.species[k]) for k in present]}:")
    for a in present:
        print("#   " + "  ".join(f"{L[-1, a, b] * to_cm2_s:11.3e}" for b in present))
    print("# (a run this short measures mostly vibration: the integrals are diffusivities once C(t) has decayed within the lags kept)")


if __name__ == "__main__":
    main()
