#!/usr/bin/env python3
"""Van Hove correlation functions of a small lithium thiophosphate frame with on-the-fly SGPR learning on the MI355X — does Li
move by hops or by flow? — counted INSIDE the device loop (ActiveCalculator.run_md(vanhove=...) -> SGPRModel.md_vanhove: at most
three launches behind a sampled step, no trajectory leaves the device) and read once at the end.  The self part is what the
reference gets from a stored trajectory with theforce/analysis/analysis.py (`TrajAnalyser.hist_rtp_displacements`), at every lag
2^l samples at once; the distinct part (where the other atoms are around the place an atom left) the reference does not have.

    python examples/md_vanhove.py --side 8 --steps 4096 --every 4 --levels 8 --rmax 4 --rbins 80 [--tbins 6 --pbins 8]
                                  [--dmax 6 --dbins 120] [--temperature 900] [--thermostat nose-hoover]

* `every`: steps between samples; level l has the lag 2^l samples, one origin and windows that do not overlap;
* displacements are raw (no centre of mass is taken out) and those of rmax and more are counted apart (`over`): choose rmax so
  that it stays empty for the lags you read;
* `dmax` may exceed half the cell (periodic images are enumerated, up to two cells either way); --dbins 0 leaves the distinct
  part, which costs a pair sweep per due level, out;
* all entries are integer counts, the same however the run is cut or halted by a model update; the holder adds up the tables
  of several runs;
* printed per species and lag: the non-Gaussian parameter alpha_2 (0 for flow, positive for hops; BINNED, see
  transport.non_gaussian), the most probable displacement, the fraction beyond a hop length, and for the mobile species the
  height of G_d(r -> 0) / rho: other atoms arriving at the place an atom left;
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
from autoforce_amd.transport import VanHove, displacement_histogram, distinct_van_hove, non_gaussian, self_van_hove  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--every", type=int, default=4, help="steps between samples")
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--rmax", type=float, default=4.0)
    ap.add_argument("--rbins", type=int, default=80)
    ap.add_argument("--tbins", type=int, default=6)
    ap.add_argument("--pbins", type=int, default=8)
    ap.add_argument("--dmax", type=float, default=6.0)
    ap.add_argument("--dbins", type=int, default=120)
    ap.add_argument("--hop", type=float, default=1.5, help="Angstrom: displacements beyond it count as hops")
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--thermostat", choices=["langevin", "nose-hoover"], default="langevin")
    ap.add_argument("--out", default="md_vanhove_out")
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
    vh = VanHove(args.every, args.levels, args.rmax, args.rbins, args.tbins, args.pbins, args.dmax, args.dbins)   # <- the holder
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, vanhove=vh, **kw):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}; "
          f"{vh.samples} samples, windows per level {vh.count.tolist()}, beyond rmax per level {vh.over.sum(axis=1).tolist()}")
    r, Gs = self_van_hove(vh)
    a2 = non_gaussian(vh)
    out = dict(r=r, lags=vh.lags, count=vh.count, species=vh.species, n=vh.n, self_hist=vh.hist, over=vh.over,
               Gs=np.stack([Gs[int(z)] for z in vh.species if int(z) in Gs]), alpha2=np.stack([a2[int(z)] for z in vh.species if int(z) in a2]))
    if args.dbins:
        rd, Gd = distinct_van_hove(vh)
        out.update(rd=rd, pairs=np.array(list(Gd)), Gd=np.stack(list(Gd.values())), distinct_hist=vh.distinct)
    np.savez(f"{args.out}/vanhove.npz", **out)
    for z in Gs:
        for l in range(vh.levels):
            if vh.count[l] == 0:
                continue
            P = Gs[z][l] * 4 * np.pi * r ** 2 * (args.rmax / args.rbins)
            line = (f"# Z={z:2d} lag {int(vh.lags[l] * args.dt):6d} fs ({int(vh.count[l]):4d} windows): alpha_2 = {a2[z][l]:6.3f}, most probable |d| = "
                    f"{r[int(np.argmax(P))]:5.2f} A, beyond {args.hop} A: {P[r > args.hop].sum():6.4f}")
            if args.dbins and z == species[0]:
                line += f", G_d({z},{z})(r < 1 A) / rho = {Gd[(z, z)][l][rd < 1.0].mean():6.3f}"
            print(line)
    if args.tbins > 1 or args.pbins > 1:   # (the reference's own return for one lag, as its hist_rtp_displacements gives it)
        l = int(np.flatnonzero(vh.count > 0)[-1])
        rr, tt, pp, h, rho = displacement_histogram(vh, l, species[0])
        k = np.unravel_index(int(np.argmax(h)), h.shape)
        print(f"# Z={species[0]} lag {int(vh.lags[l] * args.dt)} fs: fullest (r, theta, phi) bin at ({rr[k[0]]:.2f} A, {tt[k[1]]:.2f}, {pp[k[2]]:.2f}) holds {h[k]:.4f}; rho = {rho:.5f} / A^3")
    print(f"# written {args.out}/vanhove.npz")


if __name__ == "__main__":
    main()
