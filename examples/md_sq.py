#!/usr/bin/env python3
"""Static structure factors and coherent intermediate scattering functions of a small lithium thiophosphate frame with on-the-fly
SGPR learning on the MI355X: the species' densities rho_z(q) at the wave vectors of a half-sphere of the cell's reciprocal lattice
are formed and correlated INSIDE the device loop (ActiveCalculator.run_md(sq=...) -> SGPRModel.md_sq: three launches behind a
sampled step, no position leaves the device) and the tables are read once at the end.

    python examples/md_sq.py --side 8 --steps 4000 --qmax 3.0 --every 4 --lags 64 [--origin-every 4] [--temperature 900]

* `qmax` (1 / Angstrom): every vector of the reciprocal lattice up to it, one of each +- pair (transport.q_vectors); the smallest
  |q| a cell of side L holds is 2 pi / L — the long-wavelength limit needs a large cell, not a small qmax;
* `every`: steps between samples; `lags`: F(q, t) is kept up to (lags - 1) every dt; lags = 1 is the static S(q) alone and by far
  the cheapest (per sample lags nq S^2 sums are updated); `origin_every`: every how many samples a new time origin is taken;
* S_ab(q): Ashcroft-Langreth partials averaged over shells of equal |q|; `--weights` (Z=b ...): a weighted total, e.g. neutron
  scattering lengths; the Bragg part |<rho>|^2 is split off (diffuse=True) — in a crystal it carries almost everything;
* the holder adds up the tables of several runs: call run_md again with the same holder to improve the statistics;
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
from autoforce_amd.transport import Sq, dynamic_structure_factor, intermediate_scattering, q_vectors, structure_factor  # noqa: E402
from autoforce_amd.workloads import lips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8, help="lattice sites per direction (8: 512 atoms, 192 Li / 64 P / 256 S)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--qmax", type=float, default=3.0, help="1 / Angstrom")
    ap.add_argument("--every", type=int, default=4, help="steps between samples")
    ap.add_argument("--lags", type=int, default=64, help="lags of 0 ... lags - 1 samples (1: the static S(q) alone)")
    ap.add_argument("--origin-every", type=int, default=1, help="samples between time origins")
    ap.add_argument("--weights", nargs="*", default=["3=-1.90", "15=5.13", "16=2.847"], help="Z=b: weights of the total (neutron lengths, fm)")
    ap.add_argument("--temperature", type=float, default=900.0)
    ap.add_argument("--dt", type=float, default=1.0, help="fs")
    ap.add_argument("--out", default="md_sq_out")
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
    hkl = q_vectors(cell, args.qmax)                                                                        # <- the wave vectors
    sq = Sq(args.every, hkl, args.lags, args.origin_every)                                                  # <- the holder
    print(f"# {len(hkl)} wave vectors up to {args.qmax} / A (largest index {np.abs(hkl).max()}), {args.lags} lags of {args.every} steps")
    t0 = time.time()
    for step, E, T, updated, wall in calc.run_md(at, args.steps, args.temperature, dt_fs=args.dt, chunk=256, friction=1e-3, seed=1, sq=sq):
        if step % 200 == 0 or updated:
            print(f"{step:6d} E={E:14.6f} T={T:7.1f} size={calc.size} wall={wall * 1e3:8.2f} ms", flush=True)
    print(f"# {args.steps} steps in {time.time() - t0:.1f} s on the {'device' if calc.md_on_device_ok() else 'host'} loop; final model {calc.size}; "
          f"{sq.samples} samples")
    present = [k for k, n in enumerate(sq.n) if n > 0]
    names = [f"S_{int(sq.species[a])}_{int(sq.species[b])}" for a in present for b in present if a <= b]
    q, S = structure_factor(sq)
    _, Sd = structure_factor(sq, diffuse=True)
    weights = {int(w.split("=")[0]): float(w.split("=")[1]) for w in args.weights}
    _, tot = structure_factor(sq, weights=weights)
    _, tot_d = structure_factor(sq, weights=weights, diffuse=True)
    cols = [q, tot, tot_d] + [S[:, a, b] for a in present for b in present if a <= b] + [Sd[:, a, b] for a in present for b in present if a <= b]
    np.savetxt(f"{args.out}/sq.dat", np.column_stack(cols),
               header="|q| (1/A)  S_total  S_total_diffuse  " + "  ".join(names) + "  " + "  ".join(n + "_diffuse" for n in names))
    k = int(np.argmax(tot))
    print(f"# the weighted total peaks at |q| = {q[k]:.3f} / A: S = {tot[k]:.2f}, of which diffuse {tot_d[k]:.2f} ({args.out}/sq.dat)")
    if args.lags > 1:
        qs, t, F, Fn = intermediate_scattering(sq)
        li = present[0]
        np.savetxt(f"{args.out}/fqt_{int(sq.species[li])}.dat", np.column_stack([t * args.dt] + [Fn[:, j, li, li] for j in range(len(qs))]),
                   header="t (fs)  F(q, t) / F(q, 0) of species {} at |q| = ".format(int(sq.species[li])) + "  ".join(f"{v:.3f}" for v in qs))
        half = [int(np.argmax(Fn[:, j, li, li] < 0.5)) for j in range(len(qs))]
        j = int(np.argmin(qs))
        print(f"# F_{int(sq.species[li])}{int(sq.species[li])}(q, t) / F(q, 0) at the smallest |q| = {qs[j]:.3f} / A "
              + (f"falls below 1/2 after {t[half[j]] * args.dt:.0f} fs" if half[j] else f"stays above 1/2 over the {t[-1] * args.dt:.0f} fs kept"))
        try:
            f, _, Sw = dynamic_structure_factor(sq, args.dt)
            np.savetxt(f"{args.out}/sqw_{int(sq.species[li])}.dat", np.column_stack([f] + [Sw[:, j, li, li] for j in range(len(qs))]),
                       header="f (THz)  S(q, f) of species {} at |q| = ".format(int(sq.species[li])) + "  ".join(f"{v:.3f}" for v in qs))
            print(f"# S(q, f) up to {f[-1]:.1f} THz in steps of {f[1]:.2f} THz ({args.out}/sqw_{int(sq.species[li])}.dat)")
        except ValueError as e:   # (a run too short for two lags with samples)
            print(f"# no S(q, f): {e}")


if __name__ == "__main__":
    main()
