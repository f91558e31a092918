"""Machine-learning accelerated relaxation from the command line — theforce/cl/relax.py in this package's terms:

    python -m autoforce_amd.cl.relax -i start.xyz -o relaxed.xyz      # keywords from ./ARGS

The reference minimises with an optimizer of `ase.optimize` (`algo = 'BFGS'` by default, cl/relax.py:50-54) around the
active calculator — the model learns on the way, `calculate()` being what it is inside MD — and then CONFIRMS the minimum
(cl/relax.py:59-70): as long as `update_data(try_fake=False)` accepts the exact labels of the current structure, the model
is updated and the relaxation continues from there.  With ASE installed this driver uses ASE's optimizers (and
`UnitCellFilter` for `cell = True`) exactly as the reference does.  ASE is a dependency of the reference, not part of it,
and is absent from the build image: without it two of its optimizers are restated here from their published algorithms
(ase/optimize/bfgs.py, ase/optimize/fire.py, ASE 3.22) — `BFGS` (dense Hessian, H0 = 70 eV/A^2, the step taken through the
eigen-decomposition with |omega|, the longest atomic step scaled down to 0.2 A) and `FIRE` — and so is the cell filter of
`cell = True` (ase/constraints.py::UnitCellFilter with a mask, ASE 3.22, LGPL: `UnitCellFilter` below) — through this driver
with `algo = 'FIRE'`; `cell = True` with `'BFGS'` still asks for ASE.
  `FIRE` and `LBFGS` run on the device (ActiveCalculator.run_relax: the state stays in HBM between model updates): FIRE is
per-atom arithmetic and three global sums; L-BFGS without line search (ase/optimize/lbfgs.py, restated in md_lbfgs.inc and
workloads.lbfgs_relax) is two passes over a history of at most 128 pairs and a small solve.  `LBFGS` is a device-loop optimizer
only — BUILT_IN stays BFGS and FIRE: with a calculator that cannot hand the loop over, and without ASE, the driver answers as for
any other ase.optimize name; with ASE installed and a device-capable calculator it takes the device loop rather than
ase.optimize.LBFGS, exactly as FIRE does.  It has no curvature test: set clear_hist, so that no pair spans a model update.
`BFGS`, the reference's default and therefore the default here, keeps a dense 3N x 3N Hessian and takes its eigen-decomposition every step — 12288^2 at 4096 atoms — and stays on the host, for small systems.
Structures and the trajectory are extended XYZ."""
import argparse

import numpy as np

from . import gen_active_calc, get_default_args, read_args, update_args
from ..sgprio import Frame, format_extxyz
from .md import read_structure


def force_max(forces):
    """The convergence measure of ase.optimize.Optimizer.converged: the largest atomic force."""
    return float(np.sqrt((np.asarray(forces) ** 2).sum(axis=1).max())) if len(forces) else 0.0


def voigt_mask(mask):
    """Six Voigt flags xx yy zz yz xz xy (None: all ones) as the symmetric 3 x 3 matrix UnitCellFilter multiplies with."""
    m = np.ones(6) if mask is None else np.asarray(mask, float)
    if m.shape == (3, 3):
        return m.copy()
    if m.shape != (6,):
        raise ValueError("mask: six Voigt flags (xx yy zz yz xz xy) or a 3 x 3 matrix")
    return np.array([[m[0], m[5], m[4]], [m[5], m[1], m[3]], [m[4], m[3], m[2]]])


class UnitCellFilter:
    """ase.constraints.UnitCellFilter(atoms, mask=mask) restated (ASE 3.22, LGPL; the only form the reference uses,
    cl/relax.py:45-48): positions and cell as ONE set of N + 3 generalised coordinates for an optimizer.  With h0 the cell at
    construction (rows = vectors), D the deformation gradient (h = h0 D^T) and c = N (ASE's cell_factor):
        get_positions:  [ x D^-T ; c D ]
        get_forces:     [ F D ; (W D^-T o M) / c ],   W = -V stress (the full 3 x 3 matrix of the six components)
        set_positions:  D = X[N:] / c,  h = h0 D^T,  x = X[:N] D^T
    The other keywords of ASE's class are not restated."""

    def __init__(self, atoms, mask=None, cell_factor=None, hydrostatic_strain=False, constant_volume=False, scalar_pressure=0.0):
        if hydrostatic_strain or constant_volume or scalar_pressure:
            raise NotImplementedError("UnitCellFilter: hydrostatic_strain, constant_volume and scalar_pressure are ASE's own: install ASE")
        self.atoms = atoms
        self.orig_cell = np.array(atoms.cell, float).reshape(3, 3)
        self.mask = voigt_mask(mask)
        self.cell_factor = float(len(atoms)) if cell_factor is None else float(cell_factor)

    def __len__(self):
        return len(self.atoms) + 3

    def deform_grad(self):
        return np.linalg.solve(self.orig_cell, np.asarray(self.atoms.cell, float)).T

    def get_positions(self):
        D = self.deform_grad()
        return np.concatenate([np.linalg.solve(D, self.atoms.positions.T).T, self.cell_factor * D])

    def set_positions(self, new):
        n = len(self.atoms)
        new = np.asarray(new, float)
        D = new[n:] / self.cell_factor
        # (scale_atoms, as ASE does: atoms held by a constraint follow the cell — their undeformed coordinate is what stays —;
        # without constraints the positions are overwritten in full below and the scaling would be work for nothing)
        self.atoms.set_cell(self.orig_cell @ D.T, scale_atoms=bool(len(getattr(self.atoms, "constraints", None) or ())))
        self.atoms.set_positions(new[:n] @ D.T)

    def get_forces(self):
        a = self.atoms
        F, s = np.asarray(a.get_forces(), float), np.asarray(a.get_stress(), float)
        W = -a.get_volume() * np.array([[s[0], s[5], s[4]], [s[5], s[1], s[3]], [s[4], s[3], s[2]]])
        D = self.deform_grad()
        return np.concatenate([F @ D, np.linalg.solve(D, W.T).T * self.mask / self.cell_factor])

    def get_potential_energy(self):
        return self.atoms.get_potential_energy()


class BFGS:
    """ase/optimize/bfgs.py restated: quasi-Newton on the coordinates with a dense 3N x 3N Hessian (an eigen-decomposition
    per step: for small systems)."""

    def __init__(self, atoms, maxstep=0.2, alpha=70.0):
        self.atoms, self.maxstep, self.alpha = atoms, maxstep, alpha
        self.initialize()

    def initialize(self):
        self.H, self.pos0, self.forces0 = None, None, None

    def update(self, pos, forces):
        if self.H is None:
            self.H = np.eye(len(pos)) * self.alpha
            return
        dpos = pos - self.pos0
        if np.abs(dpos).max() < 1e-7:   # (same configuration again: nothing learnt)
            return
        dforces = forces - self.forces0
        a = dpos @ dforces
        dg = self.H @ dpos
        b = dpos @ dg
        self.H -= np.outer(dforces, dforces) / a + np.outer(dg, dg) / b

    def step(self, forces):
        pos = self.atoms.get_positions()
        f = np.asarray(forces, float).reshape(-1)
        self.update(pos.reshape(-1), f)
        omega, V = np.linalg.eigh(self.H)
        dpos = (V @ ((f @ V) / np.fabs(omega))).reshape(-1, 3)
        longest = np.sqrt((dpos ** 2).sum(axis=1)).max()
        if longest >= self.maxstep:
            dpos *= self.maxstep / longest
        self.pos0, self.forces0 = pos.reshape(-1).copy(), f.copy()
        self.atoms.set_positions(pos + dpos)


class FIRE:
    """ase/optimize/fire.py restated (Bitzek et al., PRL 97, 170201): damped dynamics with an adaptive time step."""

    def __init__(self, atoms, dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99):
        self.atoms = atoms
        self.dt0, self.maxstep, self.dtmax, self.nmin, self.finc, self.fdec, self.astart, self.fa = dt, maxstep, dtmax, nmin, finc, fdec, astart, fa
        self.initialize()

    def initialize(self):
        self.v, self.dt, self.a, self.nsteps = None, self.dt0, self.astart, 0

    def step(self, forces):
        f = np.asarray(forces, float)
        if self.v is None:
            self.v = np.zeros_like(f)
        else:
            vf = np.vdot(f, self.v)
            if vf > 0.0:
                self.v = (1.0 - self.a) * self.v + self.a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(self.v, self.v))
                if self.nsteps > self.nmin:
                    self.dt = min(self.dt * self.finc, self.dtmax)
                    self.a *= self.fa
                self.nsteps += 1
            else:
                self.v[:] = 0.0
                self.a = self.astart
                self.dt *= self.fdec
                self.nsteps = 0
        self.v += self.dt * f
        dr = self.dt * self.v
        norm = np.sqrt(np.vdot(dr, dr))
        if norm > self.maxstep:
            dr = self.maxstep * dr / norm
        self.atoms.set_positions(self.atoms.get_positions() + dr)


BUILT_IN = {"BFGS": BFGS, "FIRE": FIRE}


class _Runner:
    """`dyn.irun(fmax)` / `dyn.run(fmax)` / `dyn.initialize()` of an ase.optimize optimizer around the built-in steppers."""

    def __init__(self, atoms, algo, trajectory, master, max_steps=100000, target=None):
        # (target: what the optimizer moves — the atoms, or a UnitCellFilter around them)
        self.target = atoms if target is None else target
        self.atoms, self.opt, self.master, self.max_steps = atoms, BUILT_IN[algo](self.target), master, max_steps
        self.out = open(trajectory, "w") if (trajectory and master) else None
        self.nsteps = 0

    def initialize(self):
        self.opt.initialize()

    def _dump(self, forces):
        if self.out is not None:
            a = self.atoms
            self.out.writelines(format_extxyz(Frame(a.numbers, a.positions, a.cell, a.pbc, a.calc.results.get("energy"), forces[:len(a)], None)))
            self.out.flush()
        if self.master:
            print(f"{type(self.opt).__name__}: {self.nsteps:4d}  energy {self.atoms.calc.results.get('energy', float('nan')):.6f}  fmax {force_max(forces):.4f}")

    def irun(self, fmax):
        forces = self.target.get_forces()
        self._dump(forces)
        yield False
        while force_max(forces) >= fmax and self.nsteps < self.max_steps:
            self.opt.step(forces)
            self.nsteps += 1
            forces = self.target.get_forces()
            self._dump(forces)
            yield False
        yield True

    def run(self, fmax):
        for _ in self.irun(fmax):
            pass
        return force_max(self.target.get_forces()) < fmax


class _DeviceRunner:
    """The same surface around ActiveCalculator.run_relax: FIRE or L-BFGS (`algo`) with the state in device memory between model
    updates.  Every run starts the optimizer afresh (relax_begin); clear_hist re-initialises it behind every model update inside
    a run."""

    def __init__(self, atoms, calc, cell, mask, trajectory, master, clear_hist, max_steps=100000, algo="FIRE"):
        self.atoms, self.calc, self.cell, self.mask, self.master, self.clear_hist, self.max_steps = atoms, calc, cell, mask, master, clear_hist, max_steps
        self.algo = algo
        self.out = open(trajectory, "w") if (trajectory and master) else None
        self.nsteps = 0

    def initialize(self):
        pass

    def _write(self, n, fr):
        a = self.atoms
        self.out.writelines(format_extxyz(Frame(a.numbers, fr["positions"], fr["cell"], a.pbc, float(fr["energy"]), fr["forces"], None)))

    def run(self, fmax):
        # (a frame per evaluation, as _Runner writes them: from the device loop's frame record, the run is not cut for it; the last
        # one is the final structure with the results the calculator then answers with)
        res = self.calc.run_relax(self.atoms, fmax=fmax, steps=self.max_steps, cell=self.cell, mask=self.mask, clear_hist=self.clear_hist,
                                  on_frame=self._write if self.out is not None else None, **({} if self.algo == "FIRE" else dict(optimizer=self.algo)))
        self.nsteps += res["steps"]
        a, r = self.atoms, self.calc.results
        if self.out is not None:
            self.out.flush()
        if self.master:
            print(f"{self.algo} (device): {self.nsteps:4d}  energy {float(r['energy']):.6f}  fmax {force_max(r['forces']):.4f}")
        return res["converged"]

    def irun(self, fmax):
        yield False
        yield self.run(fmax)


def _optimizer(atoms, algo, cell, mask, trajectory, master, clear_hist=False):
    calc = atoms.calc
    # FIRE is per-atom arithmetic and three global sums, L-BFGS two passes over its history and a memory x memory solve: they run
    # inside the device loop where the calculator can hand the loop over (BFGS, the default, needs a dense Hessian's
    # eigen-decomposition per step and stays on the host).  LBFGS is a device-loop optimizer only: without such a calculator
    # (and without ASE) the driver answers as it does for any name outside BUILT_IN
    # (atoms.constraints: FixAtoms and FixCartesian are held inside the device loop; any other kind stays with the host optimizer)
    if algo in ("FIRE", "LBFGS") and hasattr(calc, "run_relax") and hasattr(calc, "md_on_device_ok") and (calc.md_on_device_ok() or calc._needs_seed()) \
            and all(type(c).__name__ in ("FixAtoms", "FixCartesian") for c in (getattr(atoms, "constraints", None) or ())):
        return _DeviceRunner(atoms, calc, cell, mask, trajectory, master, clear_hist, algo=algo)
    try:
        from ase import optimize
        from ase.constraints import UnitCellFilter as AseUnitCellFilter
    except ImportError:
        if algo not in BUILT_IN:
            raise NotImplementedError(f"algo = '{algo}' is an ase.optimize class: install ASE; without it: {sorted(BUILT_IN)}")
        if cell and algo != "FIRE":
            # (the driver relaxes a cell with FIRE only: the dense Hessian of BFGS over 3N + 9 coordinates that differ in scale
            # by the cell factor is ASE's own business — the class itself accepts the filter, for whoever drives it by hand)
            raise NotImplementedError("cell = True with algo = 'BFGS' is ase.constraints.UnitCellFilter around ase.optimize.BFGS "
                                      "(cl/relax.py:46-49): install ASE; without it algo = 'FIRE' relaxes the cell")
        return _Runner(atoms, algo, trajectory, master, target=UnitCellFilter(atoms, mask=mask) if cell else None)
    filtered = AseUnitCellFilter(atoms, mask=mask) if cell else atoms          # cl/relax.py:46-49
    return getattr(optimize, algo)(filtered, trajectory=trajectory, master=master)


def relax(atoms, fmax=0.01, cell=False, mask=None, algo="BFGS", trajectory="relax.xyz", rattle=0.02, clear_hist=False, confirm=True,
          calc=None, seed=None):
    """The keywords of theforce/cl/relax.py::relax (same names and defaults; the trajectory is extended XYZ unless ASE
    writes it).  Returns the number of exact (teacher) calculations the run asked for.
      algo = "FIRE" or "LBFGS" with a calculator whose md_on_device_ok() holds: the minimisation and every re-run of the confirm loop go
    through ActiveCalculator.run_relax — the state stays on the device between model updates, cell = True included.  The default
    stays the reference's "BFGS", which does not scale (a dense 3N x 3N Hessian and its eigen-decomposition every step) and
    runs on the host only."""
    rng = np.random.default_rng(seed)
    numbers = np.asarray(atoms.numbers)
    calc = gen_active_calc(species=sorted(set(int(z) for z in numbers))) if calc is None else calc
    load1 = calc.size[0]
    master = calc.rank == 0
    if rattle:
        atoms.set_positions(atoms.get_positions() + rng.normal(scale=rattle, size=(len(numbers), 3)))   # atoms.rattle(rattle)
    atoms.calc = calc
    dyn = _optimizer(atoms, algo, cell, mask, trajectory, master, clear_hist)
    for _ in dyn.irun(fmax):
        if calc.updated and clear_hist:
            dyn.initialize()
    load2 = calc.size[0]
    if calc.active and confirm:                                             # cl/relax.py:59-70
        while True:
            load2 += 1
            if calc.update_data(try_fake=False):
                calc.update(data=False)
                calc.results.clear()
                if clear_hist:
                    dyn.initialize()
                dyn.run(fmax=fmax)
            else:
                break
        ml = ("ML", calc.results["energy"], calc.results["forces"])
        exact = ("Ab initio", *calc._test())
        for method, energy, forces in (ml, exact):
            forces = np.asarray(forces)
            if master:
                print(f"\n    relaxation result ({method}):\n    energy:      {energy}\n    force (rms): {np.sqrt(np.mean(forces ** 2))}\n"
                      f"    force (max): {abs(forces).max()}\n")
    if master:
        print(f"\tTotal number of Ab initio calculations: {load2 - load1}\n")
    return load2 - load1


def main(argv=None):
    ap = argparse.ArgumentParser(description="Machine Learning accelerated relaxation")
    ap.add_argument("-i", "--input", default="POSCAR.xyz", help="the initial coordinates of the atoms (extended XYZ)")
    ap.add_argument("-o", "--output", default="CONTCAR.xyz", help="the final coordinates of the atoms (extended XYZ)")
    a = ap.parse_args(argv)
    from ..ase_shim import Atoms
    fr = read_structure(a.input)
    atoms = Atoms(fr.numbers, fr.positions, fr.cell, fr.pbc)
    kwargs = get_default_args(relax)
    kwargs.pop("calc", None)
    update_args(kwargs, read_args())
    relax(atoms, **kwargs)
    with open(a.output, "w") as f:
        f.writelines(format_extxyz(Frame(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc, None, None, None)))


if __name__ == "__main__":
    main()
