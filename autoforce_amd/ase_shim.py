"""Minimal stand-ins for the few ASE names the calculator surface touches, used ONLY when ASE is
not installed (it is absent from the build image; SURVEY.md §8c lists the API the reference's hot
path uses: Atoms.positions/numbers/cell/pbc/get_volume/get_temperature/copy/.calc and
Calculator.__init__/calculate/results/get_property).  With ASE present, autoforce_amd.calculator
subclasses ase.calculators.calculator.Calculator and these classes are not used.
"""
import numpy as np

all_changes = ["positions", "numbers", "cell", "pbc", "initial_charges", "initial_magmoms"]
kB = 8.617330337217213e-05  # eV/K (ase.units.kB)
kcal_mol = 0.04336410390059322  # eV (ase.units.kcal / ase.units.mol)


class FixAtoms:
    """ase.constraints.FixAtoms: the chosen atoms do not move.  indices: integers, or mask: [N] booleans, True = held."""

    def __init__(self, indices=None, mask=None):
        if (indices is None) == (mask is None):
            raise ValueError("FixAtoms: indices or mask, one of them")
        self.index = np.nonzero(np.asarray(mask, bool))[0] if indices is None else np.unique(np.asarray(indices, int).reshape(-1))

    def get_removed_dof(self, atoms):
        return 3 * len(self.index)

    def adjust_positions(self, atoms, new):
        new[self.index] = atoms.positions[self.index]

    def adjust_momenta(self, atoms, momenta):
        momenta[self.index] = 0.0

    adjust_forces = adjust_momenta

    def copy(self):
        return FixAtoms(indices=self.index)


class FixCartesian:
    """ase.constraints.FixCartesian: the chosen Cartesian components of the atoms `a` do not move.  mask: three flags, True =
    held (the meaning of ASE 3.23; readers derive the components from adjust_forces, not from the attributes)."""

    def __init__(self, a, mask=(True, True, True)):
        self.index = np.unique(np.asarray(a, int).reshape(-1))
        self.mask = np.asarray(mask, bool).reshape(3).copy()

    def get_removed_dof(self, atoms):
        return int(self.mask.sum()) * len(self.index)

    def adjust_positions(self, atoms, new):
        new[self.index] = np.where(self.mask, atoms.positions[self.index], new[self.index])

    def adjust_momenta(self, atoms, momenta):
        momenta[self.index] = np.where(self.mask, 0.0, momenta[self.index])

    adjust_forces = adjust_momenta

    def copy(self):
        return FixCartesian(self.index, self.mask)


def constraints_from_mask(fixed):
    """An [N, 3] held-component mask (True = held) as a list of constraints: FixAtoms for the atoms held in all three
    components, one FixCartesian per other pattern of components.  None / nothing held: None."""
    if fixed is None:
        return None
    fx = np.asarray(fixed, bool).reshape(-1, 3)
    out = []
    whole = fx.all(axis=1)
    if whole.any():
        out.append(FixAtoms(mask=whole))
    code = fx[:, 0] * 1 + fx[:, 1] * 2 + fx[:, 2] * 4
    for c in range(1, 7):
        idx = np.nonzero(code == c)[0]
        if len(idx):
            out.append(FixCartesian(idx, [bool(c & 1), bool(c & 2), bool(c & 4)]))
    return out or None


class Atoms:
    def __init__(self, numbers=None, positions=None, cell=None, pbc=False, velocities=None, masses=None,
                 calculator=None, constraint=None):
        self.numbers = np.asarray(numbers, dtype=int).copy()
        self.positions = np.asarray(positions, dtype=float).reshape(-1, 3).copy()
        self.cell = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=float).reshape(3, 3).copy()
        self.pbc = np.broadcast_to(np.asarray(pbc, dtype=bool), (3,)).copy()
        self._velocities = None if velocities is None else np.asarray(velocities, float).copy()
        self._masses = None if masses is None else np.asarray(masses, float).copy()
        self.calc = calculator
        self.constraints = []
        self.set_constraint(constraint)
        if self.constraints and self._velocities is not None:   # (ase.Atoms.__init__ sets the velocities under the constraints)
            self.set_velocities(self._velocities)

    def set_constraint(self, constraint=None):
        """ase.Atoms.set_constraint: one constraint, a list of them, or None (none)."""
        self.constraints = [] if constraint is None else (list(constraint) if isinstance(constraint, (list, tuple)) else [constraint])

    def __len__(self):
        return len(self.numbers)

    def get_global_number_of_atoms(self):
        return len(self)

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def get_positions(self):
        return self.positions.copy()

    def set_positions(self, p, apply_constraint=True):
        new = np.asarray(p, float).reshape(-1, 3).copy()
        if apply_constraint:
            for c in self.constraints:   # (held coordinates keep their current values: ase.Atoms.set_positions)
                c.adjust_positions(self, new)
        self.positions = new

    def get_cell(self):
        return self.cell.copy()

    def set_cell(self, cell, scale_atoms=False):
        """ase.Atoms.set_cell: scale_atoms moves the atoms with the cell (the same fractional coordinates)."""
        new = np.asarray(cell, dtype=float).reshape(3, 3).copy()
        if scale_atoms:
            self.positions = self.positions @ np.linalg.solve(self.cell, new)
        self.cell = new

    def get_pbc(self):
        return self.pbc.copy()

    def get_volume(self):
        v = abs(np.linalg.det(self.cell))
        if v == 0.0:
            raise ValueError("You have atoms with no cell; volume not defined")
        return v

    def get_velocities(self):
        return None if self._velocities is None else self._velocities.copy()

    def set_velocities(self, v):
        new = np.asarray(v, float).reshape(-1, 3).copy()
        for c in self.constraints:       # (held components: zero, as ase.Atoms.set_momenta under a constraint)
            c.adjust_momenta(self, new)
        self._velocities = new

    def get_masses(self):
        return np.ones(len(self)) if self._masses is None else self._masses.copy()

    def get_kinetic_energy(self):
        if self._velocities is None:
            return 0.0
        return 0.5 * float((self.get_masses()[:, None] * self._velocities**2).sum())

    def get_number_of_degrees_of_freedom(self):
        return 3 * len(self) - sum(c.get_removed_dof(self) for c in self.constraints)

    def get_temperature(self):
        n = len(self)
        if n == 0:
            return 0.0
        if not self.constraints:
            return 2.0 * self.get_kinetic_energy() / (3.0 * n * kB)
        return 2.0 * self.get_kinetic_energy() / (self.get_number_of_degrees_of_freedom() * kB)   # (the remaining ones, as ASE)

    def copy(self):
        return Atoms(self.numbers, self.positions, self.cell, self.pbc, self._velocities, self._masses,
                     constraint=[c.copy() for c in self.constraints] or None)

    # ASE protocol: atoms.get_*() -> calc.get_property()
    def _get(self, name):
        if self.calc is None:
            raise RuntimeError("Atoms object has no calculator.")
        return self.calc.get_property(name, self)

    def get_potential_energy(self):
        return float(self._get("energy"))

    def get_forces(self, apply_constraint=True):
        F = np.array(self._get("forces"))
        if apply_constraint:
            for c in self.constraints:   # (zero on held components; calc.results["forces"] stay the calculator's own)
                c.adjust_forces(self, F)
        return F

    def get_stress(self):
        return np.array(self._get("stress"))


class Calculator:
    implemented_properties = []

    def __init__(self, **kw):
        self.atoms = None
        self.results = {}

    def _changed(self, atoms):
        a = self.atoms
        # (positions first: in a loop they are what has changed — and of them the first coordinate, one scalar comparison,
        # before 3N of them)
        if a is None or len(a) != len(atoms) or (len(a) and a.positions[0, 0] != atoms.positions[0, 0]):
            return True
        return (not np.array_equal(a.positions, atoms.positions)
                or not np.array_equal(a.numbers, atoms.numbers) or not np.array_equal(a.cell, atoms.cell)
                or not np.array_equal(a.pbc, atoms.pbc))

    def calculate(self, atoms=None, properties=("energy",), system_changes=all_changes):
        """ase.calculators.calculator.Calculator.calculate: the calculator keeps a COPY of the atoms it was asked about.  The
        copy of the previous call is re-used when the frame is the same system (same numbers): its arrays are overwritten in
        place instead of six fresh allocations per step."""
        if atoms is None:
            return
        a = self.atoms
        if (a is not None and a is not atoms and len(a) == len(atoms) and np.array_equal(a.numbers, atoms.numbers)
                and (a._velocities is None) == (atoms._velocities is None) and (a._masses is None) == (atoms._masses is None)):
            np.copyto(a.positions, atoms.positions)
            np.copyto(a.cell, atoms.cell)
            np.copyto(a.pbc, atoms.pbc)
            if atoms._velocities is not None:
                np.copyto(a._velocities, atoms._velocities)
            if atoms._masses is not None:
                np.copyto(a._masses, atoms._masses)
        else:
            self.atoms = atoms.copy()

    def get_property(self, name, atoms=None):
        if name not in self.implemented_properties:
            raise NotImplementedError(name)
        if atoms is not None and (self._changed(atoms) or name not in self.results):
            self.results = {}
            self.calculate(atoms, [name], all_changes)
        return self.results[name]


class SinglePointCalculator(Calculator):
    """ase.calculators.singlepoint.SinglePointCalculator: stored results for one configuration."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, atoms, **results):
        Calculator.__init__(self)
        self.atoms = atoms.copy()
        self.results = {k: (np.array(v, float) if k != "energy" else float(v)) for k, v in results.items()
                        if v is not None}

    def get_property(self, name, atoms=None):
        if name not in self.results:
            raise NotImplementedError(f"SinglePointCalculator holds no {name}")
        if atoms is not None and self._changed(atoms):
            raise RuntimeError("SinglePointCalculator: the atoms have changed since the stored calculation")
        return self.results[name]
