"""relax(cell=True) without ASE: cl/relax.py's UnitCellFilter (ase.constraints.UnitCellFilter with a mask, restated) under the
built-in FIRE and BFGS around a CPU teacher — the filter's generalised forces against central differences of the energy, the
minimisation itself, the mask.  The system is the sheared 27-atom cell of test_npt_twin_cpu.py stretched by 4 %."""
import numpy as np
import pytest

from autoforce_amd.ase_shim import Atoms
from autoforce_amd.cl.relax import BFGS, FIRE, UnitCellFilter, force_max, relax
from helpers import PairTeacher
from test_npt_twin_cpu import _system

MASKS = [None, [1, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0]]
IDS = ["full", "diagonal", "zz"]


class _Calc(PairTeacher):
    """The teacher with the few attributes cl.relax.relax reads from an active calculator (it learns nothing)."""
    size, rank, active, updated = (0, 0), 0, False, False


def _atoms(calc=None):
    numbers, pos, cell, mass, v = _system(shear=True)
    at = Atoms(numbers, 1.04 * pos, 1.04 * cell, True)
    at.calc = _Calc(rc=4.0) if calc is None else calc
    return at


def _sym(mask):
    m = np.ones(6) if mask is None else np.asarray(mask, float)
    return np.array([[m[0], m[5], m[4]], [m[5], m[1], m[3]], [m[4], m[3], m[2]]])


def test_relax_with_a_cell_returns(tmp_path):
    """On the parent: NotImplementedError (cell = True needed ASE)."""
    at = _atoms()
    cell0, e0 = at.cell.copy(), at.get_potential_energy()
    n = relax(at, fmax=0.01, cell=True, algo="FIRE", confirm=False, rattle=0, calc=at.calc, trajectory=str(tmp_path / "relax.xyz"))
    assert n == 0
    assert np.abs(at.cell - cell0).max() > 1e-3 and at.get_potential_energy() < e0
    # (a fresh filter refers to the relaxed cell, D = 1: its generalised forces are the forces and -V stress / N)
    assert force_max(UnitCellFilter(at).get_forces()) < 0.01
    for algo in ("LBFGS", "BFGS"):   # (the driver relaxes a cell with FIRE; the BFGS class itself takes the filter: below)
        with pytest.raises(NotImplementedError):
            relax(_atoms(), cell=True, algo=algo, confirm=False, rattle=0, calc=_Calc(rc=4.0), trajectory=None)
    for kw in (dict(hydrostatic_strain=True), dict(constant_volume=True), dict(scalar_pressure=0.1)):
        with pytest.raises(NotImplementedError):
            UnitCellFilter(_atoms(), **kw)


@pytest.mark.parametrize("mask", MASKS, ids=IDS)
def test_generalised_forces_are_minus_the_gradient(mask):
    """-G . delta against the central difference of the energy along random directions of X, away from the identity (the
    filter has already deformed the cell), rtol 1e-6."""
    rng = np.random.default_rng(7)
    at = _atoms()
    flt = UnitCellFilter(at, mask=mask)
    N = len(at)
    M = _sym(mask)
    X = flt.get_positions()
    X[:N] += 0.02 * rng.normal(size=(N, 3))
    X[N:] += N * 0.01 * rng.normal(size=(3, 3)) * M
    flt.set_positions(X)
    np.testing.assert_allclose(flt.get_positions(), X, rtol=0, atol=1e-9)
    G = flt.get_forces()
    assert G.shape == (N + 3, 3)
    for _ in range(3):
        d = rng.normal(size=(N + 3, 3))
        d[N:] *= N * M
        d *= 1e-5 / np.linalg.norm(d)
        flt.set_positions(X + d)
        ep = at.get_potential_energy()
        flt.set_positions(X - d)
        em = at.get_potential_energy()
        num, ana = (ep - em) / 2.0, -float((G * d).sum())
        print(mask, num, ana)
        assert abs(num - ana) <= 1e-6 * abs(ana), (num, ana)
    flt.set_positions(X)


@pytest.mark.parametrize("mask", MASKS, ids=IDS)
def test_fire_converges_and_the_mask_holds(mask):
    at = _atoms()
    flt = UnitCellFilter(at, mask=mask)
    opt = FIRE(flt)
    e0, n = at.get_potential_energy(), 0
    f = flt.get_forces()
    off = _sym(mask) == 0
    while force_max(f) >= 0.01:
        assert n < 400, "FIRE has not converged within 400 evaluations"
        opt.step(f)
        n += 1
        f = flt.get_forces()
        assert np.abs((flt.deform_grad() - np.eye(3))[off]).max() <= 1e-12 if off.any() else True
    print(mask, "evaluations", n + 1)
    assert at.get_potential_energy() < e0
    if mask is None:
        assert np.abs(at.get_stress()).max() < 1e-3
        assert np.count_nonzero(np.abs(at.cell) > 1e-6) == 9       # a general cell: all nine components


def test_bfgs_with_a_cell_converges():
    at = _atoms()
    flt = UnitCellFilter(at)
    opt = BFGS(flt)
    e0, n = at.get_potential_energy(), 0
    f = flt.get_forces()
    while force_max(f) >= 0.01:
        assert n < 400, "BFGS has not converged within 400 evaluations"
        opt.step(f)
        n += 1
        f = flt.get_forces()
    print("BFGS evaluations", n + 1)
    assert at.get_potential_energy() < e0 and np.abs(at.get_stress()).max() < 1e-3
