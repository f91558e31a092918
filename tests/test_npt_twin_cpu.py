"""workloads.npt_moving_cell — the moving-cell dynamics written by evaluation index in the device loop's operations (the host
twin of sgpr_md_barostat) — against npt.NPT (ase.md.npt.NPT restated) around the same CPU teacher: the two differ by the
order of rounding only (explicit 3 x 3 algebra and fixed-order sums on one side, BLAS / LAPACK on the other), so over 30
steps they agree to the tolerances the constant-cell twin is held to in test_npt_cpu.py."""
import numpy as np
import pytest

from autoforce_amd.ase_shim import Atoms, kB
from autoforce_amd.npt import GPA, NPT
from autoforce_amd.workloads import FS, MASS, nose_hoover_nvt, npt_moving_cell
from helpers import PairTeacher

STEPS = 30
PFACTOR = (75.0 * FS) ** 2 * 40.0 * GPA


def _system(seed=0, temperature=300.0, a=2.15, shear=False):
    rng = np.random.default_rng(seed)
    sites = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], float) * a
    numbers = np.array(([3, 9] * 14)[:27])
    cell = np.diag([3 * a] * 3)
    pos = sites + 0.05 * rng.normal(size=sites.shape)
    if shear:   # the same fractional coordinates in a cell with all three upper components
        new = cell.copy()
        new[0, 1], new[0, 2], new[1, 2] = 0.21, -0.13, 0.17
        pos = pos @ np.linalg.inv(cell) @ new
        cell = new
    mass = np.array([MASS[int(z)] for z in numbers])
    v = rng.normal(size=pos.shape) * np.sqrt(kB * temperature / mass)[:, None]
    v -= (mass[:, None] * v).sum(0) / mass.sum()
    v -= (mass[:, None] * v).sum(0) / mass[:, None] / len(mass)
    return numbers, pos, cell, mass, v


def _compare(kw_npt, kw_twin, iso=False, shear=False):
    numbers, pos, cell, mass, v = _system(shear=shear)
    at = Atoms(numbers, pos, cell, True, velocities=v, masses=mass)
    at.calc = PairTeacher(rc=4.0)
    dyn = NPT(at, 1.0 * FS, 300.0, ttime=25.0 * FS, **kw_npt)
    if iso:
        dyn.set_fraction_traceless(0.0)
    twin = npt_moving_cell(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, STEPS, 300.0, 1.0, 25.0, vel=v, iso=iso, **kw_twin)
    n = 0
    cells = []
    for (k, E, T, _), (kt, Et, Tt, _, xt, vt, ht, et, zeta, zint) in zip(dyn.run(STEPS), twin):
        assert k == kt
        np.testing.assert_allclose(at.positions, xt, rtol=0, atol=1e-10)
        np.testing.assert_allclose(np.asarray(at.cell), ht, rtol=0, atol=1e-10)
        np.testing.assert_allclose(dyn.eta, et, rtol=0, atol=1e-10)
        assert abs(E - Et) < 1e-9 and abs(dyn.zeta - zeta) < 1e-12 and abs(dyn.zeta_integrated - zint) < 1e-12
        if k:
            np.testing.assert_allclose(at.get_velocities(), vt, rtol=0, atol=1e-10)
        cells.append(ht.copy())
        n += 1
    assert n == STEPS + 1
    return cell, np.array(cells)


def test_full_barostat():
    cell, cells = _compare(dict(externalstress=1.0 * GPA, pfactor=PFACTOR), dict(externalstress=1.0 * GPA, pfactor=PFACTOR))
    assert np.abs(cells[-1] - cell).max() > 1e-6
    assert (cells[:, 1, 0] == 0).all() and (cells[:, 2, 0] == 0).all() and (cells[:, 2, 1] == 0).all()


def test_iso_keeps_the_shape():
    cell, cells = _compare(dict(externalstress=1.0 * GPA, pfactor=PFACTOR), dict(externalstress=1.0 * GPA, pfactor=PFACTOR), iso=True)
    assert cells[-1][0, 0] != cell[0, 0]
    np.testing.assert_allclose(cells[-1] / cells[-1][0, 0], cell / cell[0, 0], atol=1e-12)


def test_mask_freezes_the_other_components():
    kw = dict(externalstress=1.0 * GPA, pfactor=PFACTOR, mask=(0, 0, 1))
    cell, cells = _compare(kw, kw)
    assert cells[-1][2, 2] != cell[2, 2]
    for c in cells:
        c2 = c.copy()
        c2[2, 2] = cell[2, 2]
        np.testing.assert_array_equal(c2, cell)


def test_sheared_start_cell():
    cell, cells = _compare(dict(externalstress=1.0 * GPA, pfactor=PFACTOR), dict(externalstress=1.0 * GPA, pfactor=PFACTOR), shear=True)
    assert cell[0, 1] != 0 and cell[0, 2] != 0 and cell[1, 2] != 0
    assert np.abs(cells[-1] - cell).max() > 1e-6


def test_voigt_external_stress():
    ext = np.array([-1.0, -0.5, -2.0, 0.1, 0.0, -0.2]) * GPA
    _compare(dict(externalstress=ext, pfactor=PFACTOR), dict(externalstress=ext, pfactor=PFACTOR))


def test_without_a_barostat_it_is_nose_hoover():
    numbers, pos, cell, mass, v = _system()
    _compare(dict(pfactor=None), dict(pfactor=None))
    ref = nose_hoover_nvt(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, STEPS, 300.0, 1.0, 25.0, vel=v)
    twin = npt_moving_cell(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, STEPS, 300.0, 1.0, 25.0, vel=v, pfactor=None)
    for (k, E, T, _, x, vv, zeta, zint), (kt, Et, Tt, _, xt, vt, ht, et, zt, zit) in zip(ref, twin):
        np.testing.assert_allclose(xt, x, rtol=0, atol=1e-10)
        np.testing.assert_allclose(vt, vv, rtol=0, atol=1e-10)
        assert abs(E - Et) < 1e-9 and abs(zeta - zt) < 1e-12 and abs(zint - zit) < 1e-12
        np.testing.assert_array_equal(ht, cell)
        assert not et.any()


def test_a_cell_that_is_not_upper_triangular_is_refused():
    numbers, pos, cell, mass, v = _system()
    bad = cell.copy()
    bad[1, 0] = 0.1
    with pytest.raises(ValueError):
        next(npt_moving_cell(PairTeacher(rc=4.0), numbers, pos, bad, [True] * 3, 2, 300.0, 1.0, 25.0, vel=v, pfactor=PFACTOR))
