"""workloads.fire_relax — FIRE on positions (and cell) written by evaluation index in the device loop's operations, the host
twin of sgpr_md_relax — against cl/relax.py's FIRE (and UnitCellFilter) around the same CPU teacher: the two differ by the
order of rounding only (explicit 3 x 3 algebra, fixed-order sums and the closed form of the step length on one side, numpy /
LAPACK on the other), so over 60 evaluations they take the same branch decisions — nsteps, dt and a equal exactly — and agree
on positions, cell and energies to the tolerances of test_npt_twin_cpu.py."""
import numpy as np
import pytest

from autoforce_amd.ase_shim import Atoms
from autoforce_amd.cl.relax import FIRE, UnitCellFilter
from autoforce_amd.workloads import fire_relax
from helpers import PairTeacher
from test_npt_twin_cpu import _system

EVALS = 60


def _start():
    numbers, pos, cell, mass, v = _system(shear=True)
    return numbers, 1.04 * pos, 1.04 * cell


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True), dict(cell_relax=True, mask=[1, 1, 1, 0, 0, 0]),
                                dict(cell_relax=True, dt=0.05, maxstep=0.05, nmin=3)],
                         ids=["positions", "cell", "cell-diagonal", "cell-keywords"])
def test_twin_is_fire_around_the_filter(kw):
    numbers, pos, cell = _start()
    fire = {k: v for k, v in kw.items() if k not in ("cell_relax", "mask")}
    at = Atoms(numbers, pos, cell, True)
    at.calc = PairTeacher(rc=4.0)
    target = UnitCellFilter(at, mask=kw.get("mask")) if kw.get("cell_relax") else at
    opt = FIRE(target, **fire)
    seen, n = set(), 0
    for o in fire_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, EVALS, 1e-6, **kw):
        assert o["n"] == n and not o["converged"]
        f = target.get_forces()
        np.testing.assert_allclose(at.positions, o["positions"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(at.cell, o["cell"], rtol=0, atol=1e-10)
        assert abs(at.get_potential_energy() - o["energy"]) < 1e-9
        assert abs((f ** 2).sum(axis=1).max() - o["gmax2"]) < 1e-12
        if kw.get("cell_relax"):
            np.testing.assert_allclose(target.deform_grad(), o["D"], rtol=0, atol=1e-12)
        opt.step(f)
        assert (opt.nsteps, opt.dt, opt.a) == (o["nsteps"], o["dt"], o["a"]), (n, opt.nsteps, opt.dt, opt.a, o["nsteps"], o["dt"], o["a"])
        seen.add((o["dt"], o["a"]))
        n += 1
    assert n == EVALS + 1
    assert len(seen) > 5   # the walk has raised its time step and cut it back: both branches were taken


def test_twin_reset_and_convergence():
    numbers, pos, cell = _start()
    rows = list(fire_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, 400, 0.01, cell_relax=True))
    assert rows[-1]["converged"] and len(rows) < 400 and all(not r["converged"] for r in rows[:-1])
    assert rows[-1]["gmax2"] < 1e-4 <= min(r["gmax2"] for r in rows[:-1])
    assert rows[-1]["energy"] < rows[0]["energy"]
    a = list(fire_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, 30, 1e-6, cell_relax=True, reset_at=(20,)))
    b = rows[:31]
    assert all(x["dt"] == y["dt"] and np.array_equal(x["positions"], y["positions"]) for x, y in zip(a[:20], b[:20]))
    assert a[20]["P"] == 0.0 and a[20]["dt"] == 0.1 and a[20]["a"] == 0.1 and np.array_equal(a[20]["positions"], b[20]["positions"])
    assert not np.array_equal(a[21]["positions"], b[21]["positions"])
