"""cl.md's moving-cell branch: `md(dynamics='NPT', bulk_modulus=...)` goes through the calculator's run_md — once per
temperature, with ase.md.npt.NPT's keywords as the reference sets them (pfactor = (pdamp fs)^2 x bulk modulus GPa, externalstress
= stress GPa, mask, iso), the Nose-Hoover damping time, and the ONE filter holder of the loop — on the upper-triangular cell; where
the atoms carry constraints the integrator around calculate() (npt_dynamics) stays.  A stub calculator records the calls."""
import numpy as np

import autoforce_amd.cl.md as clmd
from autoforce_amd.ase_shim import Atoms, FixAtoms
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.npt import GPA
from autoforce_amd.workloads import FS, FilterState


class _Stub:
    """What md() touches of a calculator: not active (no manual steps), rank 0, the mask of the constraints, run_md."""
    active, rank = False, 0
    constraint_mask = staticmethod(ActiveCalculator.constraint_mask)

    def __init__(self):
        self.calls = []

    def run_md(self, atoms, steps, temperature_K, **kw):
        self.calls.append((steps, temperature_K, kw, np.array(atoms.cell, float), atoms.positions.copy()))
        for step in range(steps + 1):
            yield step, -1.0, temperature_K, False, 0.0


def _atoms():
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    cell = np.diag([6.0, 7.0, 8.0]) @ R.T                            # not upper triangular
    pos = np.random.default_rng(0).uniform(0.0, 6.0, size=(5, 3)) @ R.T
    return Atoms([3, 3, 15, 16, 16], pos, cell, True), cell


def test_moving_cell_goes_through_run_md_once_per_temperature(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(clmd, "npt_dynamics", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fallback was taken")))
    atoms, cell = _atoms()
    d0 = np.linalg.norm(atoms.positions[0] - atoms.positions[1])
    calc = _Stub()
    clmd.md(atoms, calc=calc, dynamics="NPT", bulk_modulus=30.0, stress=0.5, mask=(1, 1, 0), iso=True, tem=[300.0, 450.0], picos=-6, dt=2.0,
            tdamp=40, pdamp=150, ml_filter=0.7, trajectory="t.xyz", loginterval=3, seed=1)
    assert [(c[0], c[1]) for c in calc.calls] == [(6, 300.0), (6, 450.0)]
    for steps, T, kw, c, x in calc.calls:
        assert kw["pfactor"] == (150 * FS) ** 2 * 30.0 * GPA and kw["externalstress"] == 0.5 * GPA
        assert kw["mask"] == (1, 1, 0) and kw["iso"] is True and kw["tdamp_fs"] == 40.0 and kw["dt_fs"] == 2.0 and kw["sync_every"] == 3
        assert c[1, 0] == c[2, 0] == c[2, 1] == 0.0                  # behind make_cell_upper_triangular
        assert abs(abs(np.linalg.det(c)) - abs(np.linalg.det(cell))) < 1e-9 and abs(np.linalg.norm(x[0] - x[1]) - d0) < 1e-12
    holders = [c[2]["ml_filter"] for c in calc.calls]
    assert isinstance(holders[0], FilterState) and holders[0] is holders[1] and holders[0].shrink == 0.7   # the one holder
    assert len(clmd.read_frames("t.xyz", ":")) == 2 * 3              # steps 0, 3, 6 of each temperature
    # without a bulk modulus: Nose-Hoover NVT as before, no barostat keyword
    calc = _Stub()
    clmd.md(_atoms()[0], calc=calc, dynamics="NPT", tem=300.0, picos=-2, trajectory=None, seed=1)
    assert len(calc.calls) == 1 and "pfactor" not in calc.calls[0][2] and calc.calls[0][2]["tdamp_fs"] == 25.0


def test_constraints_fall_back_to_the_integrator_around_calculate(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    taken = []

    class _Dyn:
        def run(self, steps):
            taken.append(steps)
            return iter(())
    monkeypatch.setattr(clmd, "npt_dynamics", lambda atoms, calc, dt, T, bulk, *rest: (taken.append((T, bulk)), _Dyn())[1])
    atoms, _ = _atoms()
    atoms.set_constraint(FixAtoms(indices=[0]))
    calc = _Stub()
    clmd.md(atoms, calc=calc, dynamics="NPT", bulk_modulus=30.0, tem=[300.0, 450.0], picos=-4, trajectory=None, seed=1)
    assert not calc.calls and taken == [(300.0, 30.0), 4, (450.0, 30.0), 4]
