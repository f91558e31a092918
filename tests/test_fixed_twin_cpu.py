"""Held atoms and components (`fixed=`) in the host twins of the device loops — workloads.langevin_nvt, nose_hoover_nvt and
fire_relax —, the constraint classes of ase_shim and the mask ActiveCalculator derives from atoms.constraints.  The rules (the
ones sgpr_md_fix states): the integrator sees F = 0 on a held component, its velocity is exactly 0, it draws no noise, and its
coordinate is handed on by selection — bit for bit the one it started with (FIRE with a moving cell: the undeformed coordinate).
  Without a mask the twins must keep the bits they had before `fixed=` existed: tests/golden/fixed_twins_unmasked.npz holds
walks of the three twins recorded from the commit before it (tests/golden/gen/make_fixed_twins.py, which runs fixed_common.walks on
whatever package it finds) around fixed_common.Springs, a toy calculator of elementwise arithmetic only — no library call whose
rounding could depend on the machine."""
import os

import numpy as np
import pytest

from autoforce_amd.ase_shim import Atoms, FixAtoms, FixCartesian, constraints_from_mask, kB
from autoforce_amd.cl.relax import FIRE, UnitCellFilter
from autoforce_amd.workloads import FS, MASS, _row_mul, fire_relax, langevin_nvt, nose_hoover_nvt
from fixed_common import mask as _mask, toy as _toy, walks as _walks
from helpers import PairTeacher
from test_npt_twin_cpu import _system

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_twins_unmasked.npz")


@pytest.mark.parametrize("kw", [dict(), dict(fixed=None), dict(fixed="atoms"), dict(fixed="components")],
                         ids=["no-keyword", "none", "all-false-atoms", "all-false-components"])
def test_without_a_mask_the_twins_keep_their_bits(kw):
    gold = np.load(GOLDEN)
    if isinstance(kw.get("fixed"), str):
        kw = dict(fixed=np.zeros(27, bool) if kw["fixed"] == "atoms" else np.zeros((27, 3), bool))
    got = _walks(**kw)
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        assert np.array_equal(got[k], gold[k]), k


def test_langevin_holds_the_mask_and_the_free_components_draw_what_they_drew():
    """Springs couples no two components: the free components of the constrained run are those of the unconstrained one bit for
    bit exactly when they are fed the same deviates — the stream is consumed as before, the held entries unused."""
    numbers, pos, cell, v, calc = _toy()
    N = len(numbers)
    fx = _mask(N)

    class Counting:
        def __init__(self, seed):
            self.rng, self.sizes = np.random.default_rng(seed), []

        def normal(self, size=None):
            self.sizes.append(size)
            return self.rng.normal(size=size)

    ra, rb = Counting(11), Counting(11)
    free = [(p.copy(), w.copy()) for _, _, _, _, p, w in langevin_nvt(calc, numbers, pos, cell, [True] * 3, 40, 300.0, 1.0, 0.05, vel=v, rng=ra)]
    held = [(p.copy(), w.copy(), T) for _, _, T, _, p, w in langevin_nvt(calc, numbers, pos, cell, [True] * 3, 40, 300.0, 1.0, 0.05, vel=v, rng=rb,
                                                                        fixed=fx)]
    assert ra.sizes == rb.sizes == [(N, 3)] * 40
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    for (p0, v0), (p1, v1, T) in zip(free, held):
        assert np.array_equal(p1[fx], pos[fx])                       # the bits they started with
        assert np.array_equal(v1[fx], np.zeros(fx.sum())) and not np.signbit(v1[fx]).any()
        assert np.array_equal(p1[~fx], p0[~fx]) and np.array_equal(v1[~fx], v0[~fx])
        assert T == float((mass * v1 ** 2).sum() / ((3 * N - fx.sum()) * kB))
    assert np.abs(free[-1][0][fx] - pos[fx]).min() > 0               # (unconstrained, they all moved)
    # [N] flags hold whole atoms
    whole = fx.all(axis=1)
    last = list(langevin_nvt(calc, numbers, pos, cell, [True] * 3, 5, 300.0, 1.0, 0.05, vel=v, seed=2, fixed=whole))[-1]
    assert np.array_equal(last[4][whole], pos[whole]) and np.abs(last[4][~whole] - pos[~whole]).min() > 0
    with pytest.raises(ValueError):
        next(langevin_nvt(calc, numbers, pos, cell, [True] * 3, 5, fixed=np.zeros((N, 2), bool)))


def test_nose_hoover_holds_the_mask_and_settles_over_the_remaining_degrees_of_freedom():
    """The bound: the instantaneous temperature of g degrees of freedom fluctuates by sqrt(2 / g) of its mean (canonical); the
    1000 steps averaged are some 1000 / tdamp = 40 independent samples, so the mean is within sqrt(2 / g) / sqrt(40) = 0.03 for
    g = 60: four of these, 0.12.  Counting all 3N degrees of freedom instead would read 0.74 T."""
    numbers, pos, cell, mass, v = _system(temperature=300.0)
    N = len(numbers)
    fx = _mask(N)
    g = 3 * N - int(fx.sum())
    assert 55 <= g <= 62
    T, tdamp, steps = 300.0, 25.0, 1500
    calc = PairTeacher(rc=4.0)
    Ts, H = [], []
    tfact = 2.0 / (g * kB * T * (tdamp * FS) ** 2)
    for n, E, Tk, _, p, w, zeta, zint in nose_hoover_nvt(calc, numbers, pos, cell, [True] * 3, steps, T, 1.0, tdamp, vel=v, fixed=fx):
        assert np.array_equal(p[fx], pos[fx])
        assert np.array_equal(w[fx], np.zeros(fx.sum()))
        ke = 0.5 * float((mass[:, None] * w * w).sum())
        assert abs(Tk - 2.0 * ke / (g * kB)) <= 1e-12 * max(Tk, 1.0)
        Ts.append(Tk)
        H.append(E + ke + zeta * zeta / tfact + 2.0 * (0.5 * g * kB * T) * zint)   # (printed: the GPU test holds it to a bound)
    mean = float(np.mean(Ts[500:]))
    print("mean temperature over g degrees of freedom", mean, "extended energy: max drift", np.abs(np.array(H) - H[0]).max())
    assert abs(mean - T) < 0.12 * T, mean


def _constraints(kind, fx):
    if kind == "FixAtoms":
        whole = fx.all(axis=1)
        return [FixAtoms(mask=whole)], np.repeat(whole[:, None], 3, axis=1)
    if kind == "FixCartesian":
        idx = np.nonzero(fx[:, 0] & ~fx[:, 1] & ~fx[:, 2])[0]
        m = np.zeros_like(fx)
        m[idx, 0] = True
        return [FixCartesian(idx, [True, False, False])], m
    return constraints_from_mask(fx), fx


@pytest.mark.parametrize("kind,cell_relax", [("FixAtoms", False), ("FixCartesian", False), ("both", False), ("FixAtoms", True)],
                         ids=["FixAtoms", "FixCartesian", "both", "FixAtoms-UnitCellFilter"])
def test_fire_twin_is_fire_on_constrained_atoms(kind, cell_relax):
    """The frame, tolerances and the 60 evaluations of test_relax_twin_cpu.py: cl/relax.py's FIRE (and UnitCellFilter) on shim
    Atoms that carry the constraints against fire_relax(fixed=): same branch decisions, positions and cell to rounding."""
    numbers, pos, cell, mass, v = _system(shear=True)
    pos, cell = 1.04 * pos, 1.04 * cell
    N = len(numbers)
    cons, fx = _constraints(kind, _mask(N))
    assert fx.any()
    at = Atoms(numbers, pos, cell, True, constraint=cons)
    at.calc = PairTeacher(rc=4.0)
    target = UnitCellFilter(at) if cell_relax else at
    opt = FIRE(target)
    seen, n = set(), 0
    for o in fire_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, 60, 1e-6, cell_relax=cell_relax, fixed=fx):
        assert o["n"] == n and not o["converged"]
        f = target.get_forces()
        np.testing.assert_allclose(at.positions, o["positions"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(at.cell, o["cell"], rtol=0, atol=1e-10)
        assert abs(at.get_potential_energy() - o["energy"]) < 1e-9
        assert abs((f ** 2).sum(axis=1).max() - o["gmax2"]) < 1e-12
        if cell_relax:   # the held atoms keep their undeformed coordinate: x = r D^T in the twin's own operations
            DT = [[o["D"][b][a] for b in range(3)] for a in range(3)]
            assert np.array_equal(o["positions"][fx], _row_mul(pos, DT)[fx])
        else:
            assert np.array_equal(o["positions"][fx], pos[fx])
        opt.step(f)
        assert (opt.nsteps, opt.dt, opt.a) == (o["nsteps"], o["dt"], o["a"]), (n, opt.nsteps, opt.dt, opt.a, o["nsteps"], o["dt"], o["a"])
        seen.add((o["dt"], o["a"]))
        n += 1
    assert n == 61 and len(seen) > 5
    if cell_relax:
        assert np.abs(o["cell"] - cell).max() > 1e-6 and np.abs(o["positions"][fx] - pos[fx]).max() > 1e-6   # they followed the cell


def test_fire_convergence_is_judged_on_the_free_components():
    numbers, pos, cell, v, calc = _toy()
    N = len(numbers)
    fx = _mask(N)
    rows = list(fire_relax(calc, numbers, pos, cell, [True] * 3, 400, 1e-3, fixed=fx))
    assert rows[-1]["converged"] and len(rows) < 400
    at = Atoms(numbers, rows[-1]["positions"], cell, True)
    F = calc.get_property("forces", at)
    assert (F[fx] ** 2).max() > 1e-3 ** 2 > rows[-1]["gmax2"]          # a held component still carries a force above fmax
    assert np.array_equal(rows[-1]["positions"][fx], pos[fx])
    G = np.where(fx, 0.0, F)
    assert rows[-1]["gmax2"] == float(((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]).max())


def test_shim_constraints():
    numbers, pos, cell, mass, v = _system()
    N = len(numbers)
    a = Atoms(numbers, pos, cell, True, velocities=v, masses=mass)
    assert a.constraints == [] and a.get_number_of_degrees_of_freedom() == 3 * N
    T0 = a.get_temperature()
    assert T0 == 2.0 * a.get_kinetic_energy() / (3.0 * N * kB)
    fa, fc = FixAtoms(indices=[1, 4]), FixCartesian([2, 7], mask=(False, True, True))
    assert fa.get_removed_dof(a) == 6 and fc.get_removed_dof(a) == 4
    assert np.array_equal(FixAtoms(mask=np.arange(N) < 2).index, [0, 1])
    with pytest.raises(ValueError):
        FixAtoms()
    a.set_constraint([fa, fc])
    held = np.zeros((N, 3), bool)
    held[[1, 4]] = True
    held[[2, 7], 1:] = True
    ones = np.ones((N, 3))
    for c in a.constraints:
        c.adjust_forces(a, ones)
    assert np.array_equal(ones == 0.0, held)
    a.set_positions(pos + 1.0)
    assert np.array_equal(a.positions[held], pos[held]) and np.array_equal(a.positions[~held], (pos + 1.0)[~held])
    a.set_positions(pos + 2.0, apply_constraint=False)
    assert np.array_equal(a.positions, pos + 2.0)
    a.set_velocities(v)
    assert np.array_equal(a.get_velocities()[held], np.zeros(held.sum())) and np.array_equal(a.get_velocities()[~held], v[~held])
    assert a.get_number_of_degrees_of_freedom() == 3 * N - 10
    assert a.get_temperature() == 2.0 * a.get_kinetic_energy() / ((3 * N - 10) * kB)
    c = Atoms(numbers, pos, cell, True, velocities=v, masses=mass, constraint=[fa, fc])   # (as ase.Atoms: set under the constraints)
    assert np.array_equal(c.get_velocities(), a.get_velocities()) and c.get_temperature() == a.get_temperature()
    a.calc = PairTeacher(rc=4.0)
    F = a.get_forces()
    raw = a.get_forces(apply_constraint=False)
    assert np.array_equal(F[held], np.zeros(held.sum())) and np.array_equal(F[~held], raw[~held]) and np.abs(raw[held]).min() > 0
    assert np.array_equal(a.calc.results["forces"], raw)               # the calculator's own results stay raw
    b = a.copy()
    assert [type(c).__name__ for c in b.constraints] == ["FixAtoms", "FixCartesian"] and b.constraints[0] is not a.constraints[0]
    a.set_constraint()
    assert a.constraints == [] and len(b.constraints) == 2
    back = constraints_from_mask(held)
    ones = np.ones((N, 3))
    for c in back:
        c.adjust_forces(None, ones)
    assert np.array_equal(ones == 0.0, held) and constraints_from_mask(np.zeros((N, 3), bool)) is None


def test_the_mask_is_derived_from_what_the_constraints_do():
    from autoforce_amd.calculator import ActiveCalculator
    numbers, pos, cell, mass, v = _system()
    N = len(numbers)
    a = Atoms(numbers, pos, cell, True)
    assert ActiveCalculator.constraint_mask(a) is None
    a.set_constraint([FixAtoms(indices=[0, 3]), FixCartesian([5], mask=(True, False, False))])
    want = np.zeros((N, 3), bool)
    want[[0, 3]] = True
    want[5, 0] = True
    assert np.array_equal(ActiveCalculator.constraint_mask(a), want)

    # a FixCartesian whose stored flags mean the opposite (True = free, as older ASE kept them): the mask follows adjust_forces
    Old = type("FixCartesian", (), dict(__init__=lambda self, i, free: (setattr(self, "a", i), setattr(self, "mask", np.asarray(free, bool)))[0],
                                        adjust_forces=lambda self, atoms, f: f.__setitem__(self.a, np.where(self.mask, f[self.a], 0.0))))
    a.set_constraint(Old(6, (True, True, False)))
    want = np.zeros((N, 3), bool)
    want[6, 2] = True
    assert np.array_equal(ActiveCalculator.constraint_mask(a), want)

    class FixBondLength:
        def adjust_forces(self, atoms, f):
            f[:2] = 0.0
    a.set_constraint([FixAtoms(indices=[0]), FixBondLength()])
    with pytest.raises(NotImplementedError, match="FixBondLength"):
        ActiveCalculator.constraint_mask(a)


def test_run_md_and_run_relax_fall_back_to_the_twins_with_the_mask(tmp_path):
    """On an engine without a device loop run_md integrates through the host twins and run_relax through cl/relax.py's FIRE on
    the atoms themselves: the constraints go with them."""
    import active_common as ac
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import OracleModel
    from oracle import oracle as orc
    orc.set_num_threads(1)   # (a fixed summation order in the CPU engine: the two loops are compared bit for bit)
    try:
        _fall_back(tmp_path, ac, ActiveCalculator, OracleModel)
    finally:
        orc.set_num_threads(os.cpu_count() or 1)


def _fall_back(tmp_path, ac, ActiveCalculator, OracleModel):
    held, steps = [0, 5, 9], 6

    def make(name):
        np.random.seed(7)
        rng0, numbers, pos, cell = ac.start(0)
        (tmp_path / name).mkdir()
        calc = ActiveCalculator(engine=OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                                logfile=str(tmp_path / name / "active.log"), pckl=None, tape=None, **ac.KW)
        return calc, numbers, pos, cell

    vel = 0.02 * np.random.default_rng(3).normal(size=(18, 3))
    fx = np.zeros((18, 3), bool)
    fx[held] = True
    for kw, twin in ((dict(friction=0.02), lambda c, n, p, h: langevin_nvt(c, n, p, h, True, steps, 300.0, 1.0, 0.02, vel=vel,
                                                                          rng=np.random.default_rng(9), fixed=fx)),
                     (dict(tdamp_fs=20.0), lambda c, n, p, h: nose_hoover_nvt(c, n, p, h, True, steps, 300.0, 1.0, 20.0, vel=vel, fixed=fx))):
        calc, numbers, pos, cell = make("run" + str(len(kw)) + next(iter(kw)))
        assert not calc.md_on_device_ok()
        at = Atoms(numbers, pos, cell, True, velocities=vel, constraint=FixAtoms(indices=held))
        out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, rng=np.random.default_rng(9), **kw))
        assert len(out) == steps + 1
        assert np.array_equal(at.positions[held], pos[held]) and np.array_equal(at.get_velocities()[held], np.zeros((3, 3)))
        assert np.abs(at.positions[~fx] - pos[~fx]).min() > 0
        assert abs(at.get_temperature() - out[-1][2]) <= 1e-9 * out[-1][2]          # the yield's temperature is over g
        calc2, numbers, pos, cell = make("twin" + next(iter(kw)))
        rows = [(E, T, p.copy()) for _, E, T, _, p, *rest in twin(calc2, numbers, pos, cell)]
        assert [o[1] for o in out] == [r[0] for r in rows] and [o[2] for o in out] == [r[1] for r in rows]
        assert np.array_equal(at.positions, rows[-1][2]) and calc.size == calc2.size
        # the log lines too, the first one included: the held velocities the caller handed over are dropped before anything is logged
        logs = [[ln.split(" ", 2)[2] for ln in open(tmp_path / d / "active.log").read().splitlines()]
                for d in ("run" + str(len(kw)) + next(iter(kw)), "twin" + next(iter(kw)))]
        assert len(logs[0]) > steps and logs[0] == logs[1]
    calc, numbers, pos, cell = make("relax")
    at = Atoms(numbers, pos, cell, True, constraint=[FixAtoms(indices=held), FixCartesian([11], [False, False, True])])
    res = calc.run_relax(at, fmax=0.05, steps=8)
    assert res["evaluations"] >= 2
    assert np.array_equal(at.positions[held], pos[held]) and at.positions[11, 2] == pos[11, 2] and at.positions[11, 0] != pos[11, 0]
    at.set_constraint(type("FixBondLength", (), dict(adjust_forces=lambda self, a, f: None))())
    with pytest.raises(NotImplementedError, match="FixBondLength"):
        calc.run_relax(at)
    with pytest.raises(NotImplementedError, match="FixBondLength"):
        next(calc.run_md(at, 2, 300.0))
