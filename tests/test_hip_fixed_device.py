"""GPU tests of held atoms and components inside the device loops (sgpr_md_fix: ase.constraints.FixAtoms / FixCartesian as a
per-component mask): finalize_next_kernel<4>, shard_next_kernel<4> and the FIX forms of md_fire_kernel / md_fire_move_kernel
against the host twins with `fixed=` around the same library, bit for bit — BAOAB Langevin with uploaded and with on-device
deviates, velocity Verlet, Nose-Hoover (zeta and its integral included), FIRE with and without a moving cell; every scalar row and
the final state, however the run is cut into md_run calls; a covloss halt and its resume —; an empty mask against the run without
one; the held coordinates against the uploaded ones and the reported forces against predict's; the generalised extended energy of
Nose-Hoover; convergence of FIRE judged on the free components; ActiveCalculator.run_md / run_relax on constrained atoms against
the twins around calculate(); two ranks on the one GPU against the single process; the error cases.  Frame, model and helpers
are those of test_hip_npt_device.py."""
import os

import numpy as np
import pytest

from test_hip_npt_device import _PredictCalc, _model

pytestmark = pytest.mark.gpu

STEPS, T, FRICTION = 60, 600.0, 0.05
CUTS = (7, 1, 20, 33)      # 61 evaluations in four calls, the last one `final`


def _mask(pos, seed=5):
    """The lowest quarter of the atoms in z held whole, single components of a dozen others."""
    N = len(pos)
    fx = np.zeros((N, 3), bool)
    order = np.argsort(pos[:, 2], kind="stable")
    fx[order[:N // 4]] = True
    rest = np.random.default_rng(seed).permutation(order[N // 4:])
    fx[rest[:5], 0] = True
    fx[rest[5:9], 2] = True
    fx[rest[9:12], :2] = True
    return fx


def _setup(scale=0.02):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS
    mdl, (numbers, pos, cell, pbc) = _model(scale=scale)
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return mdl, numbers, pos, cell, pbc, mass, vel, _mask(pos)


def _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=FRICTION, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=friction, kT=kB * T, **kw)


def _run(mdl, cuts, noise=None, steps=STEPS):
    rows = []
    for n in cuts:
        xi = None if noise is None else noise[len(rows):len(rows) + n]
        if xi is not None and len(xi) < n:   # (the last, `final` evaluation moves nothing)
            xi = np.concatenate([xi, np.zeros((n - len(xi),) + xi.shape[1:])])
        sc, code = mdl.md_run(n, xi, final=(len(rows) + n == steps + 1))
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
    return np.array(rows)


class _Rows:
    """A Generator stand-in that deals given rows of deviates to a host loop."""

    def __init__(self, xi):
        self.xi, self.k = xi, 0

    def normal(self, size):
        self.k += 1
        return self.xi[self.k - 1]


def _held_as_uploaded(mdl, numbers, pos, cell, pbc, fx):
    """At constant cell: the held coordinates are the uploaded bits, their velocities exactly zero, and the forces the state
    reports on them are the model's own (predict's), not zeros."""
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"][fx], pos[fx])
    assert np.array_equal(st["velocities"][fx], np.zeros(fx.sum())) and np.array_equal(st["velocities_pre"][fx], np.zeros(fx.sum()))
    ref = mdl.predict(numbers, st["positions"], cell, pbc)
    assert np.array_equal(st["forces"], ref["forces"]) and np.abs(st["forces"][fx]).min() > 0
    return st


@pytest.mark.parametrize("how", ["uploaded", "on-device", "verlet"])
def test_langevin_and_velocity_verlet_are_the_twin_bit_for_bit(how):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import langevin_nvt
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    g = 3 * N - int(fx.sum())
    friction = 0.0 if how == "verlet" else FRICTION
    out = {}
    for cuts in ((STEPS + 1,), CUTS):
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=friction, seed=77 if how == "on-device" else 0, fixed=fx)
        if how == "uploaded":
            xi = np.random.default_rng(9).normal(size=(STEPS, N, 3))
            sc = _run(mdl, cuts, noise=xi)
        else:
            sc = _run(mdl, cuts)
            xi = mdl.md_deviates(0, STEPS) if how == "on-device" else np.zeros((STEPS, N, 3))
        st = _held_as_uploaded(mdl, numbers, pos, cell, pbc, fx)
        out[cuts] = (sc[:, :14], st["positions"], st["velocities"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                   # however the run is cut into calls
    calc = _PredictCalc(mdl)
    host = [(E, Tk, p.copy(), v.copy()) for _, E, Tk, _, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=1.0, friction=friction, vel=vel, rng=_Rows(xi), fixed=fx)]
    sc, x, v = out[CUTS]
    assert [r[0] for r in sc] == [h[0] for h in host]                 # energies: same positions, every evaluation
    assert np.array_equal(sc[:, 11], np.array(calc.betas))
    np.testing.assert_allclose(sc[:, 12] / (g * kB), [h[1] for h in host], rtol=1e-12)   # (the sum over atoms runs in another order)
    assert np.array_equal(x, host[-1][2]) and np.array_equal(v, host[-1][3])
    assert np.abs(x[~fx] - pos[~fx]).min() > 0
    mdl.close()


def test_langevin_twin_on_the_device_with_the_mask():
    """workloads.langevin_nvt_device(fixed=): the same random stream as the host loop, the temperature over g."""
    from autoforce_amd.workloads import langevin_nvt, langevin_nvt_device
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    calc = _PredictCalc(mdl)
    host = [(E, Tk, p.copy(), v.copy()) for _, E, Tk, _, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, 40, temperature=T, dt_fs=1.0, friction=FRICTION, seed=3, fixed=fx)]
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, 40, temperature=T, dt_fs=1.0, friction=FRICTION, seed=3, chunk=16, fixed=fx))
    assert [d[1] for d in dev] == [h[0] for h in host]
    np.testing.assert_allclose([d[2] for d in dev], [h[1] for h in host], rtol=1e-12)
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][2]) and np.array_equal(st["velocities"], host[-1][3])
    mdl.close()


def test_nose_hoover_is_the_twin_bit_for_bit_and_survives_a_halt():
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, nose_hoover_nvt
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N, tdamp = len(numbers), 20.0
    g = 3 * N - int(fx.sum())
    calc = _PredictCalc(mdl)
    host = [(E, Tk, p.copy(), v.copy(), z, zi) for _, E, Tk, _, p, v, z, zi in
            nose_hoover_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=1.0, tdamp_fs=tdamp, vel=vel, fixed=fx)]
    b = np.array(calc.betas)
    v0 = np.where(fx, 0.0, vel)
    out = {}
    for cuts in ((STEPS + 1,), CUTS):
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=tdamp * FS, fixed=fx)
        sc = _run(mdl, cuts)
        st = _held_as_uploaded(mdl, numbers, pos, cell, pbc, fx)
        out[cuts] = (sc, st["positions"], st["velocities"], st["velocities_pre"])
        assert [r[0] for r in sc] == [h[0] for h in host]
        assert np.array_equal(sc[:, 14], np.array([h[4] for h in host]))           # zeta
        assert np.array_equal(sc[:, 15], np.array([h[5] for h in host]))           # its integral
        assert np.array_equal(sc[:, 11], b)
        np.testing.assert_allclose(sc[:, 12] / (g * kB), [h[1] for h in host], rtol=1e-12)
        assert np.array_equal(st["positions"], host[-1][2]) and np.array_equal(st["velocities"], host[-1][3])
        assert np.array_equal(st["velocities_pre"], host[-2][3])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)
    assert np.abs(out[CUTS][0][:, 14]).max() > 0
    # a covloss halt in the middle and its resume
    later = np.nonzero(b > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    ediff = 0.5 * (b[:k].max() + b[k])
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=tdamp * FS, fixed=fx)
    sc1, code = mdl.md_run(STEPS + 1, None, ediff=ediff, final=True)
    assert code == 1 and len(sc1) == k + 1
    sth = mdl.md_state(results=True)
    assert np.array_equal(sth["positions"], host[k][2]) and np.array_equal(sth["velocities"], host[k][3])
    assert np.array_equal(sth["velocities_pre"], host[k - 1][3] if k else v0)
    assert np.array_equal(sth["positions"][fx], pos[fx])
    sc2, code = mdl.md_run(STEPS + 1 - k, None, ediff=0.0, final=True)
    assert code == 0 and [r[0] for r in sc2] == [h[0] for h in host[k:]]
    assert np.array_equal(sc2[:, 14], np.array([h[4] for h in host[k:]])) and np.array_equal(sc2[:, 15], np.array([h[5] for h in host[k:]]))
    st2 = mdl.md_state(results=True)
    assert np.array_equal(st2["positions"], host[-1][2]) and np.array_equal(st2["velocities"], host[-1][3])
    mdl.close()


def test_a_langevin_halt_and_its_resume_equal_the_twin():
    from autoforce_amd.workloads import langevin_nvt, langevin_nvt_device
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    calc = _PredictCalc(mdl)
    host = [(E, p.copy(), v.copy()) for _, E, _, _, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, 45, temperature=900.0, dt_fs=1.0, friction=FRICTION, seed=4, fixed=fx)]
    b = np.array(calc.betas)
    later = np.nonzero(b > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk; pick another seed"
    k = int(later[0])
    ediff = 0.5 * (b[:k].max() + b[k])
    seen = []
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, 45, temperature=900.0, dt_fs=1.0, friction=FRICTION, seed=4, ediff=ediff,
                                   chunk=64, on_halt=lambda model, state: seen.append(state), fixed=fx))
    assert len(seen) >= 1
    st = seen[0]
    assert np.array_equal(st["positions"], host[k][1]) and np.array_equal(st["velocities"], host[k][2])
    assert st["beta"].max() == b[k] >= ediff
    assert np.array_equal(st["forces"], mdl.predict(numbers, host[k][1], cell, pbc)["forces"])
    assert [d[1] for d in dev] == [h[0] for h in host]                 # the trajectory is the host's, halts or not
    mdl.close()


def test_an_empty_mask_is_the_run_without_one():
    from autoforce_amd import _lib
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    out = []
    for kw in (dict(), dict(fixed=np.zeros((N, 3), bool)), dict(fixed=np.zeros(N, bool)), "null"):
        for th in (dict(seed=5), dict(friction=0.0, ttime=20.0 * FS)):
            _begin(mdl, numbers, pos, cell, pbc, mass, vel, **(dict() if kw == "null" else kw), **th)
            if kw == "null":   # (too late for a mask behind a thermostat; before one, NULL is accepted and changes nothing)
                assert _lib.load().sgpr_md_fix(mdl.handle, None) == (_lib.E_INVALID if "ttime" in th else _lib.OK)
            sc = _run(mdl, (5, 16), steps=20)
            st = mdl.md_state(results=True)
            out.append((sc, st["positions"], st["velocities"]))
    for k in range(2, len(out)):
        for a, c in zip(out[k % 2], out[k]):
            assert np.array_equal(a, c)
    # ... and a relaxation
    rel = []
    for kw in (dict(), dict(fixed=np.zeros((N, 3), bool))):
        mdl.relax_begin(numbers, pos, cell, pbc, 1e-9, cell_relax=True, **kw)
        sc, code = mdl.md_run(12, None)
        assert code == 0
        rel.append((sc, mdl.md_state()["positions"]))
    assert np.array_equal(rel[0][0], rel[1][0]) and np.array_equal(rel[0][1], rel[1][1])
    mdl.close()


def test_nose_hoover_conserves_its_generalised_extended_energy():
    """E + KE + zeta^2 / tfact + 2 K0 int zeta dt with tfact = 2 / (g kT ttime^2), K0 = g kT / 2 over 1500 steps, held to the
    bounds of test_hip_md.py::test_nose_hoover_conserves_its_extended_energy (the drift below 2 % of what the thermostat moves,
    the temperature — over g — within 8 % of its target, the thermostat pumping at least half the missing kinetic energy)."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS, fit_to_teacher
    mdl, (numbers, pos, cell, pbc) = _model(scale=0.05)
    fit_to_teacher(mdl, numbers, pos, cell, pbc)
    mdl.set_weights(mdl.mu, choli=mdl.choli, vscale=mdl.make_vscale())
    N, Tt, tdamp = len(numbers), 600.0, 25.0
    fx = _mask(pos)
    g = 3 * N - int(fx.sum())
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(1).normal(size=(N, 3)) * np.sqrt(kB * 300.0 / mass[:, None])   # starts cold
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=0.0, kT=kB * Tt, ttime=tdamp * FS, fixed=fx)
    assert mdl.md_dof() == g
    rows = []
    while len(rows) < 1500:
        sc, code = mdl.md_run(min(500, 1500 - len(rows)), None)
        assert code in (0, 2)
        rows.extend(sc)
    sc = np.array(rows)
    ttime, kT = tdamp * FS, kB * Tt
    tfact, K0 = 2.0 / (g * kT * ttime * ttime), 0.5 * g * kT
    thermostat = sc[:, 14] ** 2 / tfact + 2.0 * K0 * sc[:, 15]
    H = sc[:, 0] + 0.5 * sc[:, 12] + thermostat
    Tk = sc[:, 12] / (g * kB)
    print("mean T", Tk[500:].mean(), "ptp thermostat", np.ptp(thermostat), "max drift", np.abs(H - H[0]).max())
    assert abs(Tk[500:].mean() - Tt) < 0.08 * Tt, Tk[500:].mean()
    assert np.ptp(thermostat) > 0.5 * 0.5 * g * kB * 300.0
    assert np.abs(H - H[0]).max() < 0.02 * np.ptp(thermostat), (np.abs(H - H[0]).max(), np.ptp(thermostat))
    assert np.array_equal(mdl.md_state()["positions"][fx], pos[fx])
    mdl.close()


def _fire_twin(mdl, numbers, pos, cell, pbc, evals, fmax, **kw):
    from autoforce_amd.workloads import fire_relax
    calc = _PredictCalc(mdl)
    rows = [dict(o, positions=o["positions"].copy()) for o in fire_relax(calc, numbers, pos, cell, pbc, evals, fmax, species=mdl.species, **kw)]
    return rows, np.array(calc.betas)


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True), dict(cell_relax=True, mask=[1, 1, 1, 0, 0, 0])],
                         ids=["positions", "cell", "cell-diagonal"])
def test_fire_is_the_twin_bit_for_bit(kw):
    from autoforce_amd.workloads import _m3_inv, _row_mul
    from test_hip_relax_device import _device, _same_rows
    mdl, (numbers, pos, cell, pbc) = _model()
    fx = _mask(pos)
    evals, fmax = 60, 1e-9
    host, b = _fire_twin(mdl, numbers, pos, cell, pbc, evals, fmax, fixed=fx, **kw)
    assert len(host) == evals + 1 and not host[-1]["converged"]
    out = {}
    for cuts in ((evals,), (7, 1, 20, 32)):
        mdl.relax_begin(numbers, pos, cell, pbc, fmax, fixed=fx, **kw)
        sc, cells, Ds = _device(mdl, cuts)
        _same_rows(sc, host[:evals], cells, Ds)
        assert np.array_equal(sc[:, 11], b[:evals])
        st = mdl.md_state()
        assert np.array_equal(st["positions"], host[evals]["positions"])
        assert np.array_equal(st["cell"], host[evals]["cell"]) and np.array_equal(st["D"], host[evals]["D"])
        assert np.array_equal(st["velocities_pre"][fx], np.zeros(fx.sum()))
        if kw.get("cell_relax"):   # the undeformed coordinate is what is held: x = r D^T follows the cell
            DT = [[st["D"][c][a] for c in range(3)] for a in range(3)]
            whole = fx.all(axis=1)                                    # all of r as uploaded: x = pos D^T in the loop's operations
            assert whole.sum() >= len(pos) // 4 and np.array_equal(st["positions"][whole], _row_mul(pos, DT)[whole])
            # A single held component of r sits in x = r D^T next to the atom's free ones, which have moved: recover
            # r = x D^-T.  x carries three roundings of terms up to max|r| |D|, the closed-form inverse a few more per entry and
            # the product three again, with |D|, |D^-1| within a few per cent of 1: 32 eps max|pos| bounds it with room to
            # spare, and is seven orders below what a free coordinate moves by.
            r = _row_mul(st["positions"], _m3_inv(DT))
            tol = 32 * np.finfo(float).eps * np.abs(pos).max()
            print("max |r - pos| held", np.abs(r[fx] - pos[fx]).max(), "bound", tol, "free", np.abs(r[~fx] - pos[~fx]).max())
            assert np.abs(r[fx] - pos[fx]).max() <= tol and np.abs(r[~fx] - pos[~fx]).max() > 1e6 * tol
            assert np.abs(st["positions"][fx] - pos[fx]).max() > 1e-8
        else:
            assert np.array_equal(st["positions"][fx], pos[fx])
        out[cuts] = (sc, cells, Ds, st["positions"], st["velocities_pre"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)
    assert len({(h["dt"], h["a"]) for h in host}) > 3
    free, _ = _fire_twin(mdl, numbers, pos, cell, pbc, 3, fmax, **kw)
    assert free[2]["energy"] != host[2]["energy"]                     # (the mask matters on this walk)
    mdl.close()


def test_fire_converges_on_the_free_components():
    """Halt code 3 while a held atom still carries a force above fmax.  The threshold comes from the twin alone, as in
    test_hip_relax_device.py: the first evaluation in 30..50 whose largest free |G_row| undercuts every earlier one."""
    from test_hip_relax_device import _same_rows
    mdl, (numbers, pos, cell, pbc) = _model()
    fx = _mask(pos)
    host, b = _fire_twin(mdl, numbers, pos, cell, pbc, 60, 1e-9, fixed=fx)
    gm = np.sqrt(np.array([h["gmax2"] for h in host]))
    ks = [k for k in range(30, 51) if gm[k] < gm[:k].min()]
    assert ks, "no evaluation in 30..50 undercuts all earlier ones on this walk: take another seed"
    k = ks[0]
    fmax = 0.5 * (gm[k] + gm[:k].min())
    twin, _ = _fire_twin(mdl, numbers, pos, cell, pbc, 60, fmax, fixed=fx)
    assert len(twin) == k + 1 and twin[-1]["converged"]
    mdl.relax_begin(numbers, pos, cell, pbc, fmax, fixed=fx)
    sc, code = mdl.md_run(60, None)
    assert code == 3 and len(sc) == k + 1, (code, len(sc), k)
    _same_rows(sc, twin)
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[k]["positions"]) and np.array_equal(st["positions"][fx], pos[fx])
    F = st["forces"]
    assert np.array_equal(F, mdl.predict(numbers, st["positions"], cell, pbc)["forces"])
    whole = fx.all(axis=1)
    print("fmax", fmax, "largest force on a held atom", np.sqrt((F[whole] ** 2).sum(axis=1).max()))
    assert (F[whole] ** 2).sum(axis=1).max() > fmax * fmax > sc[-1, 12]
    G = np.where(fx, 0.0, F)
    assert sc[-1, 12] == ((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]).max()
    mdl.close()


def _active(tmp, name):
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import PairTeacher
    d = tmp / name
    d.mkdir()
    np.random.seed(1234)
    rng0, numbers, pos, cell = ac.start(0)
    teacher = PairTeacher(rc=4.0)
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=teacher, logfile=str(d / "active.log"),
                            pckl=None, tape=None, **ac.KW)
    return calc, numbers, pos, cell, str(d / "active.log")


def _log(path):
    import re
    return [re.sub(r"^\S+ \S+ ", "", ln) for ln in open(path).read().splitlines()]


@pytest.mark.parametrize("nh", [False, True], ids=["langevin", "nose-hoover"])
def test_run_md_on_constrained_atoms_equals_the_twin_around_calculate(tmp_path, nh):
    import re
    from autoforce_amd.ase_shim import Atoms, FixAtoms
    from autoforce_amd.workloads import langevin_nvt, nose_hoover_nvt
    steps, held = 50, [0, 5, 9, 14]
    res = {}
    for mode in ("host", "device"):
        calc, numbers, pos, cell, log = _active(tmp_path, mode)
        fx = np.zeros((len(numbers), 3), bool)
        fx[held] = True
        vel = 0.02 * np.random.default_rng(3).normal(size=pos.shape)
        if mode == "host":
            loop = (nose_hoover_nvt(calc, numbers, pos, cell, True, steps, 300.0, 1.0, 20.0, vel=vel, species=calc.engine.species, fixed=fx) if nh else
                    langevin_nvt(calc, numbers, pos, cell, True, steps, 300.0, 1.0, 0.02, vel=vel, rng=np.random.default_rng(9), fixed=fx))
            out = []
            for st, E, Tk, _, p, v, *rest in loop:
                out.append((st, E, Tk, bool(calc.updated)))
                last = (p.copy(), v.copy())
        else:
            at = Atoms(numbers, pos, cell, True, velocities=vel, constraint=FixAtoms(indices=held))
            kw = dict(tdamp_fs=20.0) if nh else dict(friction=0.02, rng=np.random.default_rng(9))
            out = [(s, E, Tk, bool(u)) for s, E, Tk, u, w in calc.run_md(at, steps, 300.0, dt_fs=1.0, chunk=16, **kw)]
            assert calc.engine._md.get("fixed") is not None             # the device loop has run, with the mask
            last = (at.positions.copy(), at.get_velocities())
            assert np.array_equal(at.positions[held], pos[held]) and np.array_equal(last[1][held], np.zeros((len(held), 3)))
            assert abs(at.get_temperature() - out[-1][2]) <= 1e-9 * out[-1][2]      # the yield's temperature is over g
            assert np.abs(calc.results["forces"][held]).min() > 0       # the calculator's own results stay raw
        res[mode] = (out, last, calc.size, _log(log))
        calc.engine.close()
    (ho, hl, hs, hlog), (do, dl, ds, dlog) = res["host"], res["device"]
    assert hs == ds and hs[1] > 2, (hs, ds)
    assert [o[0] for o in ho] == [o[0] for o in do] and [o[3] for o in ho] == [o[3] for o in do]
    assert sum(o[3] for o in ho) >= 1 and sum(o[3] for o in ho) < steps // 2      # the model was updated, most steps ran without the host
    if nh:   # (the tolerances of test_run_md_nose_hoover_on_the_device_equals_the_host_loop)
        np.testing.assert_allclose([o[1] for o in do], [o[1] for o in ho], rtol=0, atol=1e-9)
        np.testing.assert_allclose(dl[0], hl[0], rtol=0, atol=1e-9)
        np.testing.assert_allclose(dl[1], hl[1], rtol=0, atol=1e-9)
        return
    assert [o[1] for o in ho] == [o[1] for o in do]
    np.testing.assert_allclose([o[2] for o in do], [o[2] for o in ho], rtol=1e-12)
    assert len(hlog) == len(dlog)
    num = re.compile(r"^(\d+) (\S+) (\S+) (\S+) $")
    for a, b in zip(hlog, dlog):
        ma, mb = num.match(a), num.match(b)
        if ma and mb:   # a step's line: energy and covloss bit for bit, the temperature (over g) to the order of its sum
            assert ma.group(1) == mb.group(1) and ma.group(2) == mb.group(2) and ma.group(4) == mb.group(4), (a, b)
            assert abs(float(ma.group(3)) - float(mb.group(3))) <= 1e-12 * max(float(ma.group(3)), 1e-300), (a, b)
        else:
            assert a == b
    assert np.array_equal(hl[0], dl[0]) and np.array_equal(hl[1], dl[1])


@pytest.mark.parametrize("cell_relax", [False, True], ids=["positions", "cell"])
def test_run_relax_on_constrained_atoms_equals_the_twin_around_calculate(tmp_path, cell_relax):
    from autoforce_amd.ase_shim import Atoms, FixAtoms
    from autoforce_amd.workloads import fire_relax
    steps, fmax, held = 40, 1e-3, [0, 5, 9, 14]
    res = {}
    for mode in ("host", "device"):
        calc, numbers, pos, cell, log = _active(tmp_path, mode)
        fx = np.zeros((len(numbers), 3), bool)
        fx[held] = True
        if mode == "host":
            for o in fire_relax(calc, numbers, pos, cell, True, steps, fmax, cell_relax=cell_relax, species=calc.engine.species, fixed=fx):
                last = (o["positions"].copy(), o["cell"].copy(), o["energy"], o["converged"])
            n_eval = o["n"] + 1
        else:
            at = Atoms(numbers, pos, cell, True, constraint=FixAtoms(indices=held))
            out = calc.run_relax(at, fmax=fmax, steps=steps, cell=cell_relax, chunk=16)
            assert calc.engine._md.get("relax") and calc.engine._md.get("fixed") is not None
            last = (at.positions.copy(), np.array(at.cell, float), float(calc.results["energy"]), out["converged"])
            n_eval = out["evaluations"]
            if not cell_relax:
                assert np.array_equal(at.positions[held], pos[held])
            assert np.abs(calc.results["forces"][held]).min() > 0
        res[mode] = (last, n_eval, calc._calc.calls, calc.size, _log(log))
        calc.engine.close()
    (hlast, hn, hcalls, hsize, hlog), (dlast, dn, dcalls, dsize, dlog) = res["host"], res["device"]
    assert hn == dn and hcalls == dcalls and hsize == dsize, (hn, dn, hcalls, dcalls, hsize, dsize)
    assert dcalls >= 1 and dsize[1] > 2
    assert hlog == dlog
    for a, b in zip(hlast, dlast):
        assert np.array_equal(a, b)


def _two_rank_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd.watchdog import Watchdog
    from test_hip_fixed_device import _sharded_runs
    from test_hip_peer import _build
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"constrained MD on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, system = _build()
        N = len(system[0])
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        q.put((rank, _sharded_runs(mdl, system, [3 + rank, 7, 100])))   # (every rank cuts the run differently)
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def _sharded_runs(mdl, system, batches, steps=40):
    """Seeded Langevin and Nose-Hoover with the mask, `steps` evaluations cut into `batches`: final states and scalars."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    numbers, pos, cell, pbc = system
    masses = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * 600.0 / masses)[:, None]
    fx = _mask(pos)
    out = []
    for th in (dict(friction=0.02, seed=11), dict(friction=0.0, ttime=20.0 * FS)):
        mdl.md_begin(numbers, pos, cell, pbc, masses, vel, dt=1.0 * FS, kT=kB * 600.0, fixed=fx, **th)
        rows, left = [], steps
        sizes = iter(list(batches) + [100] * 8)
        n = next(sizes)
        while left > 0:
            sc, code = mdl.md_run(min(n, left), None)
            assert code in (0, 2)
            rows.append(sc)
            left -= len(sc)
            if code == 0:
                n = next(sizes)
        st = mdl.md_state()
        out.append((st["positions"], st["velocities_pre"], np.concatenate(rows)))
    return out


def test_two_ranks_on_one_gpu_equal_the_single_process_bit_for_bit():
    """Patterned on test_hip_peer.py's sharded MD test: constrained Langevin (on-device deviates) and Nose-Hoover over the
    library's own exchange against the single process in scatter form."""
    import torch.multiprocessing as mp
    from test_hip_peer import _build
    mdl, system = _build(scatter=True)
    single = _sharded_runs(mdl, system, [100])
    fx = _mask(system[1])
    for x, v, sc in single:
        assert np.array_equal(x[fx], system[1][fx]) and np.array_equal(v[fx], np.zeros(fx.sum())) and np.abs(x[~fx] - system[1][~fx]).min() > 0
    mdl.close()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + ((os.getpid() + 57) % 250)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, runs in got:
        for (x, v, sc), (xs, vs, scs) in zip(runs, single):
            assert len(sc) == len(scs) == 40
            np.testing.assert_array_equal(x, xs)
            np.testing.assert_array_equal(v, vs)
            for col in (11, 12, 14, 15):                               # covloss, kinetic energy, zeta and its integral
                np.testing.assert_array_equal(sc[:, col], scs[:, col])
            np.testing.assert_allclose(sc[:, 0], scs[:, 0], rtol=0, atol=1e-11 * max(1.0, np.abs(scs[:, 0]).max()))


def test_error_cases_leave_the_handle_working():
    from autoforce_amd import SGPRModel, _lib
    from autoforce_amd.ase_shim import Atoms, FixAtoms, kB
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    lib = _lib.load()
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    m8 = np.ascontiguousarray(fx, dtype=np.uint8)
    ext = np.array([-1.0 * GPA] * 3 + [0.0] * 3)

    def fix(mask=m8):
        return lib.sgpr_md_fix(mdl.handle, _lib.ptr(mask))

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    fresh = SGPRModel(3, 3, 4, 6.0, species=mdl.species)
    assert lib.sgpr_md_fix(fresh.handle, _lib.ptr(m8)) == _lib.E_INVALID             # no run begun
    fresh.close()
    assert lib.sgpr_md_fix(None, _lib.ptr(m8)) == _lib.E_INVALID
    _begin(mdl, numbers, pos, cell, pbc, mass, vel)
    assert fix(np.ones((N, 3), np.uint8)) == _lib.E_INVALID                           # every component held
    assert fix() == _lib.OK and fix() == _lib.OK                                      # (may be repeated before anything else is set)
    assert lib.sgpr_md_thermostat(mdl.handle, 1, 25.0 * FS, kB * T) == _lib.OK
    assert fix() == _lib.E_INVALID                                                    # behind the thermostat
    assert lib.sgpr_md_barostat(mdl.handle, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0) == _lib.E_UNSUPPORTED   # a barostat with a mask
    works()
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=25.0 * FS)
    assert lib.sgpr_md_barostat(mdl.handle, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0) == _lib.OK              # (without one: fine)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel)
    sc, code = mdl.md_run(1, None, final=True)
    assert code == 0 and fix() == _lib.E_INVALID                                      # the run has started (t = 0 still)
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    assert fix() == _lib.E_INVALID                                                    # behind sgpr_md_relax
    works()
    with pytest.raises(NotImplementedError):
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=25.0 * FS, pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, fixed=fx)
    for bad in (np.zeros((N, 2), bool), np.zeros(N + 1, bool), np.zeros((N + 1, 3), bool)):
        with pytest.raises(ValueError):
            _begin(mdl, numbers, pos, cell, pbc, mass, vel, fixed=bad)
        with pytest.raises(ValueError):
            mdl.relax_begin(numbers, pos, cell, pbc, 0.05, fixed=bad)
    works()
    # the calculator: a barostat with constraints, a constraint of another kind
    calc = ActiveCalculator(engine=mdl, calculator=None, logfile=None, pckl=None, tape=None)
    at = Atoms(numbers, pos, cell, pbc, velocities=vel, constraint=FixAtoms(indices=[0, 1]))
    with pytest.raises(NotImplementedError, match="barostat"):
        next(calc.run_md(at, 3, T, tdamp_fs=25.0, pfactor=(100.0 * FS) ** 2 * 30.0 * GPA))

    class FixBondLength:
        def adjust_forces(self, atoms, f):
            pass
    at.set_constraint(FixBondLength())
    with pytest.raises(NotImplementedError, match="FixBondLength"):
        next(calc.run_md(at, 3, T))
    with pytest.raises(NotImplementedError, match="FixBondLength"):
        calc.run_relax(at)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, fixed=fx, seed=3)                 # and after all that, the real thing runs
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    works()
    mdl.close()
