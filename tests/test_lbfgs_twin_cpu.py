"""CPU tests of workloads.lbfgs_relax and LbfgsTwin, the host twin and definition of L-BFGS inside the device relaxation
(md_lbfgs.inc): the direction p = H G of the compact representation (Byrd, Nocedal & Schnabel 1994) against the two-loop recursion
of ase/optimize/lbfgs.py (Nocedal 1980), written out here, over walks long enough for the window to slide; what a walk must keep
— an emptied history, held components, a masked cell, a skipped pair —; and ActiveCalculator.run_relax(optimizer="LBFGS") on its
host path.  The system of the walks is the sheared 27-atom cell of test_relax_twin_cpu.py stretched by 4 %."""
import numpy as np
import pytest

import active_common as ac
from autoforce_amd.ase_shim import Atoms
from autoforce_amd.calculator import ActiveCalculator
from autoforce_amd.workloads import LbfgsTwin, lbfgs_relax
from helpers import OracleModel, PairTeacher
from test_npt_twin_cpu import _system

# The twin rule: ten times the largest relative difference measured on the CPU between the compact form and the two-loop
# recursion, |p - z|_max / |z|_max, over the six walks of test_direction_is_the_two_loop_recursion (measured: 1.51e-15, at
# memory 3 with the cell rows; 5.7e-16 ... 1.2e-15 on the other five).
DIRECTION_RTOL = 1.51e-14
WALK = 30


def _start():
    numbers, pos, cell, mass, v = _system(shear=True)
    return numbers, 1.04 * pos, 1.04 * cell


def _two_loop(pairs, G, H0):
    """ase/optimize/lbfgs.py::LBFGS.step without line search: q = -f, the backward loop, z = H0 q, the forward loop, p = -z.
    pairs: (s, y) oldest first, y = g - g0 = G0 - G."""
    q = -G.reshape(-1)
    rho = [1.0 / np.dot(y.reshape(-1), s.reshape(-1)) for s, y in pairs]
    a = [0.0] * len(pairs)
    for i in range(len(pairs) - 1, -1, -1):
        s, y = pairs[i]
        a[i] = rho[i] * np.dot(s.reshape(-1), q)
        q = q - a[i] * y.reshape(-1)
    z = H0 * q
    for i in range(len(pairs)):
        s, y = pairs[i]
        b = rho[i] * np.dot(y.reshape(-1), z)
        z = z + s.reshape(-1) * (a[i] - b)
    return -z.reshape(G.shape)


def _force(X, A, x0):
    """Minus the gradient of a quartic bowl over the rows' 3R coordinates: f = 1/2 d^T A d + 1/4 sum d^4, d = X - x0."""
    d = (X - x0).reshape(-1)
    return -(A @ d + d ** 3).reshape(X.shape)


@pytest.mark.parametrize("cell", [False, True], ids=["rows", "rows+cell"])
@pytest.mark.parametrize("memory", [1, 3, 40])
def test_direction_is_the_two_loop_recursion(memory, cell):
    """300 rows (two workgroups of partial sums) — with `cell` three more that the sums add behind them —, 30 evaluations:
    the window of memory 1 and 3 slides, memory 40 never fills."""
    rng = np.random.default_rng(5)
    N = 300
    R = N + (3 if cell else 0)
    B = rng.normal(size=(3 * R, 24))
    A = B @ B.T / 24 + np.diag(rng.uniform(5.0, 90.0, size=3 * R))
    x0 = rng.normal(size=(R, 3))
    X = x0 + 0.3 * rng.normal(size=(R, 3))
    order = rng.permutation(N)
    tw = LbfgsTwin(N, order, memory, 70.0, cell=cell)
    pairs, worst, G0 = [], 0.0, None
    for n in range(WALK):
        G = _force(X, A, x0)
        ev = tw.evaluate(n, G)
        if n:
            pairs = (pairs + [(s, G0 - G)])[-memory:]
        assert ev["cnt"] == ev["pairs"] == len(pairs) == min(n, memory)
        p, pG = tw.direction()
        z = _two_loop(pairs, G, 1.0 / 70.0)
        rel = np.abs(p - z).max() / np.abs(z).max()
        worst = max(worst, rel)
        assert abs(pG - (z * G).sum()) <= 1e-12 * abs((z * G).sum())
        longest = np.sqrt((p ** 2).sum(axis=1).max())
        Xn = X + p * (0.2 / longest if longest >= 0.2 else 1.0)
        s = Xn - X
        tw.moved(n, s)
        X, G0 = Xn, G
    print("memory", memory, "cell", cell, "largest relative difference", worst, "|G| first, last", np.abs(_force(x0 + 0.3, A, x0)).max(), np.abs(G).max())
    assert worst <= DIRECTION_RTOL, worst
    assert np.abs(G).max() < 1e-2 * np.abs(_force(x0 + 0.3, A, x0)).max()   # the walk went somewhere


def test_a_skipped_pair_leaves_the_run_finite():
    """Two evaluations with the same forces: y = 0, s.y = 0 — ASE would divide by it.  The pair keeps its slot and is left out;
    the direction is that of the pairs that remain, and the walk goes on."""
    rng = np.random.default_rng(9)
    N = 40
    A = np.diag(rng.uniform(5.0, 90.0, size=3 * N))
    x0 = rng.normal(size=(N, 3))
    X = x0 + 0.2 * rng.normal(size=(N, 3))
    tw = LbfgsTwin(N, np.arange(N), 3, 70.0)
    pairs, G0 = [], None
    for n in range(8):
        G = G0 if n == 3 else _force(X, A, x0)        # evaluation 3 answers with the forces of evaluation 2
        ev = tw.evaluate(n, G)
        if n:
            pairs = (pairs + [(s, G0 - G, n != 3)])[-3:]
        assert ev["cnt"] == min(n, 3) and ev["pairs"] == sum(ok for _, _, ok in pairs)
        p, pG = tw.direction()
        assert np.isfinite(p).all() and np.isfinite(pG)
        z = _two_loop([(s_, y_) for s_, y_, ok in pairs if ok], G, 1.0 / 70.0)
        assert np.abs(p - z).max() <= DIRECTION_RTOL * np.abs(z).max()
        s = p.copy()
        tw.moved(n, s)
        X, G0 = X + s, G
    assert ev["pairs"] == 3                            # the skipped pair has left the window


def test_reset_held_components_and_the_masked_cell():
    numbers, pos, cell = _start()
    N = len(numbers)
    calc = PairTeacher(rc=4.0)
    kw = dict(memory=3, alpha=70.0)
    rows = [dict(o, positions=o["positions"].copy()) for o in lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 12, 1e-9, cell_relax=True, **kw)]
    assert [r["pairs"] for r in rows] == [0, 1, 2] + [3] * 10 and not rows[-1]["converged"]
    assert rows[-1]["pG"] == 0.0 and rows[-1]["scale"] == 0.0 and all(r["pG"] > 0.0 and 0.0 < r["scale"] <= 1.0 for r in rows[:-1])
    assert rows[-1]["energy"] < rows[0]["energy"] and np.count_nonzero(rows[-1]["D"]) == 9
    # a reset empties the history: the evaluations before it are untouched, the one behind it steps along H0 G
    again = [dict(o, positions=o["positions"].copy()) for o in lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 12, 1e-9, cell_relax=True,
                                                                            reset_at=(7,), **kw)]
    assert [r["pairs"] for r in again] == [0, 1, 2, 3, 3, 3, 3, 0, 1, 2, 3, 3, 3]
    assert all(np.array_equal(a["positions"], b["positions"]) and a["pG"] == b["pG"] for a, b in zip(again[:7], rows[:7]))
    assert np.array_equal(again[7]["positions"], rows[7]["positions"]) and again[7]["pG"] != rows[7]["pG"]
    assert not np.array_equal(again[8]["positions"], rows[8]["positions"])
    # held components take a zero step and keep their bits (constant cell: x is r)
    fixed = np.zeros((N, 3), bool)
    fixed[::4] = True
    fixed[1, 2] = True
    held = list(lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 10, 1e-9, fixed=fixed, **kw))
    assert all(np.array_equal(o["positions"][fixed], pos[fixed]) for o in held)
    assert all((o["positions"][~fixed] != pos[~fixed]).all() for o in held[1:])
    # ... and with the cell r keeps its bits while x = r D^T follows the cell
    heldc = list(lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 10, 1e-9, cell_relax=True, fixed=fixed, **kw))
    for o in heldc[1:]:
        r = np.linalg.solve(o["D"], o["positions"].T).T
        np.testing.assert_allclose(r[fixed], pos[fixed], rtol=0, atol=1e-12)
        assert not np.array_equal(o["positions"][fixed], pos[fixed])
    # the diagonal mask: the off-diagonal entries of D stay exactly 0
    diag = list(lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 10, 1e-9, cell_relax=True, mask=[1, 1, 1, 0, 0, 0], **kw))
    off = ~np.eye(3, dtype=bool)
    assert all(np.array_equal(o["D"][off], np.zeros(6)) for o in diag)
    assert np.abs(np.diag(diag[-1]["D"]) - 1.0).min() > 1e-6
    with pytest.raises(TypeError):
        next(lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 3, 0.01, dt=0.1))
    with pytest.raises(ValueError):
        next(lbfgs_relax(calc, numbers, pos, cell, [True] * 3, 3, 0.01, memory=129))


def test_lbfgs_converges_as_fire_does():
    """Both optimizers to fmax = 0.01 on the unstretched cell, positions only; the counts are printed, not asserted (L-BFGS
    without line search and without a curvature test is not always the quicker one on this soft pair potential)."""
    from autoforce_amd.workloads import fire_relax
    numbers, pos, cell, mass, v = _system(shear=True)
    lb = list(lbfgs_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, 400, 0.01))
    fi = list(fire_relax(PairTeacher(rc=4.0), numbers, pos, cell, [True] * 3, 400, 0.01))
    print("evaluations to fmax = 0.01: L-BFGS", len(lb), "FIRE", len(fi))
    assert lb[-1]["converged"] and fi[-1]["converged"] and lb[-1]["gmax2"] < 1e-4 <= min(r["gmax2"] for r in lb[:-1])
    assert len(lb) < 400 and all(not r["converged"] for r in lb[:-1])
    # (a minimum each, not necessarily the same one: the two walks end 0.013 eV apart here)
    assert lb[-1]["energy"] < lb[0]["energy"] - 0.1 and abs(lb[-1]["energy"] - fi[-1]["energy"]) < 0.05


def test_run_relax_with_lbfgs_on_the_host_path(tmp_path, monkeypatch):
    """ActiveCalculator.run_relax(optimizer="LBFGS") around the CPU engine — md_on_device_ok() says no: the host loop is
    lbfgs_relax around calculate() — on the PairTeacher frame of test_cl_cpu.py: the model learns on the way and the run ends
    converged.  The two-loop recursion alone, around the teacher, converges on this frame with the same keywords: checked first.
    clear_hist: a pair formed across a model update carries the jump of the forces in its y, and without a curvature test such
    pairs stall the walk until they leave the window — the history is emptied behind every update, as the reference's
    clear_hist does for its optimizers."""
    from autoforce_amd.cl.relax import force_max
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    rng0, numbers, pos, cell = ac.start(0)
    fmax, alpha = 0.1, 70.0
    at = Atoms(numbers, pos, cell, True)
    at.calc = PairTeacher(rc=4.0)
    pairs, G0, X = [], None, pos.copy()
    for n in range(200):
        at.positions = X
        G = at.get_forces()
        if force_max(G) < fmax:
            break
        if n:
            pairs = (pairs + [(s, G0 - G)])[-100:]
        p = _two_loop(pairs, G, 1.0 / alpha)
        longest = np.sqrt((p ** 2).sum(axis=1).max())
        s = (X + p * (0.2 / longest if longest >= 0.2 else 1.0)) - X
        X, G0 = X + s, G
    print("the two-loop recursion around the teacher converges behind", n, "moves")
    assert force_max(G) < fmax and n < 100
    calc = ActiveCalculator(engine=OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0), logfile="active.log", pckl=None,
                            tape=None, **ac.KW)
    atoms = Atoms(numbers, pos, cell, True)
    frames = []
    out = calc.run_relax(atoms, fmax=fmax, steps=200, optimizer="LBFGS", alpha=alpha, clear_hist=True, on_frame=lambda n, fr: frames.append(n))
    print(out, "model size", calc.size)
    assert out["converged"] and out["evaluations"] == out["steps"] + 1 <= 200
    assert frames == list(range(out["evaluations"]))
    assert calc.size[0] >= 1 and force_max(calc.results["forces"]) < fmax
    assert np.array_equal(atoms.positions, calc.atoms.positions) and atoms.get_potential_energy() == calc.results["energy"]
    with pytest.raises(ValueError):
        calc.run_relax(atoms, optimizer="BFGS")
