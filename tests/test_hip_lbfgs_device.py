"""GPU tests of L-BFGS inside the device relaxation (sgpr_md_relax_lbfgs: ase/optimize/lbfgs.py without line search on the
generalised coordinates of the FIRE loop, the product H G in the compact representation): md_lbfgs.inc's four kernels behind
every evaluation against their host twin workloads.lbfgs_relax around the same library, bit for bit — the sixteen scalars of
every evaluation, cell and deformation gradient of every configuration, the final state —, however the run is cut into calls;
held components; a covloss halt in the middle, resumed and reset; convergence as the third halt code; frames off the kernels'
grids; the error cases of sgpr_md_relax_lbfgs; the relaxation driver end to end.  Frame, model and helpers are those of
test_hip_npt_device.py.  Memory 3 throughout: the window slides and the slots wrap within a few evaluations."""
import numpy as np
import pytest

from test_hip_npt_device import _PredictCalc, _model

pytestmark = pytest.mark.gpu

EVALS = 30
FMAX = 1e-9   # (far below anything 30 evaluations reach on this frame: the bit-for-bit walks never converge)
LB = dict(optimizer="LBFGS", memory=3)


def _twin(mdl, numbers, pos, cell, pbc, evals=EVALS, fmax=FMAX, memory=3, **kw):
    """The twin's first `evals` evaluations and the configuration behind the last of them (evaluation `evals`)."""
    from autoforce_amd.workloads import lbfgs_relax
    calc = _PredictCalc(mdl)
    rows = []
    for o in lbfgs_relax(calc, numbers, pos, cell, pbc, evals, fmax, species=mdl.species, memory=memory, **kw):
        rows.append(dict(o, positions=o["positions"].copy()))
    return rows, np.array(calc.betas)


def _device(mdl, cuts):
    rows, cells, Ds = [], [], []
    for n in cuts:
        sc, code = mdl.md_run(n, None)
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        c, d = mdl.md_cells()
        assert len(c) == n
        rows.extend(sc)
        cells.extend(c)
        Ds.extend(d)
    return np.array(rows), np.array(cells), np.array(Ds)


def _same_rows(sc, host, cells=None, Ds=None):
    """Device scalars (and cells) of consecutive evaluations against the twin's rows, bit for bit."""
    dE = np.abs(sc[:, 0] - np.array([h["energy"] for h in host]))
    print("max |dE|", dE.max(), "first differing evaluation", np.nonzero(dE)[0][:1])
    assert [r[0] for r in sc] == [h["energy"] for h in host]
    for col, key in ((12, "gmax2"), (13, "pG"), (14, "scale"), (15, "pairs")):
        d = np.nonzero(sc[:, col] != np.array([float(h[key]) for h in host]))[0]
        assert not len(d), (key, d[:3], sc[d[:3], col], [host[i][key] for i in d[:3]])
    if cells is not None:
        assert np.array_equal(cells, np.array([h["cell"] for h in host]))
        assert np.array_equal(Ds, np.array([h["D"] for h in host]))


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True), dict(cell_relax=True, mask=[1, 1, 1, 0, 0, 0])],
                         ids=["positions", "cell", "cell-diagonal"])
def test_device_loop_is_the_twin_bit_for_bit(kw):
    mdl, (numbers, pos, cell, pbc) = _model()
    host, b = _twin(mdl, numbers, pos, cell, pbc, **kw)
    assert len(host) == EVALS + 1 and not host[-1]["converged"]
    out = {}
    for cuts in ((EVALS,), (7, 1, 10, 12)):
        mdl.relax_begin(numbers, pos, cell, pbc, FMAX, **LB, **kw)
        sc, cells, Ds = _device(mdl, cuts)
        _same_rows(sc, host[:EVALS], cells, Ds)
        assert np.array_equal(sc[:, 11], b[:EVALS])                 # the largest covloss of every evaluation
        st = mdl.md_state()
        assert np.array_equal(st["positions"], host[EVALS]["positions"])
        assert np.array_equal(st["cell"], host[EVALS]["cell"]) and np.array_equal(st["D"], host[EVALS]["D"])
        prev = mdl.md_state(which=-1)
        assert np.array_equal(prev["positions"], host[EVALS - 1]["positions"]) and np.array_equal(prev["cell"], host[EVALS - 1]["cell"])
        out[cuts] = (sc, cells, Ds, st["positions"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                 # however the run is cut into calls
    assert [h["pairs"] for h in host[:5]] == [0, 1, 2, 3, 3]        # the window has filled and slides
    assert all(h["pG"] != 0.0 and 0.0 < h["scale"] <= 1.0 for h in host[:EVALS])   # (every evaluation moved)
    if kw.get("cell_relax"):
        moved = np.abs(host[EVALS]["cell"] - cell)
        assert moved.max() > 1e-6
        if kw.get("mask"):
            off = ~np.eye(3, dtype=bool)
            assert np.array_equal(host[EVALS]["D"][off], np.zeros(6))
        else:
            assert np.count_nonzero(host[EVALS]["D"]) == 9          # a general cell
    else:
        assert np.array_equal(host[EVALS]["cell"], cell)
    mdl.close()


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True)], ids=["positions", "cell"])
def test_held_components_against_the_twin(kw):
    mdl, (numbers, pos, cell, pbc) = _model()
    N = len(numbers)
    fixed = np.zeros((N, 3), bool)
    fixed[::5] = True
    fixed[3, 1] = True
    evals = 12
    host, _ = _twin(mdl, numbers, pos, cell, pbc, evals=evals, fixed=fixed, **kw)
    mdl.relax_begin(numbers, pos, cell, pbc, FMAX, fixed=fixed, **LB, **kw)
    sc, cells, Ds = _device(mdl, (5, 7))
    _same_rows(sc, host[:evals], cells, Ds)
    st = mdl.md_state()
    assert np.array_equal(st["positions"], host[evals]["positions"])
    if not kw:
        assert np.array_equal(st["positions"][fixed], pos[fixed]) and (st["positions"][~fixed] != pos[~fixed]).all()
    mdl.close()


@pytest.mark.parametrize("reset", [False, True], ids=["resumed", "reset"])
def test_a_covloss_halt_returns_that_configuration_and_the_run_resumes(reset):
    mdl, (numbers, pos, cell, pbc) = _model()
    kw = dict(cell_relax=True)
    host, b = _twin(mdl, numbers, pos, cell, pbc, **kw)
    # the gate's evaluation, from the twin's covloss column alone: the first k >= 6 (the window is full and slides) whose covloss
    # exceeds the one before it; the gated call starts at the earliest k0 from which it is the largest so far
    rises = [j for j in range(6, EVALS - 2) if b[j] > b[j - 1]]
    assert rises, "the covloss never rises between evaluations 6 and 27 of this walk"
    k = rises[0]
    k0 = min(j for j in range(k) if b[j:k].max() < b[k])
    ediff = 0.5 * (b[k0:k].max() + b[k])
    if reset:   # the twin that empties its history in front of evaluation k
        host, _ = _twin(mdl, numbers, pos, cell, pbc, reset_at=(k,), **kw)
    mdl.relax_begin(numbers, pos, cell, pbc, FMAX, **LB, **kw)
    if k0:
        sc0, code = mdl.md_run(k0, None)
        assert code == 0 and [r[0] for r in sc0] == [h["energy"] for h in host[:k0]]
    sc1, code = mdl.md_run(EVALS, None, ediff=ediff)
    assert code == 1 and len(sc1) == k - k0 + 1, (code, len(sc1), k, k0)
    assert [r[0] for r in sc1] == [h["energy"] for h in host[k0:k + 1]] and sc1[-1, 11] == b[k]
    assert sc1[-1, 13] == 0.0 and sc1[-1, 14] == 0.0                # nothing moved
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[k]["positions"]) and np.array_equal(st["cell"], host[k]["cell"])
    assert st["energy"] == host[k]["energy"]
    if reset:
        mdl.relax_reset()
    sc2, code = mdl.md_run(EVALS - k, None)
    assert code == 0 and len(sc2) == EVALS - k
    c2, d2 = mdl.md_cells()
    _same_rows(sc2, host[k:EVALS], c2, d2)
    assert sc2[0, 15] == (0.0 if reset else 3.0)
    st2 = mdl.md_state()
    assert np.array_equal(st2["positions"], host[EVALS]["positions"]) and np.array_equal(st2["cell"], host[EVALS]["cell"])
    mdl.close()


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True)], ids=["positions", "cell"])
def test_convergence_is_the_third_halt_code(kw):
    """The threshold comes from the twin alone: the first evaluation k in 10..25 whose largest generalised force falls below every
    earlier one, and an fmax half-way between that value and the smallest earlier one."""
    mdl, (numbers, pos, cell, pbc) = _model()
    host, b = _twin(mdl, numbers, pos, cell, pbc, **kw)
    g = np.sqrt(np.array([h["gmax2"] for h in host]))
    ks = [k for k in range(10, 26) if g[k] < g[:k].min()]
    assert ks, "no evaluation in 10..25 undercuts all earlier ones on this walk: take another seed"
    k = ks[0]
    fmax = 0.5 * (g[k] + g[:k].min())
    twin, _ = _twin(mdl, numbers, pos, cell, pbc, fmax=fmax, **kw)
    assert len(twin) == k + 1 and twin[-1]["converged"]
    mdl.relax_begin(numbers, pos, cell, pbc, fmax, **LB, **kw)
    sc, code = mdl.md_run(EVALS, None)
    assert code == 3 and len(sc) == k + 1, (code, len(sc), k)
    c, d = mdl.md_cells()
    _same_rows(sc, twin, c, d)
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[k]["positions"]) and np.array_equal(st["cell"], host[k]["cell"])
    assert st["energy"] == host[k]["energy"]
    assert sc[-1, 12] < fmax * fmax and (sc[:-1, 12] >= fmax * fmax).all()
    sc, code = mdl.md_run(5, None)                # asked again, the converged configuration answers again: nothing moves
    assert code == 3 and len(sc) == 1 and sc[0, 0] == host[k]["energy"]
    mdl.close()


@pytest.mark.parametrize("N", [4099, 5])
def test_frames_off_the_kernels_grids(N):
    """N = 4099 (seventeen workgroups of partial sums, not a multiple of the 64 rows of md_lbfgs_dir_kernel's workgroups nor of
    the 256 of the others) and N = 5 (less than one wave), positions only, against the twin."""
    from autoforce_amd.workloads import lips
    mdl, _ = _model()
    side = 17 if N > 512 else 8   # (17^3 = 4913 sites)
    numbers, pos, cell, pbc = lips(side, seed=0)
    assert len(numbers) >= N
    if N == 5:   # five atoms that see each other: an atom in the middle of the frame and its four nearest
        keep = np.sort(np.argsort(np.linalg.norm(pos - pos[len(pos) // 2], axis=1))[:N])
    else:
        keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=N, replace=False))
    numbers, pos = numbers[keep], pos[keep]
    evals = 8
    host, _ = _twin(mdl, numbers, pos, cell, pbc, evals=evals)
    mdl.relax_begin(numbers, pos, cell, pbc, FMAX, **LB)
    sc, cells, Ds = _device(mdl, (3, 5))
    _same_rows(sc, host[:evals], cells, Ds)
    assert np.array_equal(mdl.md_state()["positions"], host[evals]["positions"])
    mdl.close()


def test_lbfgs_error_cases_leave_the_handle_working():
    from autoforce_amd import _lib
    mdl, (numbers, pos, cell, pbc) = _model()
    N = len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    lib = _lib.load()

    def lbfgs(memory=3, maxstep=0.2, alpha=70.0, damping=1.0):
        return lib.sgpr_md_relax_lbfgs(mdl.handle, int(memory), float(maxstep), float(alpha), float(damping))

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
    assert lbfgs() == _lib.E_INVALID                                               # before sgpr_md_relax
    works()
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    assert lbfgs(memory=0) == _lib.E_INVALID and lbfgs(memory=129) == _lib.E_INVALID
    assert lbfgs(maxstep=0.0) == _lib.E_INVALID and lbfgs(alpha=-1.0) == _lib.E_INVALID and lbfgs(damping=0.0) == _lib.E_INVALID
    works()
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)                                 # FIRE still, after the refusals
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2 and sc[0, 14] == 0.1                         # (column 14 of a FIRE row: dt)
    assert lbfgs() == _lib.E_INVALID                                               # the run has started
    works()
    with pytest.raises(TypeError):
        mdl.relax_begin(numbers, pos, cell, pbc, 0.05, optimizer="LBFGS", dt=0.1)  # a FIRE keyword
    with pytest.raises(ValueError):
        mdl.relax_begin(numbers, pos, cell, pbc, 0.05, optimizer="BFGS")
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05, cell_relax=True, optimizer="LBFGS", memory=128)   # and after all that, the real thing runs
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3 and list(sc[:, 15]) == [0.0, 1.0, 2.0]
    works()
    mdl.close()


def test_relaxation_driver_with_lbfgs_and_a_cell_runs_on_the_device(tmp_path, monkeypatch):
    """cl.relax.relax(algo="LBFGS", cell=True) end to end: the minimisation and the confirm loop go through run_relax with the
    optimizer named, the model learns on the way, the run ends below fmax with a cell that has moved, and the teacher's own forces
    there are small too.  clear_hist: the history is emptied behind every model update (a pair formed across an update carries
    the jump of the forces).  Every run is capped at 2000 moves: a walk that does not converge fails, it does not go on."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.cl.relax import UnitCellFilter, force_max, relax
    from helpers import PairTeacher
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    rng0, numbers, pos, cell = ac.start(0)
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0), logfile=None, pckl=None,
                            tape=None, **ac.KW)
    calls = []
    run_relax = calc.run_relax
    calc.run_relax = lambda *a, **k: (calls.append(k), run_relax(*a, **dict(k, steps=min(k["steps"], 2000))))[1]
    atoms = Atoms(numbers, pos, cell, True)
    n_exact = relax(atoms, fmax=0.1, cell=True, algo="LBFGS", trajectory="relax.xyz", rattle=0.02, clear_hist=True, calc=calc, seed=5)
    assert calls and all(k["cell"] and k["optimizer"] == "LBFGS" and k["clear_hist"] for k in calls) and calc.engine._md.get("relax")
    assert n_exact >= 1 and calc.size[0] >= 1
    assert np.abs(np.asarray(atoms.cell) - cell).max() > 1e-3
    assert force_max(UnitCellFilter(atoms).get_forces()) < 0.1         # the model's generalised forces on the final structure
    e_exact, f_exact = calc._test()
    assert force_max(f_exact) < 0.35, force_max(f_exact)
    assert open("relax.xyz").read().count("Lattice=") >= 1
    calc.engine.close()
