"""GPU tests of the FIRE relaxation inside the device loop (sgpr_md_relax: ase/optimize/fire.py on the positions and, with
cell_relax, on the cell through ase.constraints.UnitCellFilter's coordinates): md_fire_kernel and md_fire_move_kernel behind
every evaluation against their host twin workloads.fire_relax around the same library, bit for bit — the sixteen scalars of
every evaluation, cell and deformation gradient of every configuration, the final state —; a covloss halt in the middle, with
and without a reset of the optimizer; convergence as the third halt code; the candidate lists kept under strain against a
handle that rebuilds them every step; frames off the kernels' grids; the error cases of sgpr_md_relax.  Frame, model and helpers
are those of test_hip_npt_device.py."""
import os

import numpy as np
import pytest

from test_hip_npt_device import _PredictCalc, _model

pytestmark = pytest.mark.gpu

EVALS = 60
FMAX = 1e-9   # (far below anything 60 evaluations reach on this frame: the bit-for-bit walks never converge)


def _twin(mdl, numbers, pos, cell, pbc, evals=EVALS, fmax=FMAX, **kw):
    """The twin's first `evals` evaluations and the configuration behind the last of them (evaluation `evals`)."""
    from autoforce_amd.workloads import fire_relax
    calc = _PredictCalc(mdl)
    rows = []
    for o in fire_relax(calc, numbers, pos, cell, pbc, evals, fmax, species=mdl.species, **kw):
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
    for col, key in ((12, "gmax2"), (13, "P"), (14, "dt"), (15, "a")):
        d = np.nonzero(sc[:, col] != np.array([h[key] for h in host]))[0]
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
    for cuts in ((EVALS,), (7, 1, 20, 32)):
        mdl.relax_begin(numbers, pos, cell, pbc, FMAX, **kw)
        sc, cells, Ds = _device(mdl, cuts)
        _same_rows(sc, host[:EVALS], cells, Ds)
        assert np.array_equal(sc[:, 11], b[:EVALS])                 # the largest covloss of every evaluation
        st = mdl.md_state()
        assert np.array_equal(st["positions"], host[EVALS]["positions"])
        assert np.array_equal(st["cell"], host[EVALS]["cell"]) and np.array_equal(st["D"], host[EVALS]["D"])
        prev = mdl.md_state(which=-1)
        assert np.array_equal(prev["positions"], host[EVALS - 1]["positions"]) and np.array_equal(prev["cell"], host[EVALS - 1]["cell"])
        out[cuts] = (sc, cells, Ds, st["positions"], st["velocities_pre"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                 # however the run is cut into calls
    branches = {(h["dt"], h["a"]) for h in host}
    assert len(branches) > 3                                        # the time step has been raised (and the walk is not trivial)
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


@pytest.mark.parametrize("reset", [False, True], ids=["resumed", "reset"])
def test_a_covloss_halt_returns_that_configuration_and_the_run_resumes(reset):
    mdl, (numbers, pos, cell, pbc) = _model()
    kw = dict(cell_relax=True)
    host, b = _twin(mdl, numbers, pos, cell, pbc, **kw)
    later = np.nonzero(b[:EVALS] > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    ediff = 0.5 * (b[:k].max() + b[k])
    if reset:   # the twin that re-initialises its optimizer in front of evaluation k
        host, _ = _twin(mdl, numbers, pos, cell, pbc, reset_at=(k,), **kw)
    mdl.relax_begin(numbers, pos, cell, pbc, FMAX, **kw)
    sc1, code = mdl.md_run(EVALS, None, ediff=ediff)
    assert code == 1 and len(sc1) == k + 1, (code, len(sc1), k)
    assert [r[0] for r in sc1] == [h["energy"] for h in host[:k + 1]] and sc1[k, 11] == b[k]
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[k]["positions"]) and np.array_equal(st["cell"], host[k]["cell"])
    assert st["energy"] == host[k]["energy"]
    if reset:
        mdl.relax_reset()
    sc2, code = mdl.md_run(EVALS - k, None)
    assert code == 0 and len(sc2) == EVALS - k
    c2, d2 = mdl.md_cells()
    _same_rows(sc2, host[k:EVALS], c2, d2)
    st2 = mdl.md_state()
    assert np.array_equal(st2["positions"], host[EVALS]["positions"]) and np.array_equal(st2["cell"], host[EVALS]["cell"])
    mdl.close()


@pytest.mark.parametrize("kw", [dict(), dict(cell_relax=True)], ids=["positions", "cell"])
def test_convergence_is_the_third_halt_code(kw):
    """The threshold comes from the twin alone: the first evaluation k in 30..50 whose largest generalised force falls below every
    earlier one, and an fmax half-way between that value and the smallest earlier one."""
    mdl, (numbers, pos, cell, pbc) = _model()
    host, b = _twin(mdl, numbers, pos, cell, pbc, **kw)
    g = np.sqrt(np.array([h["gmax2"] for h in host]))
    ks = [k for k in range(30, 51) if g[k] < g[:k].min()]
    assert ks, "no evaluation in 30..50 undercuts all earlier ones on this walk: take another seed"
    k = ks[0]
    fmax = 0.5 * (g[k] + g[:k].min())
    twin, _ = _twin(mdl, numbers, pos, cell, pbc, fmax=fmax, **kw)
    assert len(twin) == k + 1 and twin[-1]["converged"]
    mdl.relax_begin(numbers, pos, cell, pbc, fmax, **kw)
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


def test_lists_survive_the_strain():
    """The same walk with a zero skin (every step rebuilds its lists) gives the same bits; with the default skin the lists are
    rebuilt fewer times — the binning kernel's affine rule under the strain of a relaxing cell."""
    from autoforce_amd import _lib
    out = {}
    for skin0 in (False, True):
        mdl, (numbers, pos, cell, pbc) = _model()
        if skin0:
            _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 0))
        mdl.relax_begin(numbers, pos, cell, pbc, FMAX, cell_relax=True)
        r0 = mdl.list_rebuilds()
        sc, cells, Ds = _device(mdl, (EVALS,))
        st = mdl.md_state()
        out[skin0] = (sc, cells, Ds, st["positions"], st["velocities_pre"], mdl.list_rebuilds() - r0)
        mdl.close()
    fast, slow = out[False], out[True]
    print("rebuilds: default skin", fast[5], "zero skin", slow[5])
    for a, c in zip(fast[:5], slow[:5]):
        np.testing.assert_array_equal(a, c)
    assert slow[5] >= EVALS and fast[5] < slow[5], (fast[5], slow[5])


@pytest.mark.parametrize("N", [4099, 5])
def test_frames_off_the_kernels_grids(N):
    """N = 4099 (not a multiple of the move kernel's 64 atoms per workgroup, nor of the reduction's 256 threads) and N = 5
    (less than one wave), positions only, against the twin."""
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
    evals = 12
    host, _ = _twin(mdl, numbers, pos, cell, pbc, evals=evals)
    mdl.relax_begin(numbers, pos, cell, pbc, FMAX)
    sc, cells, Ds = _device(mdl, (5, 7))
    _same_rows(sc, host[:evals], cells, Ds)
    assert np.array_equal(mdl.md_state()["positions"], host[evals]["positions"])
    mdl.close()


def test_relax_error_cases_leave_the_handle_working():
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    mdl, (numbers, pos, cell, pbc) = _model()
    N = len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    lib = _lib.load()
    mass = np.array([MASS[int(z)] for z in numbers])

    def relax(fmax=0.05, move_cell=0):
        return lib.sgpr_md_relax(mdl.handle, float(fmax), None, int(move_cell), None)

    def begin(cell_=cell, pbc_=pbc, **kw):
        mdl.md_begin(numbers, pos, cell_, pbc_, mass, None, dt=1.0 * FS, friction=0.0, kT=kB * 300.0, **kw)

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    begin()
    assert relax(0.0) == _lib.E_INVALID and relax(-1.0) == _lib.E_INVALID          # fmax <= 0
    works()
    begin(ttime=25.0 * FS)
    assert relax() == _lib.E_INVALID                                               # a thermostat already set
    works()
    begin(pbc_=[True, True, False])
    assert relax(move_cell=1) == _lib.E_INVALID                                    # a moving cell with an open direction
    assert relax(move_cell=0) == _lib.OK
    works()
    flat = cell.copy()
    flat[2] = flat[0] + flat[1]
    begin(cell_=flat)
    assert relax(move_cell=1) == _lib.E_INVALID                                    # a singular cell
    works()
    begin()
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert relax() == _lib.E_INVALID                                               # the run has started
    works()
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert relax() == _lib.E_INVALID                                               # ... and so has a relaxation
    assert lib.sgpr_md_thermostat(mdl.handle, 1, 25.0 * FS, kB * 300.0) == _lib.E_INVALID
    works()
    with pytest.raises(TypeError):
        mdl.relax_begin(numbers, pos, cell, pbc, 0.05, timestep=0.1)
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05, cell_relax=True)                # and after all that, the real thing runs
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    works()
    mdl.close()


def _two_rank_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd import _lib
    from autoforce_amd.watchdog import Watchdog
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"relaxation on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_relax(mdl.handle, 0.05, None, 0, None)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_relaxation_and_goes_on_working():
    """A relaxation runs on one rank: sgpr_md_relax says SGPR_E_UNSUPPORTED on every rank and the handles go on predicting."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 250)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, e0, e1 in got:
        assert code == _lib.E_UNSUPPORTED and e0 == e1
    assert got[0][2] == got[1][2]


def test_run_relax_on_the_device_equals_the_host_loop(tmp_path):
    """ActiveCalculator.run_relax(cell=True) with the state on the device against the host loop (workloads.fire_relax around
    calculate()) of the same calculator class, an active calculator that learns from nothing: the gate fires, the same updates at
    the same evaluations, the same log line by line, the same number of teacher calls, the same final structure."""
    import re
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.workloads import PairTeacher, fire_relax
    steps, fmax = 40, 1e-3
    res = {}
    for mode in ("host", "device"):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        d = tmp_path / mode
        d.mkdir()
        teacher = PairTeacher(ac.SPECIES, rc=4.0)
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=teacher,
                                logfile=str(d / "active.log"), pckl=None, tape=None, **ac.KW)
        if mode == "host":
            for o in fire_relax(calc, numbers, pos, cell, True, steps, fmax, cell_relax=True, species=calc.engine.species):
                last = (o["positions"].copy(), o["cell"].copy(), o["energy"], o["converged"])
            n_eval = o["n"] + 1
        else:
            at = Atoms(numbers, pos, cell, True)
            assert calc.md_on_device_ok() or calc._needs_seed()
            out = calc.run_relax(at, fmax=fmax, steps=steps, cell=True, chunk=16)
            assert calc.engine._md.get("relax")                        # the device loop has run
            last = (at.positions.copy(), np.array(at.cell, float), float(calc.results["energy"]), out["converged"])
            n_eval = out["evaluations"]
            assert at.get_potential_energy() == last[2]                # the calculator answers for the final structure
        txt = open(d / "active.log").read().splitlines()
        res[mode] = (last, n_eval, teacher.calls, calc.size, [re.sub(r"^\S+ \S+ ", "", ln) for ln in txt])
        calc.engine.close()
    (hlast, hn, hcalls, hsize, hlog), (dlast, dn, dcalls, dsize, dlog) = res["host"], res["device"]
    assert hn == dn and hcalls == dcalls and hsize == dsize, (hn, dn, hcalls, dcalls, hsize, dsize)
    assert dcalls >= 1 and dsize[1] > 2                                # the gate fired and the model grew
    assert len(hlog) == len(dlog), next(((i, a, b) for i, (a, b) in enumerate(zip(hlog, dlog)) if a.split(" ")[:2] != b.split(" ")[:2]), None)
    for a, b in zip(hlog, dlog):
        assert a == b, (a, b)
    for a, b in zip(hlast, dlast):
        assert np.array_equal(a, b)
    assert np.abs(dlast[1] - ac.start(0)[3]).max() > 1e-6              # the cell has moved


def test_relaxation_driver_with_fire_and_a_cell_runs_on_the_device(tmp_path, monkeypatch):
    """cl.relax.relax(algo="FIRE", cell=True) end to end: the minimisation and the confirm loop go through run_relax, the model
    learns on the way, the run ends below fmax with a cell that has moved, and the teacher's own forces there are small too."""
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
    calc.run_relax = lambda *a, **k: (calls.append(k), run_relax(*a, **k))[1]
    atoms = Atoms(numbers, pos, cell, True)
    n_exact = relax(atoms, fmax=0.1, cell=True, algo="FIRE", trajectory="relax.xyz", rattle=0.02, calc=calc, seed=5)
    assert calls and all(k["cell"] for k in calls) and calc.engine._md.get("relax")
    assert n_exact >= 1 and calc.size[0] >= 1
    assert np.abs(np.asarray(atoms.cell) - cell).max() > 1e-3
    assert force_max(UnitCellFilter(atoms).get_forces()) < 0.1         # the model's generalised forces on the final structure
    e_exact, f_exact = calc._test()
    assert force_max(f_exact) < 0.35, force_max(f_exact)
    assert open("relax.xyz").read().count("Lattice=") >= 1
    calc.engine.close()
