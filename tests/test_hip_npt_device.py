"""GPU tests of the moving-cell dynamics inside the device MD loop (sgpr_md_barostat: ase.md.npt.NPT with a pfactor, what
cl/md.py:131-166 runs when a bulk modulus is given): md_npt_kernel behind every evaluation and the moving-cell form of the
step's last kernel against their host twin workloads.npt_moving_cell around the same library, bit for bit — energies,
thermostat, cell and strain rate of every evaluation, the final state, a covloss halt in the middle —; the candidate lists
kept under strain against a handle that rebuilds them every step; `iso` and `mask`; the extended system's conserved
quantity; ActiveCalculator.run_md(pfactor=...) against the twin around calculate(); the error cases of sgpr_md_barostat.
Frame, model and parameters are those of test_hip_md.py's moving-cell test around the device calculator."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS, T, TDAMP = 60, 600.0, 25.0


class _PredictCalc:
    """The library behind the three ASE getters (what ActiveCalculator.calculate does on a prediction-only step)."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, mdl):
        self.mdl, self.calls, self.betas = mdl, 0, []
        self._key, self.results = None, {}

    def get_property(self, name, atoms=None):
        key = atoms.positions.tobytes() + np.asarray(atoms.cell, float).tobytes()
        if key != self._key:
            out = self.mdl.predict(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc)
            self.results = dict(energy=float(out["energy"]), forces=np.array(out["forces"]), stress=np.array(out["stress"]),
                                free_energy=float(out["energy"]))
            self.betas.append(float(out["beta"].max()))
            self._key = key
            self.calls += 1
        return self.results[name]


def _model(side=8, m=48, scale=0.02, seed=1):
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, lips
    numbers, pos, cell, pbc = lips(side, seed=0)
    species = sorted(set(int(z) for z in numbers))
    mdl = SGPRModel(3, 3, 4, 6.0, species=species)
    n2, p2, c2, b2 = lips(side, seed=seed)
    mdl.set_inducing(inducing_from_frame(mdl, n2, p2, c2, b2, m, seed=seed))
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(64, m)), rng.normal(size=64))
    mdl.set_weights(scale * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
    return mdl, (numbers, pos, cell, pbc)


def _setup():
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS, MASS
    mdl, (numbers, pos, cell, pbc) = _model()
    mass = np.array([MASS[int(z)] for z in numbers])
    rng = np.random.default_rng(3)
    vel = rng.normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    baro = dict(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
    return mdl, numbers, pos, cell, pbc, mass, vel, baro


def _twin(mdl, numbers, pos, cell, pbc, vel, baro, steps=STEPS, **kw):
    from autoforce_amd.workloads import npt_moving_cell
    calc = _PredictCalc(mdl)
    host = [(s, E, Tk, p.copy(), v.copy(), h.copy(), e.copy(), z, zi) for s, E, Tk, w, p, v, h, e, z, zi in
            npt_moving_cell(calc, numbers, pos, cell, pbc, steps, temperature=T, dt_fs=1.0, tdamp_fs=TDAMP, vel=vel, **baro, **kw)]
    return host, np.array(calc.betas)


def _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=0.0, kT=kB * T, ttime=TDAMP * FS, **baro, **kw)


def _device_run(mdl, cuts, steps=STEPS):
    rows, cells, etas = [], [], []
    for n in cuts:
        sc, code = mdl.md_run(n, None, final=(len(rows) + n == steps + 1))
        assert code == 0 and len(sc) == n
        c, e = mdl.md_cells()
        assert len(c) == n
        rows.extend(sc)
        cells.extend(c)
        etas.extend(e)
    return np.array(rows), np.array(cells), np.array(etas)


def _gibbs(sc, cells, etas, N, baro, cell0):
    """npt.NPT.get_gibbs_free_energy from the scalars and cells the device loop returns."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    kT, ttime = kB * T, TDAMP * FS
    det = np.array([c[0, 0] * c[1, 1] * c[2, 2] for c in cells])
    pfact = 1.0 / (baro["pfactor"] * np.linalg.det(cell0))
    ext = -baro["externalstress"] * 3
    return (sc[:, 0] + 0.5 * sc[:, 12] - ext * det / 3.0 + 1.5 * N * kT * (ttime * sc[:, 14]) ** 2 + 3 * kT * (N - 1) * sc[:, 15]
            + 0.5 / pfact * (etas ** 2).sum(axis=(1, 2)))


def test_device_loop_is_the_twin_bit_for_bit_and_survives_a_halt():
    mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup()
    N = len(numbers)
    host, b = _twin(mdl, numbers, pos, cell, pbc, vel, baro)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro)
    sc, cells, etas = _device_run(mdl, (7, 1, 20, 33))
    assert len(sc) == STEPS + 1
    dE = np.abs(sc[:, 0] - np.array([h[1] for h in host]))
    dc = np.abs(cells - np.array([h[5] for h in host]))
    print("max |dE|", dE.max(), "first differing evaluation", (np.nonzero(dE)[0][:1], np.nonzero(dc.reshape(len(dc), -1).max(1))[0][:1]))
    assert [r[0] for r in sc] == [h[1] for h in host]
    assert np.array_equal(sc[:, 14], np.array([h[7] for h in host]))
    assert np.array_equal(sc[:, 15], np.array([h[8] for h in host]))
    assert np.array_equal(cells, np.array([h[5] for h in host]))
    assert np.array_equal(etas, np.array([h[6] for h in host]))
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][3]) and np.array_equal(st["velocities"], host[-1][4])
    assert np.array_equal(st["velocities_pre"], host[-2][4])
    assert np.array_equal(st["cell"], host[-1][5]) and np.array_equal(st["eta"], host[-1][6])
    assert np.abs(st["cell"] - cell).max() > 1e-4                              # the cell has moved
    # a covloss halt in the middle
    later = np.nonzero(b > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    ediff = 0.5 * (b[:k].max() + b[k])
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro)
    sc1, code = mdl.md_run(STEPS + 1, None, ediff=ediff, final=True)
    assert code == 1 and len(sc1) == k + 1
    sth = mdl.md_state(results=True)
    assert np.array_equal(sth["positions"], host[k][3]) and np.array_equal(sth["velocities"], host[k][4])
    assert np.array_equal(sth["cell"], host[k][5]) and np.array_equal(sth["eta"], host[k][6])
    assert np.array_equal(sth["velocities_pre"], host[k - 1][4] if k else host[0][4])
    sc2, code = mdl.md_run(STEPS + 1 - k, None, ediff=0.0, final=True)           # the halted configuration again, then on
    assert code == 0 and [r[0] for r in sc2] == [h[1] for h in host[k:]]
    assert np.array_equal(sc2[:, 14], np.array([h[7] for h in host[k:]]))
    c2, e2 = mdl.md_cells()
    assert np.array_equal(c2, np.array([h[5] for h in host[k:]])) and np.array_equal(e2, np.array([h[6] for h in host[k:]]))
    st2 = mdl.md_state(results=True)
    assert np.array_equal(st2["positions"], host[-1][3]) and np.array_equal(st2["velocities"], host[-1][4])
    assert np.array_equal(st2["cell"], host[-1][5])
    mdl.close()


def test_lists_survive_the_strain():
    """The same walk with a zero skin (every step rebuilds its lists through the binning kernel) gives the same bits; with the
    default skin the lists are rebuilt on at most a quarter of the steps (the bound the host path meets on this walk)."""
    from autoforce_amd import _lib
    out = {}
    for skin0 in (False, True):
        mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup()
        if skin0:
            _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 0))
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro)
        r0 = mdl.list_rebuilds()
        sc, cells, etas = _device_run(mdl, (STEPS + 1,))
        st = mdl.md_state(results=True)
        out[skin0] = (sc[:, 0], sc[:, 14], cells, etas, st["positions"], st["velocities"], mdl.list_rebuilds() - r0)
        mdl.close()
    fast, slow = out[False], out[True]
    print("rebuilds: default skin", fast[6], "zero skin", slow[6])
    for a, b in zip(fast[:6], slow[:6]):
        np.testing.assert_array_equal(a, b)
    assert slow[6] >= STEPS and fast[6] <= STEPS // 4, (fast[6], slow[6])


def test_iso_keeps_the_shape_mask_freezes_components_and_the_extended_energy_holds():
    mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup()
    N = len(numbers)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro)
    sc, cells, etas = _device_run(mdl, (STEPS + 1,))
    G = _gibbs(sc, cells, etas, N, baro, cell)
    print("ptp G", np.ptp(G), "G0", G[0])
    assert np.ptp(G) < 0.05 * max(abs(G[0]), 1.0)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro, iso=True)
    sc, cells, etas = _device_run(mdl, (STEPS + 1,))
    c = cells[-1]
    assert c[2, 2] != cell[2, 2]
    np.testing.assert_allclose(c / c[2, 2], cell / cell[2, 2], rtol=0, atol=1e-12)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, baro, mask=(0, 0, 1))
    sc, cells, etas = _device_run(mdl, (STEPS + 1,))
    c = cells[-1].copy()
    assert c[2, 2] != cell[2, 2]
    c[2, 2] = cell[2, 2]
    np.testing.assert_array_equal(c, cell)
    mdl.close()


def test_barostat_error_cases_leave_the_handle_working():
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup()
    ref = mdl.predict(numbers, pos, cell, pbc)
    e0 = float(ref["energy"])
    lib = _lib.load()
    ext = np.array([-baro["externalstress"]] * 3 + [0.0] * 3)

    def barostat(pfactor=baro["pfactor"]):
        return lib.sgpr_md_barostat(mdl.handle, float(pfactor), _lib.ptr(ext), None, 1.0)

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    kw = dict(dt=1.0 * FS, friction=0.0, kT=kB * T, ttime=TDAMP * FS)
    bad = cell.copy()
    bad[1, 0] = 0.05
    mdl.md_begin(numbers, pos, bad, pbc, mass, vel, **kw)
    assert barostat() == _lib.E_INVALID                   # not upper triangular
    works()
    with pytest.raises(_lib.SgprError):
        mdl.md_begin(numbers, pos, bad, pbc, mass, vel, **baro, **kw)      # ... and as the Python surface reports it
    works()
    mdl.md_begin(numbers, pos, cell, [True, True, False], mass, vel, **kw)
    assert barostat() == _lib.E_INVALID                   # an open direction
    works()
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **kw)
    assert barostat(0.0) == _lib.E_INVALID and barostat(-1.0) == _lib.E_INVALID
    works()
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **kw)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert barostat() == _lib.E_INVALID                   # the run has started
    works()
    with pytest.raises(ValueError):
        mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, kT=kB * T, **baro)   # a barostat without a thermostat
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **baro, **kw)        # and after all that, the real thing runs
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    mdl.close()


def test_run_md_with_a_barostat_on_the_device_equals_the_host_loop(tmp_path):
    """ActiveCalculator.run_md(tdamp_fs=..., pfactor=...) with the state on the device against the host loop
    (workloads.npt_moving_cell around calculate()) of the same calculator class: first an active calculator that learns from
    nothing — its gate fires, the same updates at the same steps, the same log line by line —, then the same calculator
    without its teacher (evaluate only).  With sync_every = 4 atoms.positions AND atoms.cell at every yielded multiple of 4 are
    that configuration's; atoms.cell at the end is the twin's."""
    import re
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS, npt_moving_cell
    from helpers import PairTeacher
    steps = (40, 20)
    baro = dict(pfactor=(75.0 * FS) ** 2 * 40.0 * GPA, externalstress=1.0 * GPA)
    res = {}
    for mode in ("host", "device"):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        d = tmp_path / mode
        d.mkdir()
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                                logfile=str(d / "active.log"), pckl=None, tape=None, **ac.KW)
        vel = 0.02 * np.random.default_rng(3).normal(size=pos.shape)
        legs = []
        for leg, n in enumerate(steps):
            if leg == 1:
                calc._calc = None                      # evaluate only: the gate never fires
                assert not calc.active
            out, sync = [], {}
            if mode == "host":
                for st, E, Tk, _, p, v, h, e, z, zi in npt_moving_cell(calc, numbers, pos, cell, True, n, 300.0, 1.0, 20.0, vel=vel, **baro):
                    out.append((st, E, bool(calc.updated)))
                    if st % 4 == 0:
                        sync[st] = (p.copy(), h.copy())
                    last = (p.copy(), v.copy(), h.copy())
            else:
                at = Atoms(numbers, pos, cell, True, velocities=vel)
                assert calc.md_on_device_ok() or calc._needs_seed()
                for st, E, Tk, u, w in calc.run_md(at, n, 300.0, dt_fs=1.0, tdamp_fs=20.0, chunk=16, sync_every=4, **baro):
                    out.append((st, E, bool(u)))
                    if st % 4 == 0:
                        sync[st] = (at.positions.copy(), np.array(at.cell, float))
                last = (at.positions.copy(), at.get_velocities(), np.array(at.cell, float))
            assert len(out) == n + 1
            legs.append((out, sync, last, calc.size))
            # the second leg goes on from where the first ended (shifted as a whole: a calculator that is asked for the very
            # configuration it has just evaluated answers from its cache and writes no line)
            pos, vel, cell = last[0] + 0.01, last[1], last[2]
        txt = open(d / "active.log").read().splitlines()
        res[mode] = (legs, [re.sub(r"^\S+ \S+ ", "", ln) for ln in txt])
        calc.engine.close()
    (hl, hlog), (dl, dlog) = res["host"], res["device"]
    num = re.compile(r"^(\d+) (\S+) (\S+) (\S+) $")
    assert len(hlog) == len(dlog), next(((i, a, b) for i, (a, b) in enumerate(zip(hlog, dlog)) if a.split(" ")[:2] != b.split(" ")[:2]), None)
    for a, b in zip(hlog, dlog):
        ma, mb = num.match(a), num.match(b)
        if ma and mb:   # a step's line: energy and covloss bit for bit, the temperature to the order of its sum
            assert ma.group(1) == mb.group(1) and ma.group(2) == mb.group(2) and ma.group(4) == mb.group(4), (a, b)
            assert abs(float(ma.group(3)) - float(mb.group(3))) <= 1e-12 * float(ma.group(3)), (a, b)
        else:
            assert a == b
    for leg, ((ho, hs, hlast, hsize), (do, ds, dlast, dsize)) in enumerate(zip(hl, dl)):
        assert ho == do                                       # steps, energies, updates: the same
        assert hsize == dsize
        assert sorted(hs) == sorted(ds) and len(hs) == steps[leg] // 4 + 1
        for st in hs:
            assert np.array_equal(hs[st][0], ds[st][0]) and np.array_equal(hs[st][1], ds[st][1]), st
        for a, b in zip(hlast, dlast):
            assert np.array_equal(a, b)
    upd = [o[0] for o in dl[0][0] if o[2]]
    assert len(upd) >= 1 and dl[0][3][1] > 2, upd             # the gate fired and the model grew
    assert not any(o[2] for o in dl[1][0][1:])
    assert np.abs(dl[1][2][2] - ac.start(0)[3]).max() > 1e-6   # the cell has moved


def _two_rank_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.watchdog import Watchdog
    from autoforce_amd.workloads import FS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"barostat on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=0.0, kT=kB * T, ttime=TDAMP * FS)
        ext = np.array([-baro["externalstress"]] * 3 + [0.0] * 3)
        code = _lib.load().sgpr_md_barostat(mdl.handle, float(baro["pfactor"]), _lib.ptr(ext), None, 1.0)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_barostat_and_goes_on_working():
    """The sharded last kernel integrates at constant cell: sgpr_md_barostat says SGPR_E_UNSUPPORTED on every rank and the
    handles go on predicting."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29400 + (os.getpid() % 250)
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
