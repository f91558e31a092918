"""GPU tests of the pair-distance accumulator of the device MD loop (sgpr_md_rdf / sgpr_md_rdf_read; md_rdf_pair_kernel and
md_rdf_done_kernel behind a sampled evaluation) against its host twin and definition workloads.RdfCounts: the twin is fed the
positions of the SAME run's frame record at every = 1, and every integer must be equal.  One call and a cut run, other settings,
held components, Nose-Hoover, the single-image form and the image block (rmax beyond half the cell; a cell thinner than rmax, so
self-images), frames whose species segments end off a tile and span several tiles, a covloss halt in the middle (the next_due
guard and the speculative evaluation), a run that is not disturbed, the displacement accumulator beside it, what a later run and
the handle's memory owe to it, every refusal in both directions, and ActiveCalculator.run_md(rdf=) on the device against the host
loop.  Frame and model are those of test_hip_npt_device.py (LiPS, side 8: 192 / 64 / 256 atoms, cubic 21.76 A, m = 48)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from test_hip_msd_device import EVALS, T, _begin, _noise, _shared
from test_hip_msd_device import _frame as _msd_frame
from test_hip_npt_device import _model

pytestmark = pytest.mark.gpu

RDF = (1, 6.0, 60, 0.0)      # every, rmax, bins, rmin: the single-image form on the module's frame
RDF12 = (1, 12.0, 48, 0.5)   # rmax beyond half the cell: the image block with R = 1
INTS = ("hist", "species", "n")


def _frame(kind=None):
    """test_hip_msd_device's frames (None, "sub200", "chunks"), and "thin": the 256 atoms of lips((8, 8, 4)), L_z = 10.88."""
    if kind != "thin":
        return _msd_frame(kind)
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS, lips
    numbers, pos, cell, pbc = lips((8, 8, 4), seed=0)
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return numbers, pos, cell, pbc, mass, vel


def _run(fr, rdf, cuts=(EVALS,), nh=False, record=True, seed=None, msd=None, **kw):
    """A run of sum(cuts) evaluations on the module's model with the accumulator `rdf` = (every, rmax, bins, rmin) or None (and
    the displacements `msd` beside it).  Returns (table or None, recorded positions or None, scalar rows, final state, msd table)."""
    mdl = _shared()[0]
    _begin(mdl, fr, nh=nh, **({} if seed is None else dict(seed=seed)), **kw)
    if record:
        mdl.md_record(1, velocities=False, results=False)
    if msd is not None:
        mdl.md_msd(*msd)
    if rdf is not None:
        mdl.md_rdf(*rdf)
    noise = None if (nh or seed is not None) else _noise(fr, sum(cuts))
    rows, xs, t = [], [], 0
    for n in cuts:
        t_call = time.perf_counter()
        sc, code = mdl.md_run(n, None if noise is None else noise[t:t + n])
        print(f"md_run({n}) on {len(fr[0])} atoms, accumulator {rdf}: {1e6 * (time.perf_counter() - t_call) / n:.1f} us per evaluation")
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
        if record:
            f = mdl.md_frames()
            assert list(f["index"]) == list(range(t, t + n))
            xs.append(f["positions"].copy())
        t += n
    tab = None if rdf is None else mdl.md_rdf_table()
    return tab, (np.concatenate(xs) if record else None), np.array(rows), mdl.md_state(), (None if msd is None else mdl.md_msd_table())


def _twin(fr, rdf, xs):
    from autoforce_amd.workloads import RdfCounts
    tw = RdfCounts(rdf[0], rdf[1], rdf[2], rdf[3], fr[0], _shared()[0].species, fr[2], fr[3])
    for x in xs:
        tw.add(x)
    return tw


def _same(tab, want, what=""):
    S = len(want["species"])
    print(f"{what}: samples {tab['samples']} next_due {tab['next_due']} counts per pair device "
          f"{[int(tab['hist'][a, b].sum()) for a in range(S) for b in range(a, S)]} twin {[int(want['hist'][a, b].sum()) for a in range(S) for b in range(a, S)]}")
    assert tab["hist"].dtype == np.uint64 and tab["hist"].shape == want["hist"].shape
    for k in INTS:
        assert np.array_equal(tab[k], want[k]), (what, k, int((np.asarray(tab[k]) != np.asarray(want[k])).sum()))
    for k in ("samples", "next_due", "every", "bins", "rmin", "rmax", "volume"):
        assert tab[k] == want[k], (what, k, tab[k], want[k])


def test_one_call_and_a_cut_run_equal_the_twin():
    fr = _frame()
    tab, xs, rows, _, _ = _run(fr, RDF)
    tw = _twin(fr, RDF, xs)
    want = tw.table()
    assert not tw.R.any() and want["samples"] == EVALS and np.all(want["hist"].sum(axis=2) > 0)
    _same(tab, want, "one call")
    assert np.array_equal(tab["hist"], tab["hist"].transpose(1, 0, 2))
    tab2, xs2, rows2, _, _ = _run(fr, RDF, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "held", "nose-hoover"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    rdf = (3, 6.0, 60, 0.0) if variant == "every3" else RDF
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _, _ = _run(fr, rdf, cuts=(20,), nh=(variant == "nose-hoover"), **kw)
    want = _twin(fr, rdf, xs).table()
    if variant == "every3":
        assert want["samples"] == 7 and want["next_due"] == 21
    if variant == "held":
        assert np.array_equal(xs[-1][kw["fixed"]], fr[1][kw["fixed"]])
    _same(tab, want, variant)


@pytest.mark.parametrize("kind", [None, "thin"])
def test_the_image_block_beyond_half_the_cell_and_self_images(kind):
    """rmax = 12 on the cubic 21.76 A frame: R = 1 in every direction; on the 256 atoms of lips((8, 8, 4)) L_z = 10.88 < rmax:
    an atom counts its own images."""
    fr = _frame(kind)
    tab, xs, _, _, _ = _run(fr, RDF12, cuts=(2, 4))
    tw = _twin(fr, RDF12, xs)
    assert list(tw.R) == [1, 1, 1]
    if kind == "thin":
        assert tw.heights[2] < RDF12[1] and len(fr[0]) == 256
        from autoforce_amd.workloads import RdfCounts
        lone = RdfCounts(1, RDF12[1], RDF12[2], RDF12[3], fr[0][:1], _shared()[0].species, fr[2], fr[3])
        lone.add(fr[1][:1])
        assert lone.table()["hist"].sum() == 2                                           # (the images at +- L_z)
    _same(tab, tw.table(), f"rmax 12, frame {kind}")


@pytest.mark.parametrize("kind,rdf", [("sub200", RDF), ("sub200", RDF12), ("chunks", RDF), ("chunks", (2, 14.0, 100, 0.0))])
def test_segments_off_a_tile_and_over_several_tiles(kind, rdf):
    from autoforce_amd.workloads import MSD_CHUNK
    fr = _frame(kind)
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":   # (no segment ends on a tile or a wave: every diagonal tile is ragged)
        assert n.min() < 64 and np.all(n % 64 != 0) and np.all(np.cumsum(n) % 64 != 0) and n.max() < 128
    else:                  # (a species over three tiles of 128, the last ragged: off-diagonal tile pairs of one species)
        assert MSD_CHUNK < n.max() < 3 * 128 and n.max() % 128 != 0 and n.min() < 128
    tab, xs, _, _, _ = _run(fr, rdf, cuts=(2, 3))
    tw = _twin(fr, rdf, xs)
    assert bool(tw.R.any()) == (rdf[1] > 10.0)
    want = tw.table()
    assert np.array_equal(want["n"], n) and np.all(want["hist"].sum(axis=2) > 0)
    _same(tab, want, f"{kind} {rdf}")


def test_a_covloss_halt_counts_every_configuration_once():
    """The gate fires at evaluation k inside a call: k has been sampled (its halt is known one evaluation late), the speculative
    evaluation k + 1 behind it must stay out, and the repeat of k — the model unchanged, resumed as device_loop.batches resumes:
    one ungated evaluation, then on — must not count again."""
    fr, evals = _frame(), 24
    want, xs, rows, state, _ = _run(fr, RDF, cuts=(evals,), seed=77)
    b = rows[:, 11]
    ks = [k for k in range(2, evals - 2) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    ediff = 0.5 * (b[:k].max() + b[k])
    print(f"halt at evaluation {k} of {evals}: covloss {b[k]:.6e} over {b[:k].max():.6e}")
    mdl = _shared()[0]
    _begin(mdl, fr, seed=77)
    mdl.md_rdf(*RDF)
    sc, code = mdl.md_run(evals, None, ediff=ediff)
    assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
    mid = mdl.md_rdf_table()
    assert mid["next_due"] == k + 1 and mid["samples"] == k + 1
    _same(mid, _twin(fr, RDF, xs[:k + 1]).table(), f"behind the halt at {k}")
    sc1, code = mdl.md_run(1, None, ediff=0.0)
    assert code == 0 and len(sc1) == 1 and mdl.md_rdf_table()["next_due"] == k + 1
    sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
    assert code == 0 and np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows)
    _same(mdl.md_rdf_table(), want, f"halt at {k}")
    _same(want, _twin(fr, RDF, xs).table(), "the run that never halted")


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    fr = _frame()
    _, xs0, rows0, st0, _ = _run(fr, None, cuts=(9, 11), nh=nh)
    tab, xs1, rows1, st1, _ = _run(fr, (2, 6.0, 60, 0.0), cuts=(9, 11), nh=nh)
    print(f"nh {nh}: samples {tab['samples']}, E of the last row without / with {rows0[-1, 0]!r} / {rows1[-1, 0]!r}")
    assert tab["samples"] == 10 and np.array_equal(rows0, rows1) and np.array_equal(xs0, xs1)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st0[key], st1[key]), key


def test_displacements_and_pair_distances_together_equal_each_alone():
    from test_hip_msd_device import KEYS
    fr, msd, rdf = _frame(), (2, 3, True), (3, 6.0, 60, 0.0)
    both, _, rows, _, mboth = _run(fr, rdf, cuts=(9, 11), msd=msd, record=False, seed=5)
    alone, _, rows_r, _, _ = _run(fr, rdf, cuts=(9, 11), record=False, seed=5)
    _, _, rows_m, _, malone = _run(fr, None, cuts=(9, 11), msd=msd, record=False, seed=5)
    assert np.array_equal(rows, rows_r) and np.array_equal(rows, rows_m)
    assert both["samples"] == 7 and both["next_due"] == 21 and mboth["samples"] == 10 and mboth["next_due"] == 20
    _same(both, alone, "beside md_msd")
    for k in KEYS:
        assert np.array_equal(mboth[k], malone[k]), k


def test_a_later_run_starts_from_zeros_and_the_memory_owes_it_nothing():
    """A second attach on the same handle zeroes the table; a run begun behind an accumulator run is the run on a fresh handle;
    md_rdf_table refuses the plain run; a detach gives the table back at once, md_end and close() every byte."""
    from autoforce_amd import _lib
    from test_hip_teardown import _live
    fr = _frame()                     # (the module's own model is alive before the first reading)
    before = _live()
    mdl, _ = _model()

    def R():
        _begin(mdl, fr, seed=7)
        out = [mdl.md_run(n, None, final=f) for n, f in ((2, False), (4, True))]
        assert all(code == 0 for _, code in out)
        return np.concatenate([sc for sc, _ in out]), mdl.md_state(results=True)

    def A():
        _begin(mdl, fr, seed=7)
        mdl.md_rdf(*RDF)
        assert not mdl.md_rdf_table()["hist"].any() and mdl.md_rdf_table()["samples"] == 0
        sc, code = mdl.md_run(6, None)
        assert code == 0
        return mdl.md_rdf_table()
    first = R()
    t1 = A()
    t2 = A()
    assert t1["samples"] == 6 and t1["hist"].sum() > 0
    _same(t2, t1, "the second attach")
    again = R()
    assert np.array_equal(first[0], again[0])
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(first[1][key]), np.asarray(again[1][key])), key
    assert _lib.load().sgpr_md_rdf_read(mdl.handle, None, None, None) == _lib.E_INVALID
    assert b"call sgpr_md_begin and sgpr_md_rdf first" in _lib.load().sgpr_last_error()
    mdl.md_end()                      # (the table goes with the run)
    _begin(mdl, fr, seed=7)
    held = _live()
    mdl.md_rdf(*RDF)                  # 192 / 64 / 256 atoms: 2 + 1 + 2 tiles of 128, 15 tile pairs I <= J
    assert np.array_equal(_live() - held, [8 * 9 * 60 + 8 * 2 + 4 * (15 * 6 + 3), 3])     # the table, the control words, the tile pairs
    mdl.md_rdf(0, 1.0)                # (a detach frees them)
    assert np.array_equal(_live() - held, [0, 0])
    with pytest.raises(RuntimeError, match="no accumulator"):
        mdl.md_rdf_table()
    mdl.md_rdf(*RDF)
    mdl.md_end()                      # (and so does the end of the run)
    mdl.close()
    assert np.array_equal(_live() - before, [0, 0])


def test_refusals_in_both_directions_leave_the_handle_working():
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    from test_hip_neb_device import _band
    from test_hip_pimd_device import _begin as _begin_pimd, _polymer
    mdl, lib = _shared()[0], _lib.load()
    fr = _frame()
    numbers, pos, cell, pbc, mass, vel = fr
    h, N = mdl.handle, len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    _, _, rows, _, _ = _run(fr, None, cuts=(4,), record=False, seed=77)
    UNS, INV = _lib.E_UNSUPPORTED, _lib.E_INVALID

    def rdf(every=1, rmin=0.0, rmax=6.0, bins=60):
        return lib.sgpr_md_rdf(h, every, rmin, rmax, bins)

    def words(w):
        assert w in lib.sgpr_last_error(), lib.sgpr_last_error()
    mdl.md_end()
    assert rdf() == INV and lib.sgpr_md_rdf_read(h, None, None, None) == INV            # no run
    _begin(mdl, fr, seed=77)
    for args in (dict(every=-1), dict(bins=0), dict(bins=2049), dict(rmin=-0.5), dict(rmin=6.0), dict(rmin=7.0), dict(rmax=float("nan"))):
        assert rdf(**args) == INV, args
    assert lib.sgpr_md_rdf_read(h, None, None, None) == INV                             # a run without the accumulator
    assert rdf(rmax=54.0) == 0 and rdf(rmax=55.0) == UNS                                # 2.5 heights of 21.76 = 54.4
    words(b"against the cell height 21.76 along direction 0")
    with pytest.raises(NotImplementedError, match="cell height"):
        mdl.md_rdf(1, 55.0)
    # a barostat
    ext = np.array([-GPA] * 3 + [0.0] * 3)
    baro = lambda: lib.sgpr_md_barostat(h, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0)
    _begin(mdl, fr, nh=True)
    assert rdf() == 0 and baro() == UNS
    words(b"sgpr_md_barostat: the run accumulates pair distances")
    _begin(mdl, fr, nh=True)
    assert baro() == 0 and rdf() == UNS
    words(b"sgpr_md_rdf: the run has a barostat")
    # a relaxation
    _begin(mdl, fr)
    assert rdf() == 0 and lib.sgpr_md_relax(h, 0.05, None, 0, None) == UNS
    words(b"sgpr_md_relax: the run accumulates pair distances")
    _begin(mdl, fr)
    assert lib.sgpr_md_relax(h, 0.05, None, 0, None) == 0 and rdf() == UNS
    words(b"sgpr_md_rdf: the run is a relaxation")
    # a band
    band = np.ascontiguousarray(_band(pos, 1))
    _begin(mdl, fr)
    assert rdf() == 0 and lib.sgpr_md_neb(h, 1, _lib.ptr(band[1:2]), 0.05, 0.1, 0, None) == UNS
    words(b"sgpr_md_neb: the run accumulates pair distances")
    mdl.neb_begin(numbers, band, cell, pbc, 0.05)
    assert rdf() == UNS
    words(b"sgpr_md_rdf: the run is a nudged elastic band")
    # a polymer
    _, beads, bvel, _ = _polymer(numbers, pos, 2)
    _begin(mdl, fr)
    assert rdf() == 0 and lib.sgpr_md_pimd(h, 2, _lib.ptr(np.ascontiguousarray(beads)), _lib.ptr(np.ascontiguousarray(bvel)), kB * T, 0.001, 1.0) == UNS
    words(b"sgpr_md_pimd: the run accumulates pair distances")
    _begin_pimd(mdl, numbers, beads, bvel, mass, cell, pbc, seed=7)
    assert rdf() == UNS
    words(b"sgpr_md_rdf: the run is a ring polymer")
    # a committee
    member, _ = _model(seed=2)
    arr = (C.c_void_p * 1)(member.handle.value)
    _begin(mdl, fr)
    assert rdf() == 0 and lib.sgpr_md_committee(h, 1, arr) == UNS
    words(b"sgpr_md_committee: the run accumulates pair distances")
    _begin(mdl, fr)
    assert lib.sgpr_md_committee(h, 1, arr) == 0 and rdf() == UNS
    words(b"sgpr_md_rdf: the run has a committee")
    with pytest.raises(NotImplementedError, match="committee"):
        mdl.md_rdf(1, 6.0)
    mdl.md_end()
    member.close()
    # a run that has started; a detach is always taken
    _begin(mdl, fr, seed=77)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and rdf() == INV
    words(b"sgpr_md_rdf: the run has started")
    assert rdf(every=0) == 0
    # the handle works: the energy it predicted, the plain run it ran
    assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0
    _, _, again, _, _ = _run(fr, None, cuts=(4,), record=False, seed=77)
    assert np.array_equal(again, rows)


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
    with Watchdog(f"pair distances on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_rdf(mdl.handle, 1, 0.0, 6.0, 60)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    """Pair distances are accumulated on one rank (test_hip_msd_device.py's two-rank refusal, for sgpr_md_rdf)."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29920 + (os.getpid() % 40)
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


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """ActiveCalculator.run_md(rdf=holder) with a teacher — the gate fires, calculate() updates the model, the run goes on — on
    the device (the accumulator inside the loop) and through the host loop (RdfCounts fed every step's positions): the same
    trajectory (rng= given), so the same integers."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.transport import Rdf, radial_distribution
    from helpers import PairTeacher
    steps, tabs, upd = 40, [], []
    for mode in ("host", "device"):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        d = tmp_path / mode
        d.mkdir()
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                                logfile=str(d / "active.log"), pckl=None, tape=None, **ac.KW)
        if mode == "host":
            calc.md_on_device_ok = lambda: False
        at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
        rmax = 0.9 * float(np.linalg.norm(np.asarray(cell).reshape(3, 3), axis=1).min())   # (beyond half the cell and the model's rc)
        holder = Rdf(2, rmax, 50)
        out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, rng=np.random.default_rng(9), chunk=16, rdf=holder))
        assert len(out) == steps + 1
        upd.append([o[0] for o in out if o[3]])
        tabs.append(holder.table())
        calc.engine.close()
    print(f"updates at steps {upd}, samples {tabs[0]['samples']}, counts host {int(tabs[0]['hist'].sum())} device {int(tabs[1]['hist'].sum())}")
    assert upd[0] == upd[1] and len(upd[0]) >= 1, upd        # (the device loop halted and went on)
    assert tabs[0]["samples"] == 21 and tabs[0]["hist"].sum() > 0
    _same(tabs[1], tabs[0], "run_md")
    r, g = radial_distribution(holder)
    assert set(a for p in g for a in p) == set(int(z) for z in np.unique(numbers)) and all(np.all(np.isfinite(v)) for v in g.values())
