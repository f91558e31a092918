"""GPU tests of the displacement accumulator of the device MD loop (sgpr_md_msd / sgpr_md_msd_read; md_msd_part_kernel and
md_msd_fold_kernel behind a sampled evaluation) against its host twin and definition workloads.MsdBlocks, bit for bit: the twin
is fed the positions of the SAME run's frame record at every = 1, so the accumulator is exercised beside the record.  One call
and a cut run, other settings, held components, Nose-Hoover, frames whose species segments end off a wave and span several
chunks, a covloss halt in the middle (the next_due guard and the speculative evaluation), a run that is not disturbed, what a
later run and the handle's memory owe to it, every refusal in both directions, and ActiveCalculator.run_md(msd=) on the device
against the host loop.  Frame and model are those of test_hip_npt_device.py (LiPS, side 8: 192 / 64 / 256 atoms, m = 48)."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

from test_hip_npt_device import _model

pytestmark = pytest.mark.gpu

T = 600.0
EVALS = 40
KEYS = ("count", "msd", "msd_sq", "smd", "smd_sq")


@functools.lru_cache(maxsize=None)
def _shared():
    mdl, frame = _model()
    return mdl, frame


def _frame(kind=None):
    """The module's frame; "sub200": 200 of its atoms (the smallest species has fewer than 64, no segment ends on a wave);
    "chunks": 540 atoms of lips(10) — the largest species spans two chunks of 256, the second ragged."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS, lips
    numbers, pos, cell, pbc = _shared()[1]
    if kind is not None:
        if kind == "chunks":
            numbers, pos, cell, pbc = lips(10, seed=0)
        keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=200 if kind == "sub200" else 540, replace=False))
        numbers, pos = numbers[keep], pos[keep]
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return numbers, pos, cell, pbc, mass, vel


def _begin(mdl, fr, nh=False, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    numbers, pos, cell, pbc, mass, vel = fr
    par = dict(dt=1.0 * FS, kT=kB * T, friction=0.0, ttime=25.0 * FS) if nh else dict(dt=1.0 * FS, kT=kB * T, friction=0.05)
    par.update(kw)
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **par)


def _noise(fr, evals=EVALS):
    return np.random.default_rng(9).normal(size=(evals, len(fr[0]), 3))


def _run(fr, msd, cuts=(EVALS,), nh=False, record=True, seed=None, **kw):
    """A run of sum(cuts) evaluations on the module's model with the accumulator `msd` = (every, levels, com) or None.
    Returns (table or None, recorded positions [evals, N, 3] or None, scalar rows, final state)."""
    mdl = _shared()[0]
    _begin(mdl, fr, nh=nh, **({} if seed is None else dict(seed=seed)), **kw)
    if record:
        mdl.md_record(1, velocities=False, results=False)
    if msd is not None:
        mdl.md_msd(*msd)
    noise = None if (nh or seed is not None) else _noise(fr, sum(cuts))
    rows, xs, t = [], [], 0
    for n in cuts:
        t_call = time.perf_counter()
        sc, code = mdl.md_run(n, None if noise is None else noise[t:t + n])
        print(f"md_run({n}) on {len(fr[0])} atoms, accumulator {msd}: {1e6 * (time.perf_counter() - t_call) / n:.1f} us per evaluation")
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
        if record:
            f = mdl.md_frames()
            assert list(f["index"]) == list(range(t, t + n))
            xs.append(f["positions"].copy())
        t += n
    tab = None if msd is None else mdl.md_msd_table()
    return tab, (np.concatenate(xs) if record else None), np.array(rows), mdl.md_state()


def _twin(fr, msd, xs):
    from autoforce_amd.workloads import MsdBlocks
    tw = MsdBlocks(msd[0], msd[1], msd[2], fr[4], fr[0], _shared()[0].species)
    for x in xs:
        tw.add(x)
    return tw.table()


def _same(tab, want, what=""):
    print(f"{what}: count {list(tab['count'])} samples {tab['samples']} next_due {tab['next_due']} msd[0] device {list(tab['msd'][0])} "
          f"twin {list(want['msd'][0])} smd[-1] device {list(tab['smd'][-1])} twin {list(want['smd'][-1])}")
    for k in KEYS + ("lags", "species", "n"):
        assert np.array_equal(tab[k], want[k]), (what, k, np.abs(np.asarray(tab[k], float) - want[k]).max())
    assert tab["samples"] == want["samples"] and tab["next_due"] == want["next_due"], (what, tab["samples"], tab["next_due"])


def test_one_call_and_a_cut_run_equal_the_twin():
    fr, msd = _frame(), (1, 5, False)
    tab, xs, rows, _ = _run(fr, msd)
    want = _twin(fr, msd, xs)
    assert list(want["count"]) == [39, 19, 9, 4, 2] and np.all(want["msd"] > 0.0) and np.all(want["smd"] > 0.0)
    _same(tab, want, "one call")
    tab2, xs2, rows2, _ = _run(fr, msd, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "com", "held", "nose-hoover"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    msd = (3, 3, False) if variant == "every3" else (1, 5, variant == "com")
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _ = _run(fr, msd, nh=(variant == "nose-hoover"), **kw)
    want = _twin(fr, msd, xs)
    if variant == "every3":
        assert list(want["count"]) == [13, 6, 3] and list(want["lags"]) == [3, 6, 12]
    if variant == "held":   # (a held component does not move: the twin sees d = 0 there, bit for bit)
        assert np.array_equal(xs[-1][kw["fixed"]], fr[1][kw["fixed"]])
    assert np.all(want["msd"] > 0.0)
    _same(tab, want, variant)


@pytest.mark.parametrize("kind", ["sub200", "chunks"])
def test_segments_off_a_wave_and_over_several_chunks(kind):
    from autoforce_amd.workloads import MSD_CHUNK
    fr, msd = _frame(kind), (1, 4, True)
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert n.min() < 64 and np.all(n % 64 != 0) and np.all(np.cumsum(n) % 64 != 0)
    else:
        assert MSD_CHUNK < n.max() < 2 * MSD_CHUNK and n.min() < 128
    tab, xs, _, _ = _run(fr, msd, cuts=(5, 11))
    want = _twin(fr, msd, xs)
    assert np.array_equal(want["n"], n) and np.all(want["msd"] > 0.0)
    _same(tab, want, kind)


def test_a_covloss_halt_counts_every_configuration_once():
    """The gate fires at evaluation k inside a call: k has been sampled (its halt is known one evaluation late), the
    speculative evaluation k + 1 behind it must stay out, and the repeat of k — the model unchanged, resumed as
    device_loop.batches resumes: one ungated evaluation, then on — must not count again."""
    fr, msd, evals = _frame(), (1, 4, False), 24
    want, xs, rows, state = _run(fr, msd, cuts=(evals,), seed=77)
    b = rows[:, 11]
    ks = [k for k in range(2, evals - 2) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    ediff = 0.5 * (b[:k].max() + b[k])
    print(f"halt at evaluation {k} of {evals}: covloss {b[k]:.6e} over {b[:k].max():.6e}")
    mdl = _shared()[0]
    _begin(mdl, fr, seed=77)
    mdl.md_msd(*msd)
    sc, code = mdl.md_run(evals, None, ediff=ediff)
    assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
    mid = mdl.md_msd_table()
    assert mid["next_due"] == k + 1 and mid["count"][0] == k
    sc1, code = mdl.md_run(1, None, ediff=0.0)
    assert code == 0 and len(sc1) == 1 and mdl.md_msd_table()["next_due"] == k + 1
    sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
    assert code == 0 and np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows)
    _same(mdl.md_msd_table(), want, f"halt at {k}")
    _same(want, _twin(fr, msd, xs), "the run that never halted")


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    fr = _frame()
    _, _, rows0, st0 = _run(fr, None, cuts=(9, 11), nh=nh, record=False)
    tab, _, rows1, st1 = _run(fr, (2, 3, True), cuts=(9, 11), nh=nh, record=False)
    print(f"nh {nh}: count {list(tab['count'])}, E of the last row without / with {rows0[-1, 0]!r} / {rows1[-1, 0]!r}")
    assert tab["count"][0] == 9 and np.array_equal(rows0, rows1)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st0[key], st1[key]), key


def test_a_later_run_and_the_memory_owe_it_nothing():
    """The test_hip_md_restart.py rule: a run begun behind an accumulator run is the run on a fresh handle, the table is the
    run's (md_msd_table refuses the plain run), and close() gives every byte back."""
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
    first = R()
    _begin(mdl, fr, seed=7)
    mdl.md_msd(1, 6, True)
    sc, code = mdl.md_run(10, None)
    assert code == 0 and mdl.md_msd_table()["count"][0] == 9
    again = R()
    assert np.array_equal(first[0], again[0])
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(first[1][key]), np.asarray(again[1][key])), key
    tab = np.zeros((6, 3, 4))
    assert _lib.load().sgpr_md_msd_read(mdl.handle, _lib.ptr(tab), None, None) == _lib.E_INVALID
    assert b"call sgpr_md_begin and sgpr_md_msd first" in _lib.load().sgpr_last_error()
    _begin(mdl, fr, seed=7)
    mdl.md_msd(1, 6, True)
    mdl.md_end()                      # (the origins and the table go with the run)
    mdl.close()
    assert np.array_equal(_live() - before, [0, 0])


def test_a_detach_gives_the_memory_back_and_a_fresh_attach_starts_from_zeros():
    """md_msd(0, ...) on a begun run — before its first call and behind one — gives back exactly what the attach took (the way
    test_hip_vanhove_device.py's detach is checked), md_msd_table then refuses, and the next attach owes the table that went
    nothing: zeros before the first call, the twin's table behind a run."""
    from test_hip_teardown import _live
    mdl, fr, msd = _shared()[0], _frame(), (1, 6, True)
    _begin(mdl, fr, seed=7)
    mdl.md_msd(0, 0)                  # (the buffers of the run before are the handle's until a detach or md_end)
    plain = _live()
    mdl.md_msd(*msd)
    held = _live()
    assert held[0] > plain[0] and held[1] > plain[1]
    mdl.md_msd(0, 0)
    assert np.array_equal(_live(), plain)
    mdl.md_msd(*msd)
    assert np.array_equal(_live(), held)
    sc, code = mdl.md_run(6, None)
    assert code == 0 and mdl.md_msd_table()["count"][0] == 5
    running = _live()                 # (the call has sized the run's own buffers)
    mdl.md_msd(0, 0)
    print(f"live memory plain {list(plain)}, attached {list(held)}, behind a call {list(running)}, detached {list(_live())}")
    assert np.array_equal(running - _live(), held - plain)
    with pytest.raises(RuntimeError, match="no accumulator"):
        mdl.md_msd_table()
    _begin(mdl, fr, seed=7)
    mdl.md_record(1, velocities=False, results=False)
    mdl.md_msd(*msd)
    zero = mdl.md_msd_table()
    assert zero["samples"] == 0 and zero["next_due"] == 0 and not np.any(zero["count"])
    assert not any(np.any(zero[k]) for k in KEYS)
    sc, code = mdl.md_run(10, None)
    assert code == 0
    _same(mdl.md_msd_table(), _twin(fr, msd, mdl.md_frames()["positions"]), "a fresh attach behind a detach")


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
    _, _, rows, _ = _run(fr, None, cuts=(4,), record=False, seed=77)
    UNS, INV = _lib.E_UNSUPPORTED, _lib.E_INVALID

    def msd():
        return lib.sgpr_md_msd(h, 1, 4, 0)

    def words(w):
        assert w in lib.sgpr_last_error(), lib.sgpr_last_error()
    mdl.md_end()
    assert msd() == INV and lib.sgpr_md_msd_read(h, None, None, None) == INV          # no run
    _begin(mdl, fr, seed=77)
    for every, levels, com in ((-1, 4, 0), (1, 0, 0), (1, 33, 0), (1, 4, 2)):
        assert lib.sgpr_md_msd(h, every, levels, com) == INV
    assert lib.sgpr_md_msd_read(h, None, None, None) == INV                            # a run without the accumulator
    # a barostat
    ext = np.array([-GPA] * 3 + [0.0] * 3)
    baro = lambda: lib.sgpr_md_barostat(h, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0)
    _begin(mdl, fr, nh=True)
    assert msd() == 0 and baro() == UNS
    words(b"sgpr_md_barostat: the run accumulates displacements")
    _begin(mdl, fr, nh=True)
    assert baro() == 0 and msd() == UNS
    words(b"sgpr_md_msd: the run has a barostat")
    # a relaxation
    _begin(mdl, fr)
    assert msd() == 0 and lib.sgpr_md_relax(h, 0.05, None, 0, None) == UNS
    words(b"sgpr_md_relax: the run accumulates displacements")
    _begin(mdl, fr)
    assert lib.sgpr_md_relax(h, 0.05, None, 0, None) == 0 and msd() == UNS
    words(b"sgpr_md_msd: the run is a relaxation")
    # a band
    band = np.ascontiguousarray(_band(pos, 1))
    _begin(mdl, fr)
    assert msd() == 0 and lib.sgpr_md_neb(h, 1, _lib.ptr(band[1:2]), 0.05, 0.1, 0, None) == UNS
    words(b"sgpr_md_neb: the run accumulates displacements")
    mdl.neb_begin(numbers, band, cell, pbc, 0.05)
    assert msd() == UNS
    words(b"sgpr_md_msd: the run is a nudged elastic band")
    # a polymer
    _, beads, bvel, _ = _polymer(numbers, pos, 2)
    _begin(mdl, fr)
    assert msd() == 0 and lib.sgpr_md_pimd(h, 2, _lib.ptr(np.ascontiguousarray(beads)), _lib.ptr(np.ascontiguousarray(bvel)), kB * T, 0.001, 1.0) == UNS
    words(b"sgpr_md_pimd: the run accumulates displacements")
    _begin_pimd(mdl, numbers, beads, bvel, mass, cell, pbc, seed=7)
    assert msd() == UNS
    words(b"sgpr_md_msd: the run is a ring polymer")
    # a committee
    member, _ = _model(seed=2)
    arr = (C.c_void_p * 1)(member.handle.value)
    _begin(mdl, fr)
    assert msd() == 0 and lib.sgpr_md_committee(h, 1, arr) == UNS
    words(b"sgpr_md_committee: the run accumulates displacements")
    _begin(mdl, fr)
    assert lib.sgpr_md_committee(h, 1, arr) == 0 and msd() == UNS
    words(b"sgpr_md_msd: the run has a committee")
    with pytest.raises(NotImplementedError, match="committee"):
        mdl.md_msd(1, 4)
    mdl.md_end()
    member.close()
    # a run that has started; a detach is always taken
    _begin(mdl, fr, seed=77)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and msd() == INV
    words(b"sgpr_md_msd: the run has started")
    assert lib.sgpr_md_msd(h, 0, 0, 0) == 0
    # the handle works: the energy it predicted, the plain run it ran
    assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0
    _, _, again, _ = _run(fr, None, cuts=(4,), record=False, seed=77)
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
    with Watchdog(f"displacements on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_msd(mdl.handle, 1, 4, 0)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    """Displacements are accumulated on one rank (test_hip_record_device.py's two-rank refusal, for sgpr_md_msd)."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29870 + (os.getpid() % 40)
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
    """ActiveCalculator.run_md(msd=holder) with a teacher — the gate fires, calculate() updates the model, the run goes on —
    on the device (the accumulator inside the loop) and through the host loop (MsdBlocks fed every step's positions): the
    same trajectory (rng= given), so the same tables, bit for bit."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.transport import Msd, diffusion_constants
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
        holder = Msd(2, 4, True)
        out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, rng=np.random.default_rng(9), chunk=16, msd=holder))
        assert len(out) == steps + 1
        upd.append([o[0] for o in out if o[3]])
        tabs.append(holder.table())
        calc.engine.close()
    print(f"updates at steps {upd}, counts {list(tabs[0]['count'])}, msd[0] host {list(tabs[0]['msd'][0])} device {list(tabs[1]['msd'][0])}")
    assert upd[0] == upd[1] and len(upd[0]) >= 1, upd        # (the device loop halted and went on)
    assert list(tabs[0]["count"]) == [20, 10, 5, 2]
    for k in KEYS + ("lags", "species", "n"):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    D = diffusion_constants(holder, 1.0)
    assert set(D) == set(int(z) for z in np.unique(numbers)) and all(np.isfinite(v["Dt"][0]) for v in D.values())
