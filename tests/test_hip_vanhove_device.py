"""GPU tests of the van Hove accumulator of the device MD loop (sgpr_md_vanhove / _edges / _read; md_vh_pair_kernel,
md_vh_self_kernel and md_vh_done_kernel behind a sampled evaluation) against its host twin and definition
workloads.VanHoveCounts: every entry is a count, every table is compared with np.array_equal.  The twin is fed the positions of
the SAME run's frame record at every = 1, so the accumulator is exercised beside the record.  One call and a cut run, other
settings, held components, Nose-Hoover, angular bins and radial only, the distinct part with one image and with the image block,
frames whose species segments end off a wave and span several chunks and tiles, a covloss halt in the middle (the next_due guard
and the speculative evaluation), a run that is not disturbed, what a later run, a detach and the handle's memory owe to it, every
refusal in both directions, and ActiveCalculator.run_md(vanhove=) on the device against the host loop.  Frame and model are those
of test_hip_msd_device.py (LiPS, side 8, m = 48)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from test_hip_msd_device import EVALS, T, _begin, _frame, _noise, _shared
from test_hip_npt_device import _model

pytestmark = pytest.mark.gpu

TABLES = ("self", "over", "distinct", "count", "lags", "species", "n")
SETTINGS = ("every", "levels", "rmax", "rbins", "tbins", "pbins", "dmax", "dbins", "volume")
RMAX = 0.12   # Angstrom: at 600 K an atom moves about 0.01 per fs — the short lags fall inside, the long ones partly beyond


def _hmin(fr):
    from autoforce_amd.workloads import rdf_geometry
    return float(rdf_geometry(fr[2], fr[3], 1.0)[2].min())


def _vh(fr, every=1, levels=5, rbins=16, tbins=6, pbins=8, heights=None, dbins=0):
    """(every, levels, rmax, rbins, tbins, pbins, dmax, dbins); heights: dmax in units of the cell's smallest height."""
    return (every, levels, RMAX, rbins, tbins, pbins, None if heights is None else heights * _hmin(fr), dbins if heights is not None else 0)


def _run(fr, vh, cuts=(EVALS,), nh=False, record=True, seed=None, **kw):
    """A run of sum(cuts) evaluations on the module's model with the accumulator `vh` (the arguments of md_vanhove) or None.
    Returns (tables or None, recorded positions [evals, N, 3] or None, scalar rows, final state)."""
    mdl = _shared()[0]
    _begin(mdl, fr, nh=nh, **({} if seed is None else dict(seed=seed)), **kw)
    if record:
        mdl.md_record(1, velocities=False, results=False)
    if vh is not None:
        mdl.md_vanhove(*vh)
    noise = None if (nh or seed is not None) else _noise(fr, sum(cuts))
    rows, xs, t = [], [], 0
    for n in cuts:
        t_call = time.perf_counter()
        sc, code = mdl.md_run(n, None if noise is None else noise[t:t + n])
        print(f"md_run({n}) on {len(fr[0])} atoms, accumulator {vh}: {1e6 * (time.perf_counter() - t_call) / n:.1f} us per evaluation")
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
        if record:
            f = mdl.md_frames()
            assert list(f["index"]) == list(range(t, t + n))
            xs.append(f["positions"].copy())
        t += n
    tab = None if vh is None else mdl.md_vanhove_table()
    return tab, (np.concatenate(xs) if record else None), np.array(rows), mdl.md_state()


def _twin(fr, vh, xs):
    from autoforce_amd.workloads import VanHoveCounts
    t0 = time.perf_counter()
    tw = VanHoveCounts(*vh, fr[0], _shared()[0].species, fr[2], fr[3])
    for x in xs:
        tw.add(x)
    print(f"twin over {len(xs)} configurations: {time.perf_counter() - t0:.2f} s")
    return tw.table()


def _same(tab, want, what=""):
    print(f"{what}: count {list(tab['count'])} samples {tab['samples']} next_due {tab['next_due']} self per level device "
          f"{tab['self'].sum(axis=(1, 2, 3, 4)).tolist()} twin {want['self'].sum(axis=(1, 2, 3, 4)).tolist()} over device {tab['over'].sum(axis=1).tolist()} "
          f"twin {want['over'].sum(axis=1).tolist()} distinct device {tab['distinct'].sum(axis=(1, 2, 3)).tolist()} twin {want['distinct'].sum(axis=(1, 2, 3)).tolist()}")
    for k in TABLES:
        assert tab[k].shape == want[k].shape and tab[k].dtype == want[k].dtype, (what, k, tab[k].shape, want[k].shape, tab[k].dtype, want[k].dtype)
        assert np.array_equal(tab[k], want[k]), (what, k, int((np.asarray(tab[k]) != np.asarray(want[k])).sum()))
    for k in SETTINGS + ("samples", "next_due"):
        assert tab[k] == want[k], (what, k, tab[k], want[k])
    # conservation: every atom of every window is in a bin or beyond rmax
    assert np.array_equal(tab["self"].sum(axis=(2, 3, 4)) + tab["over"], np.outer(tab["count"], tab["n"]).astype(np.uint64))


def test_one_call_and_a_cut_run_equal_the_twin():
    fr = _frame()
    vh = _vh(fr, heights=0.45, dbins=40)
    tab, xs, rows, _ = _run(fr, vh)
    want = _twin(fr, vh, xs)
    assert list(want["count"]) == [39, 19, 9, 4, 2] and want["over"].sum() > 0 and np.all(want["self"].sum(axis=(2, 3, 4)) > 0)
    assert np.all(want["distinct"].sum(axis=3) > 0) and (want["self"].sum(axis=(0, 1, 2)) > 0).all()   # (every angular bin is visited)
    _same(tab, want, "one call")
    tab2, xs2, rows2, _ = _run(fr, vh, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "held", "nose-hoover", "radial", "images"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    vh = {"every3": _vh(fr, every=3, levels=3, heights=0.45, dbins=24), "radial": _vh(fr, rbins=64, tbins=1, pbins=1),
          "images": _vh(fr, levels=3, rbins=8, tbins=3, pbins=5, heights=1.2, dbins=64)}.get(variant, _vh(fr))
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _ = _run(fr, vh, cuts=(16,) if variant == "images" else (EVALS,), nh=(variant == "nose-hoover"), **kw)
    want = _twin(fr, vh, xs)
    if variant == "every3":
        assert list(want["count"]) == [13, 6, 3] and list(want["lags"]) == [3, 6, 12]
    if variant == "held":   # (a held atom does not move: d = 0 exactly, the bin (0, 0, pbins / 2))
        still = kw["fixed"].all(axis=1)
        assert still.any() and np.array_equal(xs[-1][still], fr[1][still])
        assert np.all(want["self"][:, :, 0, 0, 4].sum(axis=1) >= int(still.sum()) * want["count"].astype(np.uint64))
    if variant == "images":
        from autoforce_amd.workloads import rdf_geometry
        assert rdf_geometry(fr[2], fr[3], vh[6])[3].max() == 1 and np.all(want["distinct"].sum(axis=3) > 0)
    assert want["self"].sum() > 0
    _same(tab, want, variant)


@pytest.mark.parametrize("kind", ["sub200", "chunks", "chunks-images"])
def test_segments_off_a_wave_and_over_several_chunks_and_tiles(kind):
    from autoforce_amd.workloads import MSD_CHUNK
    fr = _frame(kind.split("-")[0])
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert n.min() < 64 and np.all(n % 64 != 0) and np.all(np.cumsum(n) % 64 != 0)
        vh, cuts = _vh(fr, levels=4, heights=1.2, dbins=50), (5, 11)
    else:   # (the largest species: two chunks of the self part, the second ragged; three 128-tiles, so ordered tile pairs (I, J) and (J, I))
        assert MSD_CHUNK < n.max() < 2 * MSD_CHUNK and n.min() < 128 and n.max() > 256
        vh, cuts = (_vh(fr, levels=4, heights=0.45, dbins=50), (5, 11)) if kind == "chunks" else (_vh(fr, levels=2, rbins=8, tbins=2, pbins=3, heights=1.2, dbins=32), (8,))
    tab, xs, _, _ = _run(fr, vh, cuts=cuts)
    want = _twin(fr, vh, xs)
    assert np.array_equal(want["n"], n) and want["self"].sum() > 0 and np.all(want["distinct"].sum(axis=3) > 0)
    _same(tab, want, kind)


def test_a_covloss_halt_counts_every_configuration_once():
    """The gate fires at evaluation k inside a call: k has been sampled (its halt is known one evaluation late), the
    speculative evaluation k + 1 behind it must stay out, and the repeat of k — the model unchanged, resumed as
    device_loop.batches resumes: one ungated evaluation, then on — must not count again."""
    fr, evals = _frame(), 24
    vh = _vh(fr, levels=4, heights=0.45, dbins=40)
    want, xs, rows, state = _run(fr, vh, cuts=(evals,), seed=77)
    b = rows[:, 11]
    ks = [k for k in range(2, evals - 2) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    ediff = 0.5 * (b[:k].max() + b[k])
    print(f"halt at evaluation {k} of {evals}: covloss {b[k]:.6e} over {b[:k].max():.6e}")
    mdl = _shared()[0]
    _begin(mdl, fr, seed=77)
    mdl.md_vanhove(*vh)
    sc, code = mdl.md_run(evals, None, ediff=ediff)
    assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
    mid = mdl.md_vanhove_table()
    assert mid["next_due"] == k + 1 and mid["count"][0] == k and mid["samples"] == k + 1
    sc1, code = mdl.md_run(1, None, ediff=0.0)
    again = mdl.md_vanhove_table()
    assert code == 0 and len(sc1) == 1 and again["next_due"] == k + 1
    for key in TABLES:
        assert np.array_equal(again[key], mid[key]), key
    sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
    assert code == 0 and np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows)
    _same(mdl.md_vanhove_table(), want, f"halt at {k}")
    _same(want, _twin(fr, vh, xs), "the run that never halted")


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    fr = _frame()
    _, _, rows0, st0 = _run(fr, None, cuts=(9, 11), nh=nh, record=False)
    tab, _, rows1, st1 = _run(fr, _vh(fr, every=2, levels=3, heights=1.2, dbins=16), cuts=(9, 11), nh=nh, record=False)
    print(f"nh {nh}: count {list(tab['count'])}, E of the last row without / with {rows0[-1, 0]!r} / {rows1[-1, 0]!r}")
    assert tab["count"][0] == 9 and np.array_equal(rows0, rows1)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st0[key], st1[key]), key


def test_a_later_run_a_detach_and_the_memory_owe_it_nothing():
    """The test_hip_md_restart.py rule: a run begun behind an accumulator run is the run on a fresh handle, the tables are the
    run's (md_vanhove_table refuses the plain run), a detach frees, and close() gives every byte back."""
    from autoforce_amd import _lib
    from test_hip_teardown import _live
    fr = _frame()                     # (the module's own model is alive before the first reading)
    before = _live()
    mdl, _ = _model()
    vh = _vh(fr, levels=6, heights=1.2, dbins=32)

    def R():
        _begin(mdl, fr, seed=7)
        out = [mdl.md_run(n, None, final=f) for n, f in ((2, False), (4, True))]
        assert all(code == 0 for _, code in out)
        return np.concatenate([sc for sc, _ in out]), mdl.md_state(results=True)
    first = R()
    _begin(mdl, fr, seed=7)
    mdl.md_vanhove(*vh)
    sc, code = mdl.md_run(10, None)
    assert code == 0 and mdl.md_vanhove_table()["count"][0] == 9
    again = R()
    assert np.array_equal(first[0], again[0])
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(first[1][key]), np.asarray(again[1][key])), key
    assert _lib.load().sgpr_md_vanhove_read(mdl.handle, None, None, None, None, None, None) == _lib.E_INVALID
    assert b"call sgpr_md_begin and sgpr_md_vanhove first" in _lib.load().sgpr_last_error()
    with pytest.raises(RuntimeError):
        mdl.md_vanhove_table()
    # a detach frees the origins and the tables, and the run is the plain one
    _begin(mdl, fr, seed=7)
    mdl.md_vanhove(0, 0, 0.0, 0)      # (the buffers of the run before are the handle's until a detach or md_end)
    plain = _live()
    mdl.md_vanhove(*vh)
    assert _live()[0] > plain[0]
    mdl.md_vanhove(0, 0, 0.0, 0)
    assert np.array_equal(_live(), plain)
    out = [mdl.md_run(n, None, final=f) for n, f in ((2, False), (4, True))]
    assert np.array_equal(np.concatenate([sc for sc, _ in out]), first[0])
    _begin(mdl, fr, seed=7)
    mdl.md_vanhove(*vh)
    mdl.md_end()                      # (the origins and the tables go with the run)
    mdl.close()
    assert np.array_equal(_live() - before, [0, 0])


def test_beside_the_other_accumulators_every_table_is_the_one_of_a_run_alone():
    fr = _frame()
    vh = _vh(fr, every=2, levels=3, heights=0.45, dbins=24)
    alone, _, rows, _ = _run(fr, vh, cuts=(20,), record=False, seed=5)
    mdl = _shared()[0]
    _begin(mdl, fr, seed=5)
    mdl.md_msd(1, 4, True)
    mdl.md_rdf(3, 4.0, 32)
    mdl.md_vacf(1, 8)
    mdl.md_vanhove(*vh)
    sc, code = mdl.md_run(20, None)
    assert code == 0 and np.array_equal(np.array(sc), rows)
    beside = mdl.md_vanhove_table()
    for k in TABLES + ("samples", "next_due"):
        assert np.array_equal(beside[k], alone[k]), k
    assert mdl.md_msd_table()["next_due"] == 20 and mdl.md_rdf_table()["next_due"] == 21 and beside["next_due"] == 20


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
    hmin = _hmin(fr)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    _, _, rows, _ = _run(fr, None, cuts=(4,), record=False, seed=77)
    UNS, INV = _lib.E_UNSUPPORTED, _lib.E_INVALID

    def vh(every=1, levels=4, rmax=0.5, rbins=8, tbins=2, pbins=2, dmax=0.4 * hmin, dbins=8):
        return lib.sgpr_md_vanhove(h, every, levels, rmax, rbins, tbins, pbins, dmax, dbins)

    def read():
        return lib.sgpr_md_vanhove_read(h, None, None, None, None, None, None)

    def words(w):
        assert w in lib.sgpr_last_error(), lib.sgpr_last_error()
    mdl.md_end()
    assert vh() == INV and read() == INV                                                  # no run
    _begin(mdl, fr, seed=77)
    for bad, figure in ((dict(every=-1), b"every"), (dict(levels=0), b"levels"), (dict(levels=33), b"levels <= 32"), (dict(rbins=0), b"rbins = 0"),
                        (dict(rbins=2049), b"rbins = 2049"), (dict(tbins=65), b"tbins = 65"), (dict(pbins=0), b"pbins = 0"), (dict(rmax=0.0), b"rmax > 0"),
                        (dict(dbins=2049), b"dbins = 2049"), (dict(dbins=-1), b"dbins = -1"), (dict(dmax=0.0), b"dmax > 0")):
        assert vh(**bad) == INV, bad
        words(figure)
    assert read() == INV                                                                  # a run without the accumulator
    ct = np.ones(2)
    assert lib.sgpr_md_vanhove_edges(h, _lib.ptr(ct), _lib.ptr(ct), _lib.ptr(ct)) == INV
    assert vh(levels=32, rbins=2048, tbins=64, pbins=64) == UNS                           # 32 S 2048 64 64 8 B
    words(b"at most 1 GiB")
    assert vh(dmax=2.6 * hmin) == UNS
    words(b"needs images 3 cells away")
    assert vh(dmax=2.4 * hmin) == 0 and vh(dbins=0, dmax=0.0) == 0 and read() == 0
    # a barostat
    ext = np.array([-GPA] * 3 + [0.0] * 3)
    baro = lambda: lib.sgpr_md_barostat(h, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0)
    _begin(mdl, fr, nh=True)
    assert vh() == 0 and baro() == UNS
    words(b"sgpr_md_barostat: the run accumulates van Hove functions")
    _begin(mdl, fr, nh=True)
    assert baro() == 0 and vh() == UNS
    words(b"sgpr_md_vanhove: the run has a barostat")
    # a relaxation
    _begin(mdl, fr)
    assert vh() == 0 and lib.sgpr_md_relax(h, 0.05, None, 0, None) == UNS
    words(b"sgpr_md_relax: the run accumulates van Hove functions")
    _begin(mdl, fr)
    assert lib.sgpr_md_relax(h, 0.05, None, 0, None) == 0 and vh() == UNS
    words(b"sgpr_md_vanhove: the run is a relaxation")
    # a band
    band = np.ascontiguousarray(_band(pos, 1))
    _begin(mdl, fr)
    assert vh() == 0 and lib.sgpr_md_neb(h, 1, _lib.ptr(band[1:2]), 0.05, 0.1, 0, None) == UNS
    words(b"sgpr_md_neb: the run accumulates van Hove functions")
    mdl.neb_begin(numbers, band, cell, pbc, 0.05)
    assert vh() == UNS
    words(b"sgpr_md_vanhove: the run is a nudged elastic band")
    # a polymer
    _, beads, bvel, _ = _polymer(numbers, pos, 2)
    _begin(mdl, fr)
    assert vh() == 0 and lib.sgpr_md_pimd(h, 2, _lib.ptr(np.ascontiguousarray(beads)), _lib.ptr(np.ascontiguousarray(bvel)), kB * T, 0.001, 1.0) == UNS
    words(b"sgpr_md_pimd: the run accumulates van Hove functions")
    _begin_pimd(mdl, numbers, beads, bvel, mass, cell, pbc, seed=7)
    assert vh() == UNS
    words(b"sgpr_md_vanhove: the run is a ring polymer")
    # a committee
    member, _ = _model(seed=2)
    arr = (C.c_void_p * 1)(member.handle.value)
    _begin(mdl, fr)
    assert vh() == 0 and lib.sgpr_md_committee(h, 1, arr) == UNS
    words(b"sgpr_md_committee: the run accumulates van Hove functions")
    _begin(mdl, fr)
    assert lib.sgpr_md_committee(h, 1, arr) == 0 and vh() == UNS
    words(b"sgpr_md_vanhove: the run has a committee")
    with pytest.raises(NotImplementedError, match="committee"):
        mdl.md_vanhove(1, 4, 0.5, 8)
    mdl.md_end()
    member.close()
    # beside a mask, the filter, a bias and the record it attaches (test_variants, test_run_md: held, the record); the filter here
    _begin(mdl, fr, seed=77, ml_filter=0.5)
    assert vh() == 0
    # a run that has started; a detach is always taken
    _begin(mdl, fr, seed=77)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and vh() == INV
    words(b"sgpr_md_vanhove: the run has started")
    assert lib.sgpr_md_vanhove(h, 0, 0, 0.0, 0, 0, 0, 0.0, 0) == 0
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
    with Watchdog(f"van Hove functions on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_vanhove(mdl.handle, 1, 4, 0.5, 8, 1, 1, 0.0, 0)
        msg = bytes(_lib.load().sgpr_last_error())
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1, msg))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    """Van Hove functions are accumulated on one rank (test_hip_msd_device.py's two-rank refusal, for sgpr_md_vanhove)."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 40)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, e0, e1, msg in got:
        assert code == _lib.E_UNSUPPORTED and e0 == e1 and b"sgpr_md_vanhove: the run was begun on 2 ranks" in msg
    assert got[0][2] == got[1][2]


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """ActiveCalculator.run_md(vanhove=holder) with a teacher — the gate fires, calculate() updates the model, the run goes on —
    on the device (the accumulator inside the loop) and through the host loop (VanHoveCounts fed every step's positions): the
    same trajectory (rng= given), so the same tables."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.transport import VanHove, displacement_histogram, distinct_van_hove, non_gaussian, self_van_hove
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
        holder = VanHove(2, 4, 0.6, 12, 4, 6, dmax=5.0, dbins=25)
        out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, rng=np.random.default_rng(9), chunk=16, vanhove=holder))
        assert len(out) == steps + 1
        upd.append([o[0] for o in out if o[3]])
        tabs.append(holder.table())
        calc.engine.close()
    print(f"updates at steps {upd}, counts {list(tabs[0]['count'])}, self per level host {tabs[0]['self'].sum(axis=(1, 2, 3, 4)).tolist()} device "
          f"{tabs[1]['self'].sum(axis=(1, 2, 3, 4)).tolist()}, distinct host {tabs[0]['distinct'].sum(axis=(1, 2, 3)).tolist()} device {tabs[1]['distinct'].sum(axis=(1, 2, 3)).tolist()}")
    assert upd[0] == upd[1] and len(upd[0]) >= 1, upd        # (the device loop halted and went on)
    assert list(tabs[0]["count"]) == [20, 10, 5, 2] and tabs[0]["self"].sum() > 0 and tabs[0]["distinct"].sum() > 0
    for k in TABLES + SETTINGS + ("samples",):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    Z = int(np.unique(numbers)[0])
    r, t, p, h, rho = displacement_histogram(holder, 0, Z)
    assert h.shape == (12, 4, 6) and 0.0 < h.sum() <= 1.0 + 1e-12 and rho > 0.0
    assert np.all(np.isfinite(self_van_hove(holder)[1][Z])) and np.isfinite(non_gaussian(holder)[Z]).all()
    assert all(np.all(np.isfinite(g)) for g in distinct_van_hove(holder)[1].values())
