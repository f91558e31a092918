"""GPU tests of the velocity-correlation accumulator of the device MD loop (sgpr_md_vacf / sgpr_md_vacf_read; the four kernels of
md_vacf.inc behind a sampled evaluation) against its host twin and definition workloads.VacfRing, bit for bit: the twin is fed
the observer's velocities (workloads.observer_velocities) of the SAME run's frame record at every = 1, so the accumulator is
exercised beside the record.  One call and a cut run, other settings, held components, Nose-Hoover, device deviates, frames whose
species segments end off a wave and span several chunks, a covloss halt in the middle with and without a model update between
the calls (the store that the repeat overwrites, the next_due guard, the speculative evaluation), a run that is not disturbed,
what a later run and the handle's memory owe to it, md_msd and md_rdf beside it, every refusal in both directions, and
ActiveCalculator.run_md(vacf=) on the device against the host loop.  Frame and model are those of test_hip_npt_device.py (LiPS,
side 8: 192 / 64 / 256 atoms, m = 48)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from test_hip_msd_device import T, _begin, _frame, _noise, _shared
from test_hip_npt_device import _model

pytestmark = pytest.mark.gpu

EVALS = 40
KEYS = ("tracer", "collective", "count", "lags", "species", "n")


def _run(fr, vacf, cuts=(EVALS,), nh=False, record=True, seed=None, msd=None, rdf=None, **kw):
    """A run of sum(cuts) evaluations on the module's model with the accumulator `vacf` = (every, lags, origin_every, com) or None.
    Returns (table or None, the observer's velocities [evals, N, 3] from the frame record or None, scalar rows, final state,
    dict of the other accumulators' tables)."""
    mdl = _shared()[0]
    _begin(mdl, fr, nh=nh, **({} if seed is None else dict(seed=seed)), **kw)
    if record:
        mdl.md_record(1, velocities=True, results=True)
    if msd is not None:
        mdl.md_msd(*msd)
    if rdf is not None:
        mdl.md_rdf(*rdf)
    if vacf is not None:
        mdl.md_vacf(*vacf)
    noise = None if (nh or seed is not None) else _noise(fr, sum(cuts))
    rows, vpre, F, t = [], [], [], 0
    for n in cuts:
        t_call = time.perf_counter()
        sc, code = mdl.md_run(n, None if noise is None else noise[t:t + n])
        print(f"md_run({n}) on {len(fr[0])} atoms, accumulator {vacf}: {1e6 * (time.perf_counter() - t_call) / n:.1f} us per evaluation")
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
        if record:
            f = mdl.md_frames(closed=False)
            assert list(f["index"]) == list(range(t, t + n))
            vpre.append(f["velocities_pre"].copy())
            F.append(f["forces"].copy())
        t += n
    state = mdl.md_state()
    vs = None
    if record:
        vs = _observed(fr, np.concatenate(vpre), np.concatenate(F), state, nh, kw.get("fixed"))
    other = dict(msd=None if msd is None else mdl.md_msd_table(), rdf=None if rdf is None else mdl.md_rdf_table())
    return (None if vacf is None else mdl.md_vacf_table()), vs, np.array(rows), state, other


def _observed(fr, vpre, F, state, nh, fixed):
    """The velocities an observer sees at the recorded configurations.  Langevin / velocity Verlet: the frame's velocities_pre
    with the closing half kick of the frame's forces (every frame but the first); Nose-Hoover: the centred velocity of n is what
    the integrator holds at n + 1 — the velocities_pre of frame n + 1, the final state's for the last."""
    from autoforce_amd.workloads import FS, observer_velocities
    hdt = 0.5 * (1.0 * FS)
    if nh:
        held = list(vpre[1:]) + [state["velocities_pre"]]
        return np.array([observer_velocities(v, None, fr[4], hdt, 0, fixed) for v in held])
    return np.array([observer_velocities(vpre[n], F[n], fr[4], hdt, 1 if n > 0 else 0, fixed) for n in range(len(vpre))])


def _twin(fr, vacf, vs):
    from autoforce_amd.workloads import VacfRing
    tw = VacfRing(vacf[0], vacf[1], vacf[2], vacf[3], fr[4], fr[0], _shared()[0].species)
    for v in vs:
        tw.add(v)
    return tw.table()


def _same(tab, want, what=""):
    print(f"{what}: count {list(tab['count'][:8])} samples {tab['samples']} pending {tab['pending']} next_due {tab['next_due']} tracer[0] device "
          f"{list(tab['tracer'][0])} twin {list(want['tracer'][0])} collective[1, 0] device {list(tab['collective'][min(1, len(tab['count']) - 1), 0])} "
          f"twin {list(want['collective'][min(1, len(tab['count']) - 1), 0])}")
    for k in KEYS:
        assert np.array_equal(tab[k], want[k]), (what, k, np.abs(np.asarray(tab[k], float) - want[k]).max())
    for k in ("samples", "pending", "next_due"):
        assert tab[k] == want[k], (what, k, tab[k], want[k])


def test_one_call_and_a_cut_run_equal_the_twin():
    fr, vacf = _frame(), (1, 16, 1, False)
    tab, vs, rows, st, _ = _run(fr, vacf)
    want = _twin(fr, vacf, vs)
    assert list(want["count"]) == [39 - k for k in range(16)] and np.all(want["tracer"][0] > 0.0)
    assert want["samples"] == 39 and want["pending"] == 1 and want["next_due"] == 40
    _same(tab, want, "one call")
    tab2, vs2, rows2, st2, _ = _run(fr, vacf, cuts=(7, 1, 12, 20))
    assert np.array_equal(vs2, vs) and np.array_equal(rows2, rows)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st[key], st2[key]), key
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "origin3", "lags4", "lags64", "lags13", "com", "held", "nose-hoover", "seed"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    vacf = {"every3": (3, 6, 1, False), "origin3": (1, 8, 3, False), "lags4": (1, 4, 1, False), "lags64": (1, 64, 1, False),
            "lags13": (1, 13, 2, True), "com": (1, 16, 1, True)}.get(variant, (1, 16, 1, False))
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, vs, _, _, _ = _run(fr, vacf, nh=(variant == "nose-hoover"), seed=77 if variant == "seed" else None, **kw)
    want = _twin(fr, vacf, vs)
    if variant == "every3":
        assert list(want["count"]) == [13, 12, 11, 10, 9, 8] and list(want["lags"]) == [0, 3, 6, 9, 12, 15]
    if variant == "origin3":
        assert list(want["count"]) == [13, 13, 13, 12, 12, 12, 11, 11]
    if variant == "lags4":
        assert list(want["count"]) == [39, 38, 37, 36]
    if variant == "lags64":
        assert list(want["count"]) == [39 - k for k in range(39)] + [0] * 25 and not want["tracer"][39:].any()
    if variant == "held":   # (a held component has velocity exactly 0 at every sample)
        assert kw["fixed"].any() and not vs[:, kw["fixed"]].any()
    assert np.all(want["tracer"][0] > 0.0)
    _same(tab, want, variant)


@pytest.mark.parametrize("kind", ["sub200", "chunks"])
def test_segments_off_a_wave_and_over_several_chunks(kind):
    from autoforce_amd.workloads import VACF_CHUNK
    fr, vacf = _frame(kind), (1, 6, 1, True)
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert n.min() < 64 and np.all(n % 64 != 0) and np.all(np.cumsum(n) % 64 != 0)
    else:
        assert VACF_CHUNK < n.max() < 2 * VACF_CHUNK and n.min() < 128
    tab, vs, _, _, _ = _run(fr, vacf, cuts=(5, 11))
    want = _twin(fr, vacf, vs)
    assert np.array_equal(want["n"], n) and np.all(want["tracer"][0] > 0.0)
    _same(tab, want, kind)


def test_a_covloss_halt_counts_the_configuration_once_with_the_forces_that_stand():
    """The gate fires at evaluation k inside a call: k has been stored and k - 1 correlated (the halt of k is known one
    evaluation late), the speculative evaluation k + 1 behind it must stay out.  The repeat of k — resumed as
    device_loop.batches resumes: one ungated evaluation, then on — stores again and does not correlate again.  With the model
    unchanged the table is the one of the run that never halted.  With the model changed between the calls the forces of k,
    and so its velocity, are the repeat's: the twin is fed from the record, which holds the repeat's frame of k."""
    fr, vacf, evals = _frame(), (1, 8, 1, False), 24
    want, vs, rows, state, _ = _run(fr, vacf, cuts=(evals,), seed=77)
    _same(want, _twin(fr, vacf, vs), "the run that never halted")
    b = rows[:, 11]
    ks = [k for k in range(2, evals - 2) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    ediff = 0.5 * (b[:k].max() + b[k])
    print(f"halt at evaluation {k} of {evals}: covloss {b[k]:.6e} over {b[:k].max():.6e}")
    mdl = _shared()[0]
    mu0, vs0 = np.array(mdl.mu, float), dict(mdl._vscale)   # (the update changes the weights alone and puts them back)
    for update in (False, True):
        _begin(mdl, fr, seed=77)
        mdl.md_record(1, velocities=True, results=True)
        mdl.md_vacf(*vacf)
        vpre, F = [], []

        def frames():
            f = mdl.md_frames(closed=False)
            vpre.append(f["velocities_pre"].copy()); F.append(f["forces"].copy())
        try:
            sc, code = mdl.md_run(evals, None, ediff=ediff)
            assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
            frames()
            mid = mdl.md_vacf_table()
            assert (mid["next_due"], mid["samples"], mid["pending"], mid["count"][0]) == (k + 1, k, 1, k)
            if update:
                mdl.set_weights(1.5 * mu0, choli=mdl.choli, vscale=vs0)
            sc1, code = mdl.md_run(1, None, ediff=0.0)
            assert code == 0 and len(sc1) == 1
            frames()
            again = mdl.md_vacf_table()
            assert (again["next_due"], again["samples"]) == (k + 1, k)
            for key in ("tracer", "collective", "count"):   # (the repeat stores, it does not correlate)
                assert np.array_equal(again[key], mid[key]), key
            sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
            assert code == 0
            frames()
            tab = mdl.md_vacf_table()
            vpre_, F_ = np.concatenate(vpre), np.concatenate(F)
            assert len(vpre_) == evals
            got_vs = _observed(fr, vpre_, F_, None, False, None)
            if update:
                assert not np.array_equal(got_vs[k], vs[k]) and np.array_equal(got_vs[:k], vs[:k])   # (other forces at k, the same walk up to it)
                _same(tab, _twin(fr, vacf, got_vs), f"halt at {k}, the model updated")
                assert not np.array_equal(tab["tracer"], want["tracer"])
            else:
                assert np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows) and np.array_equal(got_vs, vs)
                _same(tab, want, f"halt at {k}, the model unchanged")
        finally:
            if update:
                mdl.set_weights(mu0, choli=mdl.choli, vscale=vs0)
    _, _, rows_after, _, _ = _run(fr, None, cuts=(evals,), seed=77, record=False)   # (the module's model is the one it was)
    assert np.array_equal(rows_after, rows)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    fr = _frame()
    _, _, rows0, st0, _ = _run(fr, None, cuts=(9, 11), nh=nh, record=False)
    tab, _, rows1, st1, _ = _run(fr, (2, 5, 1, True), cuts=(9, 11), nh=nh, record=False)
    print(f"nh {nh}: count {list(tab['count'])}, E of the last row without / with {rows0[-1, 0]!r} / {rows1[-1, 0]!r}")
    assert list(tab["count"]) == [9, 8, 7, 6, 5] and np.array_equal(rows0, rows1)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st0[key], st1[key]), key


def test_a_later_run_and_the_memory_owe_it_nothing():
    """The test_hip_md_restart.py rule: a run begun behind an accumulator run is the run on a fresh handle; a later accumulator
    run on the same handle starts from a zero table; the table is the run's (md_vacf_table refuses the plain run); a detach
    gives the rings back, and close() every byte."""
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
    mdl.md_vacf(1, 6, 1, True)
    sc, code = mdl.md_run(10, None)
    one = mdl.md_vacf_table()
    assert code == 0 and one["count"][0] == 9
    again = R()
    assert np.array_equal(first[0], again[0])
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(first[1][key]), np.asarray(again[1][key])), key
    tr = np.zeros((6, 3))
    assert _lib.load().sgpr_md_vacf_read(mdl.handle, _lib.ptr(tr), None, None, None) == _lib.E_INVALID
    assert b"call sgpr_md_begin and sgpr_md_vacf first" in _lib.load().sgpr_last_error()
    _begin(mdl, fr, seed=7)
    mdl.md_vacf(1, 6, 1, True)
    zero = mdl.md_vacf_table()        # (a later run starts from a zero table)
    assert (zero["samples"], zero["pending"], zero["next_due"]) == (0, 0, 0)
    assert not zero["count"].any() and not zero["tracer"].any() and not zero["collective"].any()
    sc, code = mdl.md_run(10, None)
    two = mdl.md_vacf_table()
    for key in KEYS:
        assert np.array_equal(one[key], two[key]), key
    # a detach frees the rings
    mdl.md_end()
    _begin(mdl, fr, seed=7)
    plain = _live()
    mdl.md_vacf(1, 32, 1, False)
    held = _live()
    assert held[0] - plain[0] >= 33 * 24 * len(fr[0]) and held[1] > plain[1]
    mdl.md_vacf(0, 0)
    assert np.array_equal(_live(), plain)
    mdl.md_vacf(1, 6, 1, True)
    mdl.md_end()                      # (the rings and the tables go with the run)
    mdl.close()
    assert np.array_equal(_live() - before, [0, 0])


def test_beside_md_msd_and_md_rdf_every_table_is_the_one_of_a_run_alone():
    fr = _frame()
    vacf, msd, rdf = (2, 7, 1, True), (3, 3, True), (4, 5.0, 50, 0.0)
    v_alone, _, rows, _, _ = _run(fr, vacf, record=False, seed=77)
    _, _, _, _, m_alone = _run(fr, None, record=False, seed=77, msd=msd)
    _, _, _, _, r_alone = _run(fr, None, record=False, seed=77, rdf=rdf)
    v_all, _, rows_all, _, other = _run(fr, vacf, record=False, seed=77, msd=msd, rdf=rdf)
    assert np.array_equal(rows, rows_all) and list(v_all["count"]) == [19 - k for k in range(7)]
    _same(v_all, v_alone, "beside md_msd and md_rdf")
    for k in ("count", "msd", "msd_sq", "smd", "smd_sq", "samples", "next_due"):
        assert np.array_equal(other["msd"][k], m_alone["msd"][k]), k
    for k in ("hist", "samples", "next_due"):
        assert np.array_equal(other["rdf"][k], r_alone["rdf"][k]), k
    assert other["msd"]["next_due"] == 42 and other["rdf"]["next_due"] == 40 and v_all["next_due"] == 40


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

    def vacf():
        return lib.sgpr_md_vacf(h, 1, 4, 1, 0)

    def words(w):
        assert w in lib.sgpr_last_error(), lib.sgpr_last_error()
    mdl.md_end()
    assert vacf() == INV and lib.sgpr_md_vacf_read(h, None, None, None, None) == INV     # no run
    _begin(mdl, fr, seed=77)
    for every, lags, oe, com in ((-1, 4, 1, 0), (1, 0, 1, 0), (1, 4, 0, 0), (1, 4, 1, 2), (1, 4, 1, -1)):
        assert lib.sgpr_md_vacf(h, every, lags, oe, com) == INV
    assert lib.sgpr_md_vacf_read(h, None, None, None, None) == INV                       # a run without the accumulator
    assert lib.sgpr_md_vacf(h, 1, 8193, 1, 0) == UNS                                     # the compiled limit
    words(b"at most 8192 lags")
    assert lib.sgpr_md_vacf(h, 1, 8192, 1, 0) == 0 and lib.sgpr_md_vacf(h, 0, 0, 0, 0) == 0
    # a barostat
    ext = np.array([-GPA] * 3 + [0.0] * 3)
    baro = lambda: lib.sgpr_md_barostat(h, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0)
    _begin(mdl, fr, nh=True)
    assert vacf() == 0 and baro() == UNS
    words(b"sgpr_md_barostat: the run accumulates velocity correlations")
    _begin(mdl, fr, nh=True)
    assert baro() == 0 and vacf() == UNS
    words(b"sgpr_md_vacf: the run has a barostat")
    # a relaxation
    _begin(mdl, fr)
    assert vacf() == 0 and lib.sgpr_md_relax(h, 0.05, None, 0, None) == UNS
    words(b"sgpr_md_relax: the run accumulates velocity correlations")
    _begin(mdl, fr)
    assert lib.sgpr_md_relax(h, 0.05, None, 0, None) == 0 and vacf() == UNS
    words(b"sgpr_md_vacf: the run is a relaxation")
    # a band
    band = np.ascontiguousarray(_band(pos, 1))
    _begin(mdl, fr)
    assert vacf() == 0 and lib.sgpr_md_neb(h, 1, _lib.ptr(band[1:2]), 0.05, 0.1, 0, None) == UNS
    words(b"sgpr_md_neb: the run accumulates velocity correlations")
    mdl.neb_begin(numbers, band, cell, pbc, 0.05)
    assert vacf() == UNS
    words(b"sgpr_md_vacf: the run is a nudged elastic band")
    # a polymer
    _, beads, bvel, _ = _polymer(numbers, pos, 2)
    _begin(mdl, fr)
    assert vacf() == 0 and lib.sgpr_md_pimd(h, 2, _lib.ptr(np.ascontiguousarray(beads)), _lib.ptr(np.ascontiguousarray(bvel)), kB * T, 0.001, 1.0) == UNS
    words(b"sgpr_md_pimd: the run accumulates velocity correlations")
    _begin_pimd(mdl, numbers, beads, bvel, mass, cell, pbc, seed=7)
    assert vacf() == UNS
    words(b"sgpr_md_vacf: the run is a ring polymer")
    # the filter: its closing kick uses the filtered force
    _begin(mdl, fr)
    assert vacf() == 0 and lib.sgpr_md_filter(h, 0.5, None, None) == UNS
    words(b"sgpr_md_filter: the run accumulates velocity correlations")
    words(b"packed force")
    _begin(mdl, fr)
    assert lib.sgpr_md_filter(h, 0.5, None, None) == 0 and vacf() == UNS
    words(b"sgpr_md_vacf: the run has a filter")
    words(b"not the packed one")
    with pytest.raises(NotImplementedError, match="filter"):
        mdl.md_vacf(1, 4)
    # a bias: its closing kick uses the biased force
    cvs, sigma = np.array([[0, 0, 1]], dtype=np.int32), np.array([0.1])
    meta = lambda: lib.sgpr_md_meta(h, 1, _lib.ptr(cvs), _lib.ptr(sigma), 0.01, 0.0, 1, 64, 0, None, None)
    _begin(mdl, fr)
    assert vacf() == 0 and meta() == UNS
    words(b"sgpr_md_meta: the run accumulates velocity correlations")
    words(b"packed force")
    _begin(mdl, fr)
    assert meta() == 0 and vacf() == UNS
    words(b"sgpr_md_vacf: the run has a bias")
    words(b"not the packed one")
    # a committee
    member, _ = _model(seed=2)
    arr = (C.c_void_p * 1)(member.handle.value)
    _begin(mdl, fr)
    assert vacf() == 0 and lib.sgpr_md_committee(h, 1, arr) == UNS
    words(b"sgpr_md_committee: the run accumulates velocity correlations")
    _begin(mdl, fr)
    assert lib.sgpr_md_committee(h, 1, arr) == 0 and vacf() == UNS
    words(b"sgpr_md_vacf: the run has a committee")
    with pytest.raises(NotImplementedError, match="committee"):
        mdl.md_vacf(1, 4)
    mdl.md_end()
    member.close()
    # a run that has started; a detach is always taken
    _begin(mdl, fr, seed=77)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and vacf() == INV
    words(b"sgpr_md_vacf: the run has started")
    assert lib.sgpr_md_vacf(h, 0, 0, 0, 0) == 0
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
    with Watchdog(f"velocity correlations on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_vacf(mdl.handle, 1, 4, 1, 0)
        msg = bytes(_lib.load().sgpr_last_error())
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1, msg))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    """Velocity correlations are accumulated on one rank (test_hip_msd_device.py's two-rank refusal, for sgpr_md_vacf)."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29910 + (os.getpid() % 40)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, e0, e1, msg in got:
        assert code == _lib.E_UNSUPPORTED and e0 == e1 and b"sgpr_md_vacf: the run was begun on 2 ranks" in msg
    assert got[0][2] == got[1][2]


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """ActiveCalculator.run_md(vacf=holder) with a teacher — the gate fires, calculate() updates the model, the run goes on —
    on the device (the accumulator inside the loop: the sample of a halting configuration is the repeat's) and through the host
    loop (VacfRing fed every step's velocities): the same trajectory (rng= given), so the same tables, bit for bit."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.transport import Vacf, green_kubo, onsager, vibrational_dos
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
        holder = Vacf(2, 6, 1, True)
        out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, rng=np.random.default_rng(9), chunk=16, vacf=holder))
        assert len(out) == steps + 1
        upd.append([o[0] for o in out if o[3]])
        tabs.append(holder.table())
        calc.engine.close()
    print(f"updates at steps {upd}, counts {list(tabs[0]['count'])}, tracer[0] host {list(tabs[0]['tracer'][0])} device {list(tabs[1]['tracer'][0])}")
    assert upd[0] == upd[1] and len(upd[0]) >= 1, upd        # (the device loop halted and went on)
    assert list(tabs[0]["count"]) == [20, 19, 18, 17, 16, 15] and tabs[0]["samples"] == 20
    for k in KEYS + ("samples",):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    D = green_kubo(holder, 1.0)
    assert set(D) == set(int(z) for z in np.unique(numbers)) and all(np.isfinite(v["value"]) for v in D.values())
    assert np.all(np.isfinite(onsager(holder, 1.0)[1])) and all(np.all(np.isfinite(g)) for g in vibrational_dos(holder, 1.0)[1].values())
