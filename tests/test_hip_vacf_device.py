"""GPU tests of the velocity-correlation accumulator of the device MD loop (sgpr_md_vacf / sgpr_md_vacf_read; the four kernels of
md_vacf.inc behind a sampled evaluation) against its host twin and definition workloads.VacfRing, bit for bit: the twin is fed
the observer's velocities (workloads.observer_velocities) of the SAME run's frame record at every = 1, so the accumulator is
exercised beside the record.  One call and a cut run, other settings, held components, Nose-Hoover, device deviates, frames whose
species segments end off a wave and span several chunks, a covloss halt in the middle with and without a model update between
the calls (the store that the repeat overwrites, the next_due guard, the speculative evaluation), a run that is not disturbed,
what a later run and the handle's memory owe to it, md_msd and md_rdf beside it, every refusal in both directions, and
ActiveCalculator.run_md(vacf=) on the device against the host loop.  Frame, model, run loop and the bodies the six accumulators
share: accumulator_device.py."""
import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import _begin, _frame, _shared

pytestmark = pytest.mark.gpu

KEYS = ("tracer", "collective", "count", "lags", "species", "n")
KICKS = (dict(velocities=True, results=True), dict(closed=False), ("velocities_pre", "forces"))   # the record the observer needs


def _run(fr, vacf, nh=False, record=True, **kw):
    """accumulator_device.run with the accumulator `vacf` = (every, lags, origin_every, com) or None.  Returns (table or None, the
    observer's velocities [evals, N, 3] from the frame record or None, scalar rows, final state)."""
    tabs, kept, rows, state = A.run(fr, *A.attached(vacf=vacf), nh=nh, record=record and KICKS, label=f"accumulator {vacf}", **kw)
    return tabs.get("vacf"), (_observed(fr, *kept, state, nh, kw.get("fixed")) if record else None), rows, state


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


def _limits(c):
    assert c.raw(lags=8193) == c.UNS                                                     # the compiled limit
    c.words(b"at most 8192 lags")
    assert c.raw(lags=8192) == 0 and ACC.detach(c.h) == 0


def _modes(c):
    """The filter and a bias: their closing kick uses another force than the packed one the sample takes."""
    from autoforce_amd import _lib
    cvs, sigma = np.array([[0, 0, 1]], dtype=np.int32), np.array([0.1])
    for mode, has, call in ((b"filter", b"a filter", lambda: c.lib.sgpr_md_filter(c.h, 0.5, None, None)),
                            (b"meta", b"a bias", lambda: c.lib.sgpr_md_meta(c.h, 1, _lib.ptr(cvs), _lib.ptr(sigma), 0.01, 0.0, 1, 64, 0, None, None))):
        _begin(c.mdl, c.fr)
        assert c.raw() == 0 and call() == c.UNS
        c.words(b"sgpr_md_" + mode + b": the run accumulates velocity correlations")
        c.words(b"packed force")
        _begin(c.mdl, c.fr)
        assert call() == 0 and c.raw() == c.UNS
        c.words(b"sgpr_md_vacf: the run has " + has)
        c.words(b"not the packed one")
        if mode == b"filter":
            with pytest.raises(NotImplementedError, match="filter"):
                c.mdl.md_vacf(1, 4)


ACC = A.Acc(name="vacf", noun=b"velocity correlations", moving_cell=b"velocities in a moving cell are not sampled", polymer=b"centroid is",
            raw=lambda h, every=1, lags=4, oe=1, com=0: A.lib().sgpr_md_vacf(h, every, lags, oe, com),
            detach=lambda h: A.lib().sgpr_md_vacf(h, 0, 0, 0, 0), read=lambda h: A.lib().sgpr_md_vacf_read(h, None, None, None, None),
            py=lambda mdl: mdl.md_vacf(1, 4), limits=_limits, modes=_modes,
            invalid=[dict(every=-1), dict(lags=0), dict(oe=0), dict(com=2), dict(com=-1)],
            port=29910, run=_run, twin=_twin, same=_same)


def test_one_call_and_a_cut_run_equal_the_twin():
    fr, vacf = _frame(), (1, 16, 1, False)
    tab, vs, rows, st = _run(fr, vacf)
    want = _twin(fr, vacf, vs)
    assert list(want["count"]) == [39 - k for k in range(16)] and np.all(want["tracer"][0] > 0.0)
    assert want["samples"] == 39 and want["pending"] == 1 and want["next_due"] == 40
    _same(tab, want, "one call")
    tab2, vs2, rows2, st2 = _run(fr, vacf, cuts=(7, 1, 12, 20))
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
    tab, vs, _, _ = _run(fr, vacf, nh=(variant == "nose-hoover"), seed=77 if variant == "seed" else None, **kw)
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
    tab, vs, _, _ = _run(fr, vacf, cuts=(5, 11))
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
    want, vs, rows, state = _run(fr, vacf, cuts=(evals,), seed=77)
    _same(want, _twin(fr, vacf, vs), "the run that never halted")
    k, ediff = A.first_halt(rows, evals)
    mdl = _shared()[0]
    mu0, vs0 = np.array(mdl.mu, float), dict(mdl._vscale)   # (the update changes the weights alone and puts them back)
    for update in (False, True):
        _begin(mdl, fr, seed=77)
        mdl.md_record(1, **KICKS[0])
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
    _, _, rows_after, _ = _run(fr, None, cuts=(evals,), seed=77, record=False)   # (the module's model is the one it was)
    assert np.array_equal(rows_after, rows)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    A.moves_nothing(ACC, nh, (2, 5, 1, True), lambda tab: list(tab["count"]) == [9, 8, 7, 6, 5])


def test_a_later_run_and_the_memory_owe_it_nothing():
    """accumulator_device.later_run_and_memory; a later accumulator run on the same handle starts from a zero table; the table
    is the run's (md_vacf_table refuses the plain run); a detach gives the rings back, and close() every byte."""
    from test_hip_teardown import _live
    one = {}

    def accumulate(mdl, fr):
        _begin(mdl, fr, seed=7)
        mdl.md_vacf(1, 6, 1, True)
        sc, code = mdl.md_run(10, None)
        one.update(mdl.md_vacf_table())
        assert code == 0 and one["count"][0] == 9

    def detach(mdl, fr, first):
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
    A.later_run_and_memory(ACC, accumulate, detach)


def test_beside_md_msd_and_md_rdf_every_table_is_the_one_of_a_run_alone():
    fr = _frame()
    vacf, msd, rdf = (2, 7, 1, True), (3, 3, True), (4, 5.0, 50, 0.0)
    kw = dict(record=False, seed=77)
    v_alone, _, rows, _ = _run(fr, vacf, **kw)
    m_alone = A.run(fr, *A.attached(msd=msd), **kw)[0]
    r_alone = A.run(fr, *A.attached(rdf=rdf), **kw)[0]
    both, _, rows_all, _ = A.run(fr, *A.attached(msd=msd, rdf=rdf, vacf=vacf), **kw)
    assert np.array_equal(rows, rows_all) and list(both["vacf"]["count"]) == [19 - k for k in range(7)]
    _same(both["vacf"], v_alone, "beside md_msd and md_rdf")
    for k in ("count", "msd", "msd_sq", "smd", "smd_sq", "samples", "next_due"):
        assert np.array_equal(both["msd"][k], m_alone["msd"][k]), k
    for k in ("hist", "samples", "next_due"):
        assert np.array_equal(both["rdf"][k], r_alone["rdf"][k]), k
    assert both["msd"]["next_due"] == 42 and both["rdf"]["next_due"] == 40 and both["vacf"]["next_due"] == 40


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    A.two_rank_refusal(ACC)


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(vacf=holder), on the device the sample of a halting configuration
    being the repeat's, the host loop's VacfRing fed every step's velocities: the same tables, bit for bit."""
    from autoforce_amd.transport import Vacf, green_kubo, onsager, vibrational_dos
    tabs, holder, numbers = A.run_md_host_and_device(tmp_path, "vacf", lambda cell: Vacf(2, 6, 1, True))
    print(f"counts {list(tabs[0]['count'])}, tracer[0] host {list(tabs[0]['tracer'][0])} device {list(tabs[1]['tracer'][0])}")
    assert list(tabs[0]["count"]) == [20, 19, 18, 17, 16, 15] and tabs[0]["samples"] == 20
    for k in KEYS + ("samples",):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    D = green_kubo(holder, 1.0)
    assert set(D) == set(int(z) for z in np.unique(numbers)) and all(np.isfinite(v["value"]) for v in D.values())
    assert np.all(np.isfinite(onsager(holder, 1.0)[1])) and all(np.all(np.isfinite(g)) for g in vibrational_dos(holder, 1.0)[1].values())
