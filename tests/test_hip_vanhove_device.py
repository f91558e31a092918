"""GPU tests of the van Hove accumulator of the device MD loop (sgpr_md_vanhove / _edges / _read; md_vh_pair_kernel,
md_vh_self_kernel and md_vh_done_kernel behind a sampled evaluation) against its host twin and definition
workloads.VanHoveCounts: every entry is a count, every table is compared with np.array_equal.  The twin is fed the positions of
the SAME run's frame record at every = 1, so the accumulator is exercised beside the record.  One call and a cut run, other
settings, held components, Nose-Hoover, angular bins and radial only, the distinct part with one image and with the image block,
frames whose species segments end off a wave and span several chunks and tiles, a covloss halt in the middle (the next_due guard
and the speculative evaluation), a run that is not disturbed, what a later run, a detach and the handle's memory owe to it, every
refusal in both directions, and ActiveCalculator.run_md(vanhove=) on the device against the host loop.  Frame, model, run loop and
the bodies the six accumulators share: accumulator_device.py."""
import time

import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import EVALS, _begin, _frame, _shared

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


def _run(fr, vh, **kw):
    """accumulator_device.run with the accumulator `vh` (the arguments of md_vanhove) or None.  Returns (tables or None,
    recorded positions [evals, N, 3] or None, scalar rows, final state)."""
    tabs, xs, rows, state = A.run(fr, *A.attached(vanhove=vh), label=f"accumulator {vh}", **kw)
    return tabs.get("vanhove"), xs, rows, state


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


def _raw(h, every=1, levels=4, rmax=0.5, rbins=8, tbins=2, pbins=2, dmax=None, dbins=8):
    return A.lib().sgpr_md_vanhove(h, every, levels, rmax, rbins, tbins, pbins, 0.4 * _hmin(_frame()) if dmax is None else dmax, dbins)


def _limits(c):
    from autoforce_amd import _lib
    hmin, ct = _hmin(c.fr), np.ones(2)
    assert c.lib.sgpr_md_vanhove_edges(c.h, _lib.ptr(ct), _lib.ptr(ct), _lib.ptr(ct)) == c.INV
    assert c.raw(levels=32, rbins=2048, tbins=64, pbins=64) == c.UNS                      # 32 S 2048 64 64 8 B
    c.words(b"at most 1 GiB")
    assert c.raw(dmax=2.6 * hmin) == c.UNS
    c.words(b"needs images 3 cells away")
    assert c.raw(dmax=2.4 * hmin) == 0 and c.raw(dbins=0, dmax=0.0) == 0 and c.read() == 0


def _modes(c):
    """Beside a mask, the filter, a bias and the record it attaches (test_variants, test_run_md: held, the record); the filter here."""
    _begin(c.mdl, c.fr, seed=77, ml_filter=0.5)
    assert c.raw() == 0


ACC = A.Acc(name="vanhove", noun=b"van Hove functions", moving_cell=b"displacements and the image block are those of a constant cell",
            polymer=b"beads are", raw=_raw, detach=lambda h: A.lib().sgpr_md_vanhove(h, 0, 0, 0.0, 0, 0, 0, 0.0, 0),
            read=lambda h: A.lib().sgpr_md_vanhove_read(h, None, None, None, None, None, None),
            py=lambda mdl: mdl.md_vanhove(1, 4, 0.5, 8), limits=_limits, modes=_modes,
            invalid=[(dict(every=-1), b"every"), (dict(levels=0), b"levels"), (dict(levels=33), b"levels <= 32"), (dict(rbins=0), b"rbins = 0"),
                     (dict(rbins=2049), b"rbins = 2049"), (dict(tbins=65), b"tbins = 65"), (dict(pbins=0), b"pbins = 0"), (dict(rmax=0.0), b"rmax > 0"),
                     (dict(dbins=2049), b"dbins = 2049"), (dict(dbins=-1), b"dbins = -1"), (dict(dmax=0.0), b"dmax > 0")],
            port=29800, run=_run, twin=_twin, same=_same)


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
    def halted(mid, k, xs):
        assert mid["count"][0] == k and mid["samples"] == k + 1

    def repeated(again, mid):
        for key in TABLES:
            assert np.array_equal(again[key], mid[key]), key
    A.halt_counts_once(ACC, _vh(_frame(), levels=4, heights=0.45, dbins=40), halted, repeated)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    A.moves_nothing(ACC, nh, _vh(_frame(), every=2, levels=3, heights=1.2, dbins=16), lambda tab: tab["count"][0] == 9)


def test_a_later_run_a_detach_and_the_memory_owe_it_nothing():
    """accumulator_device.later_run_and_memory; the tables are the run's (md_vanhove_table refuses the plain run), a detach
    frees the origins and the tables, and the run is the plain one."""
    from test_hip_teardown import _live
    vh = _vh(_frame(), levels=6, heights=1.2, dbins=32)

    def accumulate(mdl, fr):
        _begin(mdl, fr, seed=7)
        mdl.md_vanhove(*vh)
        sc, code = mdl.md_run(10, None)
        assert code == 0 and mdl.md_vanhove_table()["count"][0] == 9

    def detach(mdl, fr, first):
        with pytest.raises(RuntimeError):
            mdl.md_vanhove_table()
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
    A.later_run_and_memory(ACC, accumulate, detach)


def test_beside_the_other_accumulators_every_table_is_the_one_of_a_run_alone():
    fr = _frame()
    vh = _vh(fr, every=2, levels=3, heights=0.45, dbins=24)
    alone, _, rows, _ = _run(fr, vh, cuts=(20,), record=False, seed=5)
    tabs, _, rows_b, _ = A.run(fr, *A.attached(msd=(1, 4, True), rdf=(3, 4.0, 32), vacf=(1, 8), vanhove=vh), cuts=(20,), record=False, seed=5)
    assert np.array_equal(rows_b, rows)
    beside = tabs["vanhove"]
    for k in TABLES + ("samples", "next_due"):
        assert np.array_equal(beside[k], alone[k]), k
    assert tabs["msd"]["next_due"] == 20 and tabs["rdf"]["next_due"] == 21 and beside["next_due"] == 20


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    A.two_rank_refusal(ACC, dmax=0.0, dbins=0)


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(vanhove=holder), the host loop's VanHoveCounts fed every step's
    positions: the same tables."""
    from autoforce_amd.transport import VanHove, displacement_histogram, distinct_van_hove, non_gaussian, self_van_hove
    tabs, holder, numbers = A.run_md_host_and_device(tmp_path, "vanhove", lambda cell: VanHove(2, 4, 0.6, 12, 4, 6, dmax=5.0, dbins=25))
    print(f"counts {list(tabs[0]['count'])}, self per level host {tabs[0]['self'].sum(axis=(1, 2, 3, 4)).tolist()} device "
          f"{tabs[1]['self'].sum(axis=(1, 2, 3, 4)).tolist()}, distinct host {tabs[0]['distinct'].sum(axis=(1, 2, 3)).tolist()} device {tabs[1]['distinct'].sum(axis=(1, 2, 3)).tolist()}")
    assert list(tabs[0]["count"]) == [20, 10, 5, 2] and tabs[0]["self"].sum() > 0 and tabs[0]["distinct"].sum() > 0
    for k in TABLES + SETTINGS + ("samples",):
        assert np.array_equal(tabs[0][k], tabs[1][k]), k
    Z = int(np.unique(numbers)[0])
    r, t, p, h, rho = displacement_histogram(holder, 0, Z)
    assert h.shape == (12, 4, 6) and 0.0 < h.sum() <= 1.0 + 1e-12 and rho > 0.0
    assert np.all(np.isfinite(self_van_hove(holder)[1][Z])) and np.isfinite(non_gaussian(holder)[Z]).all()
    assert all(np.all(np.isfinite(g)) for g in distinct_van_hove(holder)[1].values())
