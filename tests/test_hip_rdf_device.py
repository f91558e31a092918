"""GPU tests of the pair-distance accumulator of the device MD loop (sgpr_md_rdf / sgpr_md_rdf_read; md_rdf_pair_kernel and
md_rdf_done_kernel behind a sampled evaluation) against its host twin and definition workloads.RdfCounts: the twin is fed the
positions of the SAME run's frame record at every = 1, and every integer must be equal.  One call and a cut run, other settings,
held components, Nose-Hoover, the single-image form and the image block (rmax beyond half the cell; a cell thinner than rmax, so
self-images), frames whose species segments end off a tile and span several tiles, a covloss halt in the middle (the next_due
guard and the speculative evaluation), a run that is not disturbed, the displacement accumulator beside it, what a later run and
the handle's memory owe to it, every refusal in both directions, and ActiveCalculator.run_md(rdf=) on the device against the host
loop.  Frame, model, run loop and the bodies the six accumulators share: accumulator_device.py (cubic 21.76 A)."""
import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import EVALS, _begin, _frame, _shared

pytestmark = pytest.mark.gpu

RDF = (1, 6.0, 60, 0.0)      # every, rmax, bins, rmin: the single-image form on the module's frame
RDF12 = (1, 12.0, 48, 0.5)   # rmax beyond half the cell: the image block with R = 1
INTS = ("hist", "species", "n")


def _run(fr, rdf, **kw):
    """accumulator_device.run with the accumulator `rdf` = (every, rmax, bins, rmin) or None.  Returns (table or None, recorded
    positions or None, scalar rows, final state)."""
    tabs, xs, rows, state = A.run(fr, *A.attached(rdf=rdf), label=f"accumulator {rdf}", **kw)
    return tabs.get("rdf"), xs, rows, state


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


def _limits(c):
    assert c.raw(rmax=54.0) == 0 and c.raw(rmax=55.0) == c.UNS                          # 2.5 heights of 21.76 = 54.4
    c.words(b"against the cell height 21.76 along direction 0")
    with pytest.raises(NotImplementedError, match="cell height"):
        c.mdl.md_rdf(1, 55.0)


ACC = A.Acc(name="rdf", noun=b"pair distances", moving_cell=b"the image block and the densities are those of a constant cell", polymer=b"beads are",
            raw=lambda h, every=1, rmin=0.0, rmax=6.0, bins=60: A.lib().sgpr_md_rdf(h, every, rmin, rmax, bins),
            detach=lambda h: A.lib().sgpr_md_rdf(h, 0, 0.0, 6.0, 60), read=lambda h: A.lib().sgpr_md_rdf_read(h, None, None, None),
            py=lambda mdl: mdl.md_rdf(1, 6.0), limits=_limits,
            invalid=[dict(every=-1), dict(bins=0), dict(bins=2049), dict(rmin=-0.5), dict(rmin=6.0), dict(rmin=7.0), dict(rmax=float("nan"))],
            port=29920, run=_run, twin=lambda fr, rdf, xs: _twin(fr, rdf, xs).table(), same=_same)


def test_one_call_and_a_cut_run_equal_the_twin():
    fr = _frame()
    tab, xs, rows, _ = _run(fr, RDF)
    tw = _twin(fr, RDF, xs)
    want = tw.table()
    assert not tw.R.any() and want["samples"] == EVALS and np.all(want["hist"].sum(axis=2) > 0)
    _same(tab, want, "one call")
    assert np.array_equal(tab["hist"], tab["hist"].transpose(1, 0, 2))
    tab2, xs2, rows2, _ = _run(fr, RDF, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 20")


@pytest.mark.parametrize("variant", ["every3", "held", "nose-hoover"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    rdf = (3, 6.0, 60, 0.0) if variant == "every3" else RDF
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _ = _run(fr, rdf, cuts=(20,), nh=(variant == "nose-hoover"), **kw)
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
    tab, xs, _, _ = _run(fr, RDF12, cuts=(2, 4))
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
    tab, xs, _, _ = _run(fr, rdf, cuts=(2, 3))
    tw = _twin(fr, rdf, xs)
    assert bool(tw.R.any()) == (rdf[1] > 10.0)
    want = tw.table()
    assert np.array_equal(want["n"], n) and np.all(want["hist"].sum(axis=2) > 0)
    _same(tab, want, f"{kind} {rdf}")


def test_a_covloss_halt_counts_every_configuration_once():
    def halted(mid, k, xs):
        assert mid["samples"] == k + 1
        _same(mid, _twin(_frame(), RDF, xs[:k + 1]).table(), f"behind the halt at {k}")
    A.halt_counts_once(ACC, RDF, halted)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    A.moves_nothing(ACC, nh, (2, 6.0, 60, 0.0), lambda tab: tab["samples"] == 10, record=True)


def test_displacements_and_pair_distances_together_equal_each_alone():
    fr, msd, rdf = _frame(), (2, 3, True), (3, 6.0, 60, 0.0)
    kw = dict(cuts=(9, 11), record=False, seed=5)
    both, _, rows, _ = A.run(fr, *A.attached(msd=msd, rdf=rdf), **kw)
    alone, _, rows_r, _ = _run(fr, rdf, **kw)
    malone, _, rows_m, _ = A.run(fr, *A.attached(msd=msd), **kw)
    assert np.array_equal(rows, rows_r) and np.array_equal(rows, rows_m)
    assert both["rdf"]["samples"] == 7 and both["rdf"]["next_due"] == 21 and both["msd"]["samples"] == 10 and both["msd"]["next_due"] == 20
    _same(both["rdf"], alone, "beside md_msd")
    for k in ("count", "msd", "msd_sq", "smd", "smd_sq"):
        assert np.array_equal(both["msd"][k], malone["msd"][k]), k


def test_a_later_run_starts_from_zeros_and_the_memory_owes_it_nothing():
    """accumulator_device.later_run_and_memory; a second attach on the same handle zeroes the table; md_rdf_table refuses the
    plain run; a detach gives the table back at once, md_end and close() every byte."""
    from test_hip_teardown import _live

    def accumulate(mdl, fr):
        def attach_and_run():
            _begin(mdl, fr, seed=7)
            mdl.md_rdf(*RDF)
            assert not mdl.md_rdf_table()["hist"].any() and mdl.md_rdf_table()["samples"] == 0
            sc, code = mdl.md_run(6, None)
            assert code == 0
            return mdl.md_rdf_table()
        t1 = attach_and_run()
        t2 = attach_and_run()
        assert t1["samples"] == 6 and t1["hist"].sum() > 0
        _same(t2, t1, "the second attach")

    def detach(mdl, fr, first):
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
    A.later_run_and_memory(ACC, accumulate, detach)


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    A.two_rank_refusal(ACC)


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(rdf=holder), the host loop's RdfCounts fed every step's positions:
    the same integers."""
    from autoforce_amd.transport import Rdf, radial_distribution
    # (rmax beyond half the cell and the model's rc)
    tabs, holder, numbers = A.run_md_host_and_device(
        tmp_path, "rdf", lambda cell: Rdf(2, 0.9 * float(np.linalg.norm(np.asarray(cell).reshape(3, 3), axis=1).min()), 50))
    print(f"samples {tabs[0]['samples']}, counts host {int(tabs[0]['hist'].sum())} device {int(tabs[1]['hist'].sum())}")
    assert tabs[0]["samples"] == 21 and tabs[0]["hist"].sum() > 0
    _same(tabs[1], tabs[0], "run_md")
    r, g = radial_distribution(holder)
    assert set(a for p in g for a in p) == set(int(z) for z in np.unique(numbers)) and all(np.all(np.isfinite(v)) for v in g.values())
