"""GPU tests of the bond-angle and coordination accumulator of the device MD loop (sgpr_md_adf / sgpr_md_adf_read; md_adf_kernel
and md_adf_done_kernel behind a sampled evaluation, reading the neighbour list the step has just built) against its host twin and
definition workloads.AdfCounts: the twin is fed the positions of the SAME run's frame record, and every integer must be equal —
no tolerance anywhere.  One call and a cut run, other settings, held components, Nose-Hoover, a thin cell (atoms under several
images and their own images in the list), species segments off the chunk of 16 centres and over many chunks, a cutoff so small
that centres have no or one neighbour, all cutoffs at the model's rc (every list entry selected, a centre's pairs over many passes
of its wave; and on a compressed frame more than 64 neighbours per centre: several passes of the gather),
an exact cubic lattice whose right angles sit ON an edge, both counter forms, a covloss halt in the middle, a run that is not disturbed, the other accumulators beside it, what a later run
and the handle's memory owe to it, every refusal in both directions, and ActiveCalculator.run_md(adf=) on the device against the
host loop.  Frame, model, run loop and the bodies the six accumulators share: accumulator_device.py (cubic 21.76 A, rc = 6)."""
import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import _begin, _shared

pytestmark = pytest.mark.gpu

RC = 6.0
# bond cutoffs over Li, P, S: distinct per pair, P-P never bonds (the rattled lattice has its shells at 2.72, 3.85 and 4.71 A)
CUT = {(3, 3): 3.1, (3, 15): 3.3, (3, 16): 4.0, (15, 16): 2.9, (16, 16): 4.2}
ADF = (1, 36, CUT)           # every, bins, cutoffs


def _frame(kind=None):
    """accumulator_device's frames (None, "sub200", "chunks", "thin"), and "dense": the module's frame compressed to 0.85 of its
    size, 73 neighbours within rc on average — no helper frame reaches 64 (the module's has 45)."""
    if kind != "dense":
        return A._frame(kind)
    numbers, pos, cell, pbc, mass, vel = A._frame(None)
    return numbers, 0.85 * pos, 0.85 * np.asarray(cell), pbc, mass, vel


def _run(fr, adf, cuts=(24,), **kw):
    """accumulator_device.run with the accumulator `adf` = (every, bins, cutoffs) or None; a capacity the model outgrows halts a
    call with the loop's overflow code, and the call is repeated.  Returns (table or None, recorded positions or None, scalar
    rows, final state)."""
    tabs, xs, rows, state = A.run(fr, *A.attached(adf=adf), cuts=cuts, overflow=True, label=f"accumulator {adf and adf[:2]}", **kw)
    return tabs.get("adf"), xs, rows, state


def _twin(fr, adf, xs):
    from autoforce_amd.workloads import AdfCounts
    tw = AdfCounts(adf[0], adf[1], adf[2], fr[0], _shared()[0].species, fr[2], fr[3])
    for x in xs:
        tw.add(x)
    return tw


def _same(tab, want, what=""):
    S = len(want["species"])
    print(f"{what}: samples {tab['samples']} next_due {tab['next_due']} angles per (centre, end <= end) device "
          f"{[int(tab['angles'][a, b, c].sum()) for a in range(S) for b in range(S) for c in range(b, S)]} twin "
          f"{[int(want['angles'][a, b, c].sum()) for a in range(S) for b in range(S) for c in range(b, S)]}; largest coordination "
          f"{int(np.flatnonzero(want['coord'].sum(axis=(0, 1))).max())}")
    for k in ("angles", "coord"):
        assert tab[k].dtype == np.uint64 and tab[k].shape == want[k].shape
    for k in ("angles", "coord", "species", "n", "cut"):
        assert np.array_equal(tab[k], want[k]), (what, k, int((np.asarray(tab[k]) != np.asarray(want[k])).sum()))
    for k in ("samples", "next_due", "every", "bins"):
        assert tab[k] == want[k], (what, k, tab[k], want[k])


def _cut0():
    from autoforce_amd.workloads import adf_cutoffs
    return adf_cutoffs(CUT, _shared()[0].species)


def _raw(h, every=1, bins=36, cut=None, ct=None):
    from autoforce_amd._lib import ptr
    from autoforce_amd.workloads import adf_edges
    cut = np.ascontiguousarray(_cut0() if cut is None else cut, dtype=np.float64)
    ct = np.ascontiguousarray(adf_edges(max(bins, 1)) if ct is None else ct, dtype=np.float64)
    return A.lib().sgpr_md_adf(h, every, bins, ptr(cut), ptr(ct))


def _invalid():
    from autoforce_amd.workloads import adf_edges
    asym, neg = _cut0(), _cut0()
    asym[0, 2] += 0.1
    neg[0, 1] = neg[1, 0] = -1.0
    return [dict(every=-1), dict(bins=0), dict(bins=1025), dict(cut=asym), dict(cut=neg), dict(cut=np.zeros((3, 3))), dict(ct=adf_edges(36)[::-1])]


def _limits(c):
    assert c.raw(cut=np.full((3, 3), RC)) == 0 and c.raw(cut=np.full((3, 3), RC + 0.5)) == c.UNS
    c.words(b"lies beyond the model's cutoff 6")
    with pytest.raises(NotImplementedError, match="beyond the model's cutoff"):
        c.mdl.md_adf(1, 36, {(15, 16): 6.5})
    with pytest.raises(ValueError):
        c.mdl.md_adf(1, 36)


ACC = A.Acc(name="adf", noun=b"bond angles", moving_cell=b"the neighbours are read from the list of a constant cell", polymer=b"beads are",
            raw=_raw, detach=lambda h: _raw(h, every=0), read=lambda h: A.lib().sgpr_md_adf_read(h, None, None, None),
            py=lambda mdl: mdl.md_adf(1, 36, CUT), invalid=_invalid, limits=_limits,
            port=29960, ports=30, run=_run, twin=lambda fr, adf, xs: _twin(fr, adf, xs).table(), same=_same)


def test_one_call_and_a_cut_run_equal_the_twin():
    fr = _frame()
    tab, xs, rows, _ = _run(fr, ADF)
    want = _twin(fr, ADF, xs).table()
    assert want["samples"] == 24 and want["cut"][1, 1] == 0.0 and len(set(want["cut"][np.triu_indices(3)])) == 6
    S = 3
    for a in range(S):   # (every triple that can bond has angles; P never sees P)
        for b in range(S):
            for c in range(S):
                assert (want["angles"][a, b, c].sum() > 0) == (want["cut"][a, b] > 0 and want["cut"][a, c] > 0), (a, b, c)
    assert want["coord"][1, 1, 0] == 24 * want["n"][1]
    _same(tab, want, "one call")
    assert np.array_equal(tab["angles"], tab["angles"].transpose(0, 2, 1, 3))
    tab2, xs2, rows2, _ = _run(fr, ADF, cuts=(7, 1, 12, 4))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _same(tab2, want, "cut 7 + 1 + 12 + 4")


@pytest.mark.parametrize("variant", ["every3", "held", "nose-hoover"])
def test_variants_equal_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    adf = (3, 36, CUT) if variant == "every3" else ADF
    kw = dict(fixed=mask(len(fr[0]))) if variant == "held" else {}
    tab, xs, _, _ = _run(fr, adf, cuts=(20,), nh=(variant == "nose-hoover"), **kw)
    want = _twin(fr, adf, xs).table()
    if variant == "every3":
        assert want["samples"] == 7 and want["next_due"] == 21
    if variant == "held":
        assert np.array_equal(xs[-1][kw["fixed"]], fr[1][kw["fixed"]])
    _same(tab, want, variant)


def test_the_thin_cell_atoms_under_several_images():
    """The 256 atoms of lips((8, 8, 4)), L_z = 10.88, all cutoffs 5.9: a neighbour 5.44 away along z stands under two images (+z
    and -z), both in the list and both neighbours."""
    fr = _frame("thin")
    adf = (1, 36, 5.9)
    tab, xs, _, _ = _run(fr, adf, cuts=(2, 2))
    tw = _twin(fr, adf, xs)
    assert list(tw.R) == [0, 0, 1] and len(fr[0]) == 256
    twice = 0
    for i in range(0, 256, 16):   # (an atom under two images among a centre's neighbours: found by its distance vectors)
        d, r, b = tw.neighbours(np.asarray(xs[0]), i)
        dz = np.abs(d[:, None, :] - d[None, :, :])
        twice += int(np.sum(np.all(np.abs(dz - np.abs(tw.h[2])[None, None, :]) < 1e-9, axis=2)))
    assert twice > 0
    _same(tab, tw.table(), "thin cell")


@pytest.mark.parametrize("kind,cut", [("sub200", CUT), ("chunks", CUT), ("sub200", 2.5), ("chunks", 2.5)])
def test_segments_off_a_chunk_over_many_chunks_and_lonely_centres(kind, cut):
    """Species whose counts are no multiple of the chunk of 16 centres (and fewer than one wave's worth), and one over dozens of
    chunks; with a cutoff of 2.5 most centres have no neighbour or one: no pair, coordination 0 and 1 filled."""
    fr = _frame(kind)
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert np.all(n % 16 != 0) and n.min() < 64
    else:
        assert n.max() > 256 and np.any(n % 16 != 0)
    adf = (1, 36, cut)
    tab, xs, _, _ = _run(fr, adf, cuts=(2, 3))
    want = _twin(fr, adf, xs).table()
    assert np.array_equal(want["n"], n)
    if cut == 2.5:
        assert np.all(want["coord"][:, :, 0] > 0) and want["coord"][:, :, 1].sum() > 0
    else:
        assert want["angles"].sum() > 0
    _same(tab, want, f"{kind} {cut}")


@pytest.mark.parametrize("kind", [None, "dense"])
def test_all_cutoffs_at_the_models_cutoff(kind):
    """Every list entry is selected; a centre's ~1000 pairs take many passes of its wave.  No helper frame reaches 64 neighbours
    within rc = 6 (the module's, the densest, has 45 on average), so "dense" — the same frame compressed to 0.85 — supplies them:
    the gather takes two passes of 64 list entries and the rows hold more than 64 neighbours.  The coordination per SPECIES stays
    below the clamp at 63 even there (half the atoms are S: about 36 of them around a centre; the clamp is the twin's CPU test's
    business).  The list outgrows the capacity the module's model has from the sparser frames: the run halts with the loop's ordinary
    overflow code and the call is repeated (_run) — the configuration evaluated again counts once."""
    fr = _frame(kind)
    adf = (1, 30, RC)
    tab, xs, _, _ = _run(fr, adf, cuts=(1, 2))
    want = _twin(fr, adf, xs).table()
    total = want["coord"].sum(axis=(0, 1))   # (per-species counts; the neighbours of a centre are their sum over the species)
    print(f"frame {kind}: per-species coordination up to {int(np.flatnonzero(total).max())}, clamped {int(want['coord'][:, :, 63].sum())}")
    if kind == "dense":
        from autoforce_amd.workloads import AdfCounts
        one = AdfCounts(1, 30, RC, fr[0], _shared()[0].species, fr[2], fr[3])
        nn = np.array([len(one.neighbours(np.asarray(xs[0]), i)[1]) for i in range(0, len(fr[0]), 8)])
        assert nn.min() > 64, nn.min()
    _same(tab, want, f"all cutoffs at rc, frame {kind}")


@pytest.mark.parametrize("bins", [36, 700])
def test_an_angle_exactly_on_an_edge_belongs_to_the_bin_above(bins):
    """Configuration 0 of a run is the caller's: a simple-cubic lattice of 64 S atoms, 2.5 A apart in a cell of 10 A (every
    coordinate and shift exact), cutoff 3 — six neighbours, twelve angles with q == 0 and three with q == -p per centre.  The
    library is handed edges whose middle one is exactly 0 (numpy's cos(pi / 2) is 6e-17): q == ct[e] p holds with equality and
    only `<=` puts the right angles into bin bins / 2, in both counter forms; the twin compares with the same doubles."""
    from autoforce_amd import _lib
    from autoforce_amd.workloads import MASS, AdfCounts, adf_edges
    mdl, lib = _shared()[0], _lib.load()
    S = len(mdl.species)
    pos = np.array([[2.5 * i, 2.5 * j, 2.5 * k] for i in range(4) for j in range(4) for k in range(4)], float) + 0.25
    numbers, cell = np.full(64, 16), np.diag([10.0, 10.0, 10.0])
    pbc = np.ones(3, dtype=bool)
    fr = (numbers, pos, cell, pbc, np.full(64, MASS[16]), np.zeros((64, 3)))
    ct = adf_edges(bins)
    ct[bins // 2] = 0.0
    cut = np.full((S, S), 3.0)
    _begin(mdl, fr, seed=3)
    mdl.md_record(1, velocities=False, results=False)
    assert lib.sgpr_md_adf(mdl.handle, 1, bins, _lib.ptr(cut), _lib.ptr(ct)) == 0
    for _ in range(3):   # (the small cell may outgrow a capacity of the module's model: the overflow halt, the call repeated)
        sc, code = mdl.md_run(1, None)
        assert code in (0, 2)
        if code == 0:
            break
    assert code == 0 and len(sc) == 1 and np.array_equal(mdl.md_frames()["positions"][0], pos)
    angles, coord, info = np.zeros((S, S, S, bins), dtype=np.uint64), np.zeros((S, S, 64), dtype=np.uint64), np.zeros(4 + S, dtype=np.int64)
    assert lib.sgpr_md_adf_read(mdl.handle, _lib.ptr(angles), _lib.ptr(coord), _lib.ptr(info)) == 0
    tw = AdfCounts(1, bins, cut, numbers, mdl.species, cell, pbc, ct=ct)
    tw.add(pos)
    want = tw.table()
    z = list(mdl.species).index(16)
    print(f"bins {bins}: device {[(int(k), int(v)) for k, v in enumerate(angles[z, z, z]) if v]} twin {[(int(k), int(v)) for k, v in enumerate(want['angles'][z, z, z]) if v]}")
    assert want["angles"][z, z, z, bins // 2] == 12 * 64 and want["angles"][z, z, z, bins - 1] == 3 * 64 and want["angles"].sum() == 15 * 64
    assert np.array_equal(angles, want["angles"]) and np.array_equal(coord, want["coord"])
    assert list(info[:4]) == [1, 1, bins, S] and coord[z, z, 6] == 64
    mdl.md_end()


@pytest.mark.parametrize("bins", [7, 180, 700])
def test_both_counter_forms(bins):
    """Six species pairs: 7 and 180 bins keep the counters in LDS (42 and 1080 of them); 700 bins (4200 > 4096) take the form with
    global atomics.  The same frame and run, each equal to the twin."""
    fr = _frame()
    adf = (1, bins, CUT)
    tab, xs, _, _ = _run(fr, adf, cuts=(3,))
    _same(tab, _twin(fr, adf, xs).table(), f"{bins} bins")


def test_a_covloss_halt_counts_every_configuration_once():
    def halted(mid, k, xs):
        assert mid["samples"] == k + 1
        _same(mid, _twin(_frame(), ADF, xs[:k + 1]).table(), f"behind the halt at {k}")
    A.halt_counts_once(ACC, ADF, halted)


@pytest.mark.parametrize("nh", [False, True])
def test_the_accumulator_moves_nothing(nh):
    A.moves_nothing(ACC, nh, (2, 36, CUT), lambda tab: tab["samples"] == 10, record=True)


def test_beside_the_other_accumulators_each_table_equals_the_one_taken_alone():
    fr = _frame()
    adf, others = (3, 36, CUT), dict(msd=(2, 3, True), rdf=(4, 6.0, 60, 0.0), vanhove=(2, 3, 3.0, 30, 2, 2, 6.0, 20))
    kw = dict(cuts=(9, 11), record=False, seed=5, overflow=True)
    o, _, rows, _ = A.run(fr, *A.attached(**others, adf=adf), **kw)
    alone, _, rows_a, _ = _run(fr, adf, cuts=(9, 11), record=False, seed=5)
    oa, _, rows_o, _ = A.run(fr, *A.attached(**others), **kw)
    both = o["adf"]
    assert np.array_equal(rows, rows_a) and np.array_equal(rows, rows_o)
    assert both["samples"] == 7 and both["next_due"] == 21 and o["msd"]["next_due"] == 20 and o["rdf"]["next_due"] == 20 and o["rdf"]["samples"] == 5
    _same(both, alone, "beside md_msd, md_rdf and md_vanhove")
    for k in ("count", "msd", "msd_sq", "smd", "smd_sq"):
        assert np.array_equal(o["msd"][k], oa["msd"][k]), k
    assert np.array_equal(o["rdf"]["hist"], oa["rdf"]["hist"])
    for k in ("self", "over", "distinct", "count"):
        assert np.array_equal(o["vanhove"][k], oa["vanhove"][k]), k
    # (and the others alone are what test_hip_vanhove_device.py compares with their twins: together == alone closes the chain)


def test_a_later_run_starts_from_zeros_and_the_memory_owes_it_nothing():
    """accumulator_device.later_run_and_memory; a second attach on the same handle zeroes the tables; md_adf_table refuses the
    plain run; a detach gives the tables back at once, md_end and close() every byte."""
    from test_hip_teardown import _live

    def accumulate(mdl, fr):
        def attach_and_run():
            _begin(mdl, fr, seed=7)
            mdl.md_adf(*ADF)
            t0 = mdl.md_adf_table()
            assert not t0["angles"].any() and not t0["coord"].any() and t0["samples"] == 0
            sc, code = mdl.md_run(6, None)
            assert code == 0
            return mdl.md_adf_table()
        t1 = attach_and_run()
        t2 = attach_and_run()
        assert t1["samples"] == 6 and t1["angles"].sum() > 0
        _same(t2, t1, "the second attach")

    def detach(mdl, fr, first):
        mdl.md_end()                      # (the tables go with the run)
        _begin(mdl, fr, seed=7)
        held = _live()
        mdl.md_adf(*ADF)                  # 192 / 64 / 256 atoms: 12 + 4 + 16 chunks of 16 centres
        assert np.array_equal(_live() - held, [8 * 27 * 36 + 8 * 9 * 64 + 8 * (9 + 36) + 8 * 2 + 4 * (32 * 3 + 3), 5])
        mdl.md_adf(0)                     # (a detach frees them)
        assert np.array_equal(_live() - held, [0, 0])
        with pytest.raises(RuntimeError, match="no accumulator"):
            mdl.md_adf_table()
        mdl.md_adf(*ADF)
    A.later_run_and_memory(ACC, accumulate, detach)


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    A.two_rank_refusal(ACC, cut=np.full((3, 3), 3.0))


def test_run_md_fills_equal_tables_on_the_device_and_through_the_host_loop(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(adf=holder), the host loop's AdfCounts fed every step's positions:
    the same integers."""
    from autoforce_amd.transport import Adf, angle_distribution, coordination
    tabs, holder, numbers = A.run_md_host_and_device(tmp_path, "adf", lambda cell: Adf(2, 45, 3.6))
    print(f"samples {tabs[0]['samples']}, angles host {int(tabs[0]['angles'].sum())} device {int(tabs[1]['angles'].sum())}")
    assert tabs[0]["samples"] == 21 and tabs[0]["angles"].sum() > 0
    _same(tabs[1], tabs[0], "run_md")
    a, b, c = np.unravel_index(np.argmax(holder.angles.sum(axis=3)), holder.angles.shape[:3])
    zs = [int(z) for z in holder.species]
    th, P = angle_distribution(holder, zs[a], (zs[b], zs[c]))
    n, Pn, mean = coordination(holder, zs[a], zs[b])
    assert np.all(np.isfinite(P)) and abs(P.sum() * 180.0 / 45 - 1.0) < 1e-12 and mean > 0.0
