"""workloads.VanHoveCounts — the host twin and the definition of the van Hove accumulator of the device MD loop (md_vanhove.inc) —
against the reference's own hist_rtp_displacements (tests/golden/g20_vanhove.npz, made by tests/golden/gen/make_vanhove.py: the
counts h N windows per level and species, every used (r, theta, phi) at least `gap` >= 1e-9 from an edge), against np.histogramdd
over the reference's edges on random displacements, the conservation identity, the radial marginal, the held atom's bin, the
distinct part of a frozen trajectory against workloads.RdfCounts, the image left out once an atom has crossed more than half a
cell, the level rule, and the readers of autoforce_amd.transport."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_vanhove.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _twin(gold, rmax, rb, tb, pb, dmax=None, dbins=0, every=1, frames=None):
    from autoforce_amd.workloads import VanHoveCounts
    tw = VanHoveCounts(every, int(gold["levels"]), rmax, rb, tb, pb, dmax, dbins, gold["numbers"], gold["species"], gold["cell"], True)
    for x in (gold["positions"] if frames is None else frames):
        tw.add(x)
    return tw.table()


@pytest.mark.parametrize("name", ["rtp", "odd", "radial", "over"])
def test_twin_equals_the_reference_counts(gold, name):
    rb, tb, pb = (int(v) for v in gold[f"{name}_bins"])
    assert float(gold[f"{name}_gap"]) >= 1e-9
    tab = _twin(gold, float(gold[f"{name}_rmax"]), rb, tb, pb)
    want = gold[f"{name}_counts"]
    assert tab["self"].dtype == np.uint64 and tab["self"].shape == want.shape
    assert np.array_equal(tab["self"], want.astype(np.uint64))
    assert want.sum() > 0 and np.array_equal(tab["count"], [16, 8, 4, 2]) and np.array_equal(tab["lags"], [1, 2, 4, 8])
    assert np.array_equal(tab["n"], [17, 9, 14]) and tab["samples"] == 17 and tab["next_due"] == 17
    # conservation: every atom of every window is in a bin or beyond rmax
    assert np.array_equal(tab["self"].sum(axis=(2, 3, 4)) + tab["over"], tab["n"][None, :].astype(np.uint64) * tab["count"][:, None].astype(np.uint64))
    assert (tab["over"].sum() > 0) == (name == "over")


@pytest.mark.parametrize("name", ["rtp", "odd", "over"])
def test_angles_summed_are_the_radial_run(gold, name):
    rb, tb, pb = (int(v) for v in gold[f"{name}_bins"])
    rmax = float(gold[f"{name}_rmax"])
    full, radial = _twin(gold, rmax, rb, tb, pb), _twin(gold, rmax, rb, 1, 1)
    assert np.array_equal(full["self"].sum(axis=(3, 4)), radial["self"][:, :, :, 0, 0]) and np.array_equal(full["over"], radial["over"])


@pytest.mark.parametrize("name", ["rtp", "odd", "radial"])
def test_held_atom_lands_where_atan2_of_zero_does(gold, name):
    from autoforce_amd.workloads import VanHoveCounts
    rb, tb, pb = (int(v) for v in gold[f"{name}_bins"])
    held = int(gold["held"])
    z = int(np.flatnonzero(gold["species"] == gold["numbers"][held])[0])
    tw = VanHoveCounts(1, 4, 6.0, rb, tb, pb, None, 0, gold["numbers"][[held]], gold["species"], gold["cell"], True)
    for x in gold["positions"]:
        tw.add(x[[held]])
    tab = tw.table()
    want = np.zeros_like(tab["self"])
    want[:, z, 0, 0, pb // 2] = tab["count"].astype(np.uint64)
    assert np.array_equal(tab["self"], want) and tab["over"].sum() == 0


@pytest.mark.parametrize("shape", [(16, 6, 8), (99, 29, 59), (10, 1, 1), (12, 5, 7)])
def test_bin_rule_is_histogramdd_over_the_reference_edges(shape):
    """The comparisons of vanhove_self_bins against np.histogramdd over linspace edges with arctan2 angles, as the reference
    forms them (descriptor/sphcart.py cart_coord_to_sph restated): samples nearer than 1e-9 to an edge are left out."""
    from autoforce_amd.workloads import vanhove_edges, vanhove_self_bins
    rb, tb, pb = shape
    rmax = 3.0
    rng = np.random.default_rng(sum(shape))
    d = rng.normal(size=(20000, 3)) * rng.choice([0.05, 1.0, 2.5], size=(20000, 1))
    q = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    rtp = np.stack([np.sqrt(q + d[:, 2] * d[:, 2]), np.arctan2(np.sqrt(q), d[:, 2]), np.arctan2(d[:, 1], d[:, 0])], axis=1)
    edges = [np.linspace(0, rmax, rb + 1), np.linspace(0, np.pi, tb + 1), np.linspace(-np.pi, np.pi, pb + 1)]
    clear = np.all([np.abs(rtp[:, a, None] - edges[a][None, :]).min(axis=1) >= 1e-9 for a in range(3)], axis=0)
    d, rtp = d[clear], rtp[clear]
    assert len(d) > 19900
    inside, kr, kt, kp = vanhove_self_bins(d, rmax, rb, tb, pb, *vanhove_edges(tb, pb))
    got = np.zeros(shape, dtype=np.int64)
    np.add.at(got, (kr[inside], kt[inside], kp[inside]), 1)
    assert np.array_equal(got, np.histogramdd(rtp, bins=edges)[0].astype(np.int64))
    assert np.array_equal(inside, rtp[:, 0] < rmax) and 0 < inside.sum() < len(d)


def _frozen_case():
    g5 = np.load(os.path.join(os.path.dirname(GOLD), "g5_mixed64.npz"))
    return g5["numbers"], g5["positions"], g5["cell"].reshape(3, 3), np.asarray(g5["pbc"], bool), sorted(set(int(z) for z in g5["numbers"]))


@pytest.mark.parametrize("heights", [0.45, 1.2])
def test_frozen_trajectory_is_rdf_counts_per_window(heights):
    from autoforce_amd.workloads import RdfCounts, VanHoveCounts, rdf_geometry
    numbers, x, cell, pbc, species = _frozen_case()
    dmax = heights * float(rdf_geometry(cell, pbc, 1.0)[2].min())
    rdf = RdfCounts(1, dmax, 24, 0.0, numbers, species, cell, pbc)
    rdf.add(x)
    vh = VanHoveCounts(1, 3, 1.0, 4, 1, 1, dmax, 24, numbers, species, cell, pbc)
    assert bool(vh.R.any()) == (heights > 0.5)
    for _ in range(9):
        vh.add(x)
    tab = vh.table()
    assert np.array_equal(tab["count"], [8, 4, 2]) and rdf.hist.sum() > 0
    for l in range(3):
        assert np.array_equal(tab["distinct"][l], rdf.hist * np.uint64(tab["count"][l]))
    assert tab["volume"] == rdf.volume and tab["dmax"] == dmax and tab["dbins"] == 24


@pytest.mark.parametrize("dmax", [4.0, 13.0])
def test_an_atom_that_crossed_half_a_cell_keeps_its_images(dmax):
    """Two atoms in a cubic cell of side 10; atom 0 moves 7 along x between the two samples.  Against its own origin it stands at
    shift 0 (left out) at distance 7, and its images at shifts -1, +1 along x stand at distances 3 and 17: with dmax = 4 (one
    image, the nearest: shift -1) the 3 counts, with dmax = 13 (image block) the 3 counts too, and the 7 never."""
    from autoforce_amd.workloads import VanHoveCounts
    cell = np.diag([10.0] * 3)
    x0 = np.array([[1.0, 1.0, 1.0], [1.0, 6.0, 1.0]])
    x1 = x0 + np.array([[7.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    bins = 26
    vh = VanHoveCounts(1, 1, 20.0, 4, 1, 1, dmax, bins, [3, 3], [3], cell, True)
    vh.add(x0)
    vh.add(x1)
    got = vh.table()["distinct"][0, 0, 0].astype(np.int64)
    # brute force: every (i, j, s) but (i, i, 0)
    want = np.zeros(bins, dtype=np.int64)
    for i in range(2):
        for j in range(2):
            for s in np.ndindex(7, 7, 7):
                s = np.array(s) - 3
                if i == j and not s.any():
                    continue
                r = np.linalg.norm(x1[j] - x0[i] + s @ cell)
                if r < dmax:
                    want[min(int(r / dmax * bins), bins - 1)] += 1
    assert np.array_equal(got, want)
    k3, k7 = int(3.0 / dmax * bins), int(7.0 / dmax * bins)
    own = np.zeros(bins, dtype=np.int64)   # (atom 0 against its own origin alone)
    one = VanHoveCounts(1, 1, 20.0, 4, 1, 1, dmax, bins, [3], [3], cell, True)
    one.add(x0[:1])
    one.add(x1[:1])
    own = one.table()["distinct"][0, 0, 0].astype(np.int64)
    assert own[k3] == 1 and (k7 >= bins or own[k7] == 0)


def test_the_first_species_index_is_the_origin():
    """A Li moves from z = 1 to z = 3 while an S stays at z = 6: from the Li's origin the S stands at 5, from the S's origin the
    Li stands at 3 — distinct[l, Li, S] and distinct[l, S, Li] are different tables."""
    from autoforce_amd.workloads import VanHoveCounts
    vh = VanHoveCounts(1, 1, 5.0, 4, 1, 1, 8.0, 8, [3, 16], [3, 16], np.diag([40.0] * 3), True)
    vh.add(np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 6.0]]))
    vh.add(np.array([[1.0, 1.0, 3.0], [1.0, 1.0, 6.0]]))
    d = vh.table()["distinct"][0].astype(int)
    assert d[0, 1].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and d[1, 0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert d[0, 0].sum() == 0 and d[1, 1].sum() == 0   # (each atom against its own origin: shift 0, left out)


def test_level_rule():
    from autoforce_amd.workloads import VanHoveCounts
    rng = np.random.default_rng(3)
    vh = VanHoveCounts(1, 5, 50.0, 8, 2, 2, None, 0, [3, 16, 3], [3, 15, 16], np.eye(3), False)
    x = rng.normal(size=(3, 3))
    for _ in range(40):
        vh.add(x)
        x = x + 0.1 * rng.normal(size=(3, 3))
    tab = vh.table()
    assert np.array_equal(tab["count"], [39, 19, 9, 4, 2]) and tab["samples"] == 40 and tab["next_due"] == 40
    assert np.array_equal(tab["self"].sum(axis=(2, 3, 4)), np.outer([39, 19, 9, 4, 2], [2, 0, 1]).astype(np.uint64))
    ev = VanHoveCounts(3, 5, 50.0, 8, 2, 2, None, 0, [3, 16, 3], [3, 15, 16], np.eye(3), False)
    for _ in range(40):
        ev.add(x)
    assert np.array_equal(ev.table()["count"], [13, 6, 3, 1, 0]) and ev.table()["next_due"] == 42


def test_origin_is_set_after_measuring_and_per_level(gold):
    """The displacement of level l at sample s is x(s) - x(s - 2^l): restated from the stored trajectory."""
    from autoforce_amd.workloads import vanhove_edges, vanhove_self_bins
    pos, numbers = gold["positions"], gold["numbers"]
    tab = _twin(gold, 6.0, 16, 6, 8)
    want = np.zeros_like(tab["self"])
    for l in range(4):
        for s in range(1 << l, len(pos), 1 << l):
            for z, Z in enumerate(gold["species"]):
                sel = numbers == Z
                inside, kr, kt, kp = vanhove_self_bins(pos[s][sel] - pos[s - (1 << l)][sel], 6.0, 16, 6, 8, *vanhove_edges(6, 8))
                np.add.at(want[l, z], (kr[inside], kt[inside], kp[inside]), np.uint64(1))
    assert np.array_equal(tab["self"], want)


def test_limits():
    from autoforce_amd.workloads import VanHoveCounts
    ok = dict(every=1, levels=2, rmax=1.0, rbins=4, tbins=1, pbins=1, dmax=None, dbins=0, numbers=[3], species=[3], cell=np.eye(3) * 5, pbc=True)
    VanHoveCounts(**ok)
    for bad in (dict(levels=33), dict(levels=0), dict(rbins=2049), dict(tbins=65), dict(pbins=0), dict(every=0), dict(dbins=2049, dmax=1.0),
                dict(dbins=4, dmax=0.0)):
        with pytest.raises(ValueError):
            VanHoveCounts(**{**ok, **bad})
    with pytest.raises(NotImplementedError, match="1 GiB"):
        VanHoveCounts(**{**ok, **dict(levels=32, rbins=2048, tbins=64, pbins=64)})
    with pytest.raises(NotImplementedError, match="height"):
        VanHoveCounts(**{**ok, **dict(dbins=8, dmax=13.0)})
    VanHoveCounts(**{**ok, **dict(dbins=8, dmax=12.4)})


def test_transport_readers(gold):
    from autoforce_amd.transport import VanHove, displacement_histogram, distinct_van_hove, non_gaussian, self_van_hove
    name = "rtp"
    rb, tb, pb = (int(v) for v in gold[f"{name}_bins"])
    rmax = float(gold[f"{name}_rmax"])
    tab = _twin(gold, rmax, rb, tb, pb, dmax=4.0, dbins=10)
    vh = VanHove(1, 4, rmax, rb, tb, pb, 4.0, 10).add(tab)
    with pytest.raises(ValueError):
        VanHove(1, 4, rmax, rb, tb, pb).add(tab)
    for l in range(4):
        for Z, z in ((3, 0), (15, 1), (16, 2)):
            r, t, p, h, rho = displacement_histogram(vh, l, Z)
            assert np.allclose(h, gold[f"{name}_h"][l, z], rtol=1e-13, atol=0.0) and np.isclose(rho, tab["n"][z] / 9.0 ** 3)
            assert np.allclose(r, np.linspace(0, rmax, rb + 1)[:-1] + rmax / rb / 2) and len(t) == tb and len(p) == pb
            assert np.isclose(p[0], -np.pi + np.pi / pb) and np.isclose(t[-1], np.pi - np.pi / tb / 2)
    r, G = self_van_hove(vh)
    for Z in (3, 15, 16):   # (normalised: nothing lies beyond rmax in this case)
        assert np.allclose((G[Z] * 4 * np.pi * r ** 2 * (rmax / rb)).sum(axis=1), 1.0)
    r, Gd = distinct_van_hove(vh)
    assert set(Gd) == {(a, b) for a in (3, 15, 16) for b in (3, 15, 16)} and Gd[(3, 16)].shape == (4, 10)
    assert np.isclose(Gd[(3, 16)][1, 4], tab["distinct"][1, 0, 2, 4] / (8 * 17 * 4 * np.pi * r[4] ** 2 * 0.4 * 14 / 9.0 ** 3))
    twice = VanHove(1, 4, rmax, rb, tb, pb, 4.0, 10).add(tab).add(tab)
    assert np.array_equal(twice.table()["self"], 2 * tab["self"]) and np.array_equal(twice.count, 2 * tab["count"])
    assert np.allclose(self_van_hove(twice)[1][3], G[3])
    # alpha_2 of Gaussian walkers is 0 within the binning and the sampling: 20000 walkers, one level
    from autoforce_amd.workloads import VanHoveCounts
    rng = np.random.default_rng(8)
    tw = VanHoveCounts(1, 1, 6.0, 400, 1, 1, None, 0, [3] * 20000, [3], np.eye(3), False)
    x = np.zeros((20000, 3))
    tw.add(x)
    tw.add(x + rng.normal(size=x.shape))
    a2 = non_gaussian(VanHove(1, 1, 6.0, 400).add(tw.table()))[3]
    # (the standard error of alpha_2 over n Gaussian walkers is about sqrt(8 / (3 n)) ... 0.012 at 20000; the binning adds O((dr / r)^2) ~ 1e-4)
    assert a2.shape == (1,) and abs(a2[0]) < 0.05
