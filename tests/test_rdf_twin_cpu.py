"""workloads.RdfCounts — the host twin and the definition of the pair-distance accumulator of the device loop (md_rdf.inc) — and
transport.radial_distribution against the reference's own rdf (theforce/analysis/rdf.py, recorded in tests/golden/g19_rdf.npz by
tests/golden/gen/make_rdf.py: two-frame trajectories of four golden frames at rmax 4 and 9, the latter beyond half of every cell
height, so periodic images, self-images and — si32, L_z = 5.43 — a block of two images occur).  The histograms are integers and
must be equal; r and g restate the reference's operations and may differ in the last bits (1e-13 relative).  Then the properties
the definition promises: the table does not depend on the order of a species' atoms nor on how an atom is wrapped, the true
shells integrate to the pair count, an open direction has no images, an absent species keeps zeros and a lone atom sees only
its own images."""
import functools
import os

import numpy as np
import pytest

from autoforce_amd.transport import Rdf, radial_distribution
from autoforce_amd.workloads import RdfCounts, rdf_geometry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "g19_rdf.npz"))


def _names():
    return [str(n) for n in np.load(os.path.join(GOLDEN, "g19_rdf.npz"))["names"]]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(golden arrays of the case, frame, the twin fed its two configurations)."""
    g = _golden()
    c = {k: g[f"{name}_{k}"] for k in ("frame", "rmax", "rmin", "bins", "positions", "r", "pairs", "g", "hist", "gap")}
    f = np.load(os.path.join(GOLDEN, str(c["frame"]) + ".npz"))
    fr = (f["numbers"], f["cell"].reshape(3, 3), np.asarray(f["pbc"], bool), [int(z) for z in f["species"]])
    tw = RdfCounts(1, float(c["rmax"]), int(c["bins"]), float(c["rmin"]), fr[0], fr[3], fr[1], fr[2])
    for x in c["positions"]:
        tw.add(x)
    return c, fr, tw


@pytest.mark.parametrize("name", _names())
def test_twin_reproduces_the_reference_histograms_exactly(name):
    c, fr, tw = _case(name)
    assert float(c["gap"]) >= 1e-9
    tab = tw.table()
    assert tab["samples"] == 2 and tab["next_due"] == 2
    for (za, zb), want in zip(c["pairs"], c["hist"]):
        a, b = fr[3].index(int(za)), fr[3].index(int(zb))
        print(name, (int(za), int(zb)), "counts", int(want.sum()), "twin", int(tab["hist"][a, b].sum()))
        assert np.array_equal(tab["hist"][a, b].astype(np.int64), want), (name, za, zb)
        assert np.array_equal(tab["hist"][b, a], tab["hist"][a, b])
    if name == "si32_r9":
        assert list(tw.R) == [1, 1, 2]
    if name in ("mixed64_r4", "slab18_nearz_r4"):   # (the single-image case: rmax below half of every periodic height)
        assert not tw.R.any()


@pytest.mark.parametrize("name", _names())
def test_radial_distribution_reproduces_the_reference(name):
    c, fr, tw = _case(name)
    r, g = radial_distribution(Rdf(1, float(c["rmax"]), int(c["bins"]), float(c["rmin"])).add(tw.table()))
    assert [list(p) for p in g] == [[int(a), int(b)] for a, b in c["pairs"]]          # the reference's pairs, in its order
    assert np.abs(r / c["r"] - 1.0).max() <= 1e-13
    for p, pair in enumerate(g):
        want = c["g"][p]
        assert np.all(np.isfinite(want)) and np.array_equal(g[pair] == 0.0, want == 0.0)
        nz = want != 0.0
        err = np.abs(g[pair][nz] / want[nz] - 1.0).max() if nz.any() else 0.0
        print(name, pair, "largest relative deviation of g", err)
        assert err <= 1e-13, (name, pair, err)


def test_table_is_invariant_under_order_within_a_species_and_under_wrapping():
    c, fr, tw = _case("tric24_r9")
    numbers, cell, pbc, species = fr
    rng = np.random.default_rng(5)
    perm = np.concatenate([rng.permutation(np.flatnonzero(numbers == z)) for z in species])
    perm = perm[rng.permutation(len(perm))]                                           # (and the species interleaved anew)
    shift = rng.integers(-3, 4, size=(len(numbers), 3))
    assert shift.any(axis=1).sum() > len(numbers) // 2
    other = RdfCounts(1, float(c["rmax"]), int(c["bins"]), float(c["rmin"]), numbers[perm], species, cell, pbc)
    for x in c["positions"]:
        other.add((x + shift @ cell)[perm])
    assert np.array_equal(other.table()["hist"], tw.table()["hist"])


@pytest.mark.parametrize("name", ["mixed64_r9", "slab18_nearz_r9", "mixed64_r6_rmin"])
def test_true_shells_integrate_to_the_pair_count(name):
    c, fr, tw = _case(name)
    tab = tw.table()
    holder = Rdf(1, float(c["rmax"]), int(c["bins"]), float(c["rmin"])).add(tab)
    r, g = radial_distribution(holder, shells=True)
    w = (holder.rmax - holder.rmin) / holder.bins
    assert np.allclose(r, holder.rmin + (np.arange(holder.bins) + 0.5) * w, rtol=1e-15)
    edges = holder.rmin + w * np.arange(holder.bins + 1)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    for (za, zb), gab in g.items():
        a, b = fr[3].index(za), fr[3].index(zb)
        total = float(tab["hist"][a, b].sum()) / (tab["samples"] * tab["n"][a])
        got = float(np.sum(gab * shell * (tab["n"][b] / tab["volume"])))
        assert abs(got / total - 1.0) <= 1e-13, (name, za, zb, got, total)


def test_an_open_direction_has_no_images():
    """Two atoms 1 apart along an open z in a 3 x 3 cell: at rmax = 7 the periodic directions contribute their images (R = 2),
    z none — against a direct enumeration."""
    cell, pbc = np.diag([3.0, 3.0, 2.0]), np.array([True, True, False])
    x = np.array([[0.1, 0.2, 0.0], [0.1, 0.2, 1.0]])
    tw = RdfCounts(1, 7.0, 14, 0.0, [3, 3], [3], cell, pbc)
    assert list(tw.R) == [2, 2, 0]
    tw.add(x)
    want = np.zeros(14, dtype=np.int64)
    for s0 in range(-4, 5):
        for s1 in range(-4, 5):
            for dz in (0.0, 1.0, -1.0):
                r = np.sqrt((3.0 * s0) ** 2 + (3.0 * s1) ** 2 + dz * dz)
                if 0.0 < r < 7.0:
                    want[int(r / 7.0 * 14)] += 1 if dz else 2                           # (dz = 0: the self-images of both atoms)
    assert np.array_equal(tw.table()["hist"][0, 0].astype(np.int64), want)
    assert tw.table()["volume"] == 18.0


def test_an_absent_species_keeps_zeros_and_a_lone_atom_sees_only_its_images():
    c, fr, tw = _case("si32_r9")
    numbers, cell, pbc, _ = fr
    x = c["positions"][0]
    tab = RdfCounts(1, 9.0, 32, 0.0, numbers, [8, 14, 40], cell, pbc)
    tab.add(x)
    t = tab.table()
    one = RdfCounts(1, 9.0, 32, 0.0, numbers, [14], cell, pbc)
    one.add(x)
    assert list(t["n"]) == [0, 32, 0] and np.array_equal(t["hist"][1, 1], one.table()["hist"][0, 0])
    assert not t["hist"][0].any() and not t["hist"][2].any() and not t["hist"][:, 0].any() and not t["hist"][:, 2].any()
    r, g = radial_distribution(Rdf(1, 9.0, 32).add(t))
    assert list(g) == [(14, 14)]
    # one atom of another species among them: (a, a) holds its own images only — the lattice sums of the cell
    nb = numbers.copy()
    nb[7] = 8
    lone = RdfCounts(1, 9.0, 32, 0.0, nb, [8, 14], cell, pbc)
    lone.add(x)
    want = np.zeros(32, dtype=np.int64)
    for s in np.ndindex(9, 9, 9):
        v = (np.array(s) - 4) @ cell
        r = float(np.sqrt(v @ v))
        if 0.0 < r < 9.0:
            want[int(r / 9.0 * 32)] += 1
    h = lone.table()["hist"]
    assert want.sum() > 0 and np.array_equal(h[0, 0].astype(np.int64), want)
    assert h[0, 1].sum() + h[1, 1].sum() + h[1, 0].sum() + h[0, 0].sum() == one.table()["hist"].sum()


def test_settings_out_of_range_are_refused():
    cell, pbc = np.diag([3.0, 3.0, 3.0]), True
    with pytest.raises(NotImplementedError, match="cell height 3"):
        RdfCounts(1, 8.0, 10, 0.0, [3], [3], cell, pbc)                                  # R = 3
    for every, rmax, bins, rmin in ((0, 4.0, 10, 0.0), (1, 4.0, 0, 0.0), (1, 4.0, 2049, 0.0), (1, 4.0, 10, 4.0), (1, 4.0, 10, -1.0)):
        with pytest.raises(ValueError):
            RdfCounts(every, rmax, bins, rmin, [3], [3], cell, pbc)
    with pytest.raises(ValueError, match="no volume"):
        rdf_geometry(np.diag([3.0, 3.0, 0.0]), [True, True, False], 4.0)
    holder = Rdf(1, 4.0, 10)
    with pytest.raises(ValueError, match="no samples"):
        radial_distribution(holder)
    tw = RdfCounts(1, 4.0, 12, 0.0, [3], [3], cell, pbc)
    with pytest.raises(ValueError, match="other settings"):
        holder.add(tw.table())
