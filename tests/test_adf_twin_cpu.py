"""workloads.AdfCounts — the host twin and the definition of the bond-angle and coordination accumulator of the device loop
(md_adf.inc); the reference has no angular analysis, so the twin is checked against configurations whose answer is known without
it: a simple-cubic lattice (every angle exactly 90 or 180 degrees: q == 0 and q == -p must land in bins / 2 and bins - 1 — with
numpy's edges, and with a middle edge of exactly 0, where q == ct[e] p holds with equality and only `<=` is right), the same lattice one cell thick (the neighbours along z are the atom's own two images), an open chain
with the cutoff beyond twice the spacing (a neighbour and its double: exactly 0 degrees, bin 0), a tetrahedral AB4 cluster, and a
random two-species frame in a small triclinic cell against an independent brute force that uses arccos (no angle within 1e-9 rad
of an edge, no distance within 1e-9 of a cutoff — checked here, so that the two rules cannot differ).  Then the invariants of the
definition, `every`, cutting the stream, table()'s fields, the holder and its readers, and the argument errors."""
import functools

import numpy as np
import pytest

import accumulator_refs
from autoforce_amd.transport import Adf, angle_distribution, coordination
from autoforce_amd.workloads import ADF_MAXCOORD, AdfCounts, adf_cutoffs, adf_edges


def _cubic(nx, ny, nz, a=2.0):
    x = np.array([[a * i, a * j, a * k] for i in range(nx) for j in range(ny) for k in range(nz)], float)
    return x, np.diag([a * nx, a * ny, a * nz])


def _one(every, bins, cut, numbers, species, cell, pbc, *frames):
    tw = AdfCounts(every, bins, cut, numbers, species, cell, pbc)
    for x in frames:
        tw.add(x)
    return tw.table()


@pytest.mark.parametrize("bins", [180, 2, 64])
@pytest.mark.parametrize("shape", [(3, 3, 3), (3, 3, 1), (1, 1, 1)])
def test_cubic_lattice_angles_sit_on_the_edges(shape, bins):
    """Six neighbours and 15 pairs per centre: 12 at exactly 90 degrees (q == 0: bin bins / 2), 3 at exactly 180 (q == -p: the last
    bin).  (3, 3, 1): the neighbours along z are the atom's own images (j == i, s = +-1); (1, 1, 1): all six are."""
    x, cell = _cubic(*shape)
    N = len(x)
    t = _one(1, bins, 2.5, np.full(N, 3), [3], cell, True, x + 0.25)
    want = np.zeros(bins, dtype=np.uint64)
    want[bins // 2] += 12 * N
    want[bins - 1] += 3 * N
    assert np.array_equal(t["angles"][0, 0, 0], want)
    assert t["coord"][0, 0, 6] == N and t["coord"].sum() == N
    assert t["samples"] == 1 and t["next_due"] == 1


@pytest.mark.parametrize("bins", [2, 64, 180])
def test_an_angle_exactly_on_an_edge_belongs_to_the_bin_above(bins):
    """numpy's cos(pi / 2) is 6e-17, not 0, so with adf_edges' doubles the lattice's q == 0 passes edge bins / 2 by `<` already.  The
    library takes the caller's edges: with that one set to exactly 0, q == ct[e] p holds with equality (0 == 0 p) and only `<=`
    puts the right angles into bin bins / 2."""
    x, cell = _cubic(3, 3, 3)
    ct = adf_edges(bins)
    ct[bins // 2] = 0.0
    tw = AdfCounts(1, bins, 2.5, np.full(27, 3), [3], cell, True, ct=ct)
    tw.add(x + 0.25)
    want = np.zeros(bins, dtype=np.uint64)
    want[bins // 2] += 12 * 27
    want[bins - 1] += 3 * 27
    assert np.array_equal(tw.table()["angles"][0, 0, 0], want)


def test_wrapping_an_atom_changes_nothing():
    x, cell = _cubic(3, 3, 1)
    y = x.copy()
    y[4] += 2 * cell[0] - cell[2]
    y[7] -= cell[1]
    a, b = (_one(1, 180, 2.5, np.full(9, 3), [3], cell, True, p) for p in (x, y))
    assert np.array_equal(a["angles"], b["angles"]) and np.array_equal(a["coord"], b["coord"])


def test_open_chain_a_neighbour_and_its_double_are_at_zero_degrees():
    """Five atoms 1.7 apart on an open line, cutoff 2.5 spacings: per centre the neighbours at +-1 and +-2 spacings.  Pairs on one
    side are exactly 0 degrees (q == p: bin 0, `q <= ct[1] p` is false), on two sides exactly 180: 6 and 8 in all."""
    x = np.array([[1.7 * k, 0.3, -0.2] for k in range(5)])
    t = _one(1, 180, 4.25, np.full(5, 3), [3], np.eye(3), False, x)
    want = np.zeros(180, dtype=np.uint64)
    want[0], want[179] = 6, 8
    assert np.array_equal(t["angles"][0, 0, 0], want)
    c = np.zeros(ADF_MAXCOORD, dtype=np.uint64)
    c[2], c[3], c[4] = 2, 2, 1
    assert np.array_equal(t["coord"][0, 0], c)


def test_tetrahedral_cluster():
    """AB4 in an open box: six B-A-B angles in the bin that holds 109.47 degrees, none elsewhere; B centres with one neighbour;
    cut[B][B] = 0 honoured (the B-B distance 2.83 lies within the other cutoffs)."""
    x = 1.0 * np.array([[0, 0, 0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) + 5.0
    numbers, species = np.array([15, 16, 16, 16, 16]), [15, 16]
    t = _one(1, 180, {(15, 16): 3.0, (15, 15): 3.0}, numbers, species, np.eye(3), False, x)
    assert t["cut"][1, 1] == 0.0 and t["cut"][0, 1] == t["cut"][1, 0] == 3.0
    want = np.zeros((2, 2, 2, 180), dtype=np.uint64)
    want[0, 1, 1, 109] = 6
    assert np.array_equal(t["angles"], want)
    assert t["coord"][0, 1, 4] == 1 and t["coord"][0, 0, 0] == 1 and t["coord"][1, 0, 1] == 4 and t["coord"][1, 1, 0] == 4
    assert t["coord"].sum() == 2 * 5
    # with B-B bonds: every B sees the three others and A; (A, B) pairs are stored once and filled out
    t = _one(1, 180, 3.0, numbers, species, np.eye(3), False, x)
    assert t["coord"][1, 1, 3] == 4
    assert t["angles"][1, 1, 1].sum() == 4 * 3 and t["angles"][1, 0, 1].sum() == 4 * 3 and t["angles"][1, 0, 0].sum() == 0
    assert np.array_equal(t["angles"][1, 0, 1], t["angles"][1, 1, 0])
    assert t["angles"][1, 1, 1, 60] == 12   # (the faces of the tetrahedron: 60 degrees up to rounding, the bin above the edge or on it)
    th, P = angle_distribution(t, 15, (16, 16))
    assert abs(th[np.argmax(P)] - 109.5) < 1e-12 and abs(P.sum() * (180.0 / 180) - 1.0) < 1e-12
    n, P, mean = coordination(t, 16, 16)
    assert mean == 3.0 and P[3] == 1.0


SEED = 7


@functools.lru_cache(maxsize=None)
def _random_frame():
    rng = np.random.default_rng(SEED)
    cell = np.array([[5.2, 0.0, 0.0], [0.7, 5.6, 0.0], [-0.4, 0.9, 6.1]])
    N = 36
    x = rng.random((N, 3)) @ cell + rng.integers(-1, 2, (N, 3)) @ cell   # (some atoms a cell away: not wrapped)
    numbers = np.where(rng.random(N) < 0.4, 15, 16)
    cut = {(15, 15): 3.3, (15, 16): 2.9, (16, 16): 2.4}
    return numbers, [15, 16], cell, x, cut


def _brute(bins):
    """Independent of the twin (accumulator_refs.adf: every image from the oracle's all-pairs list, a plain norm, arccos and
    floor): (H, C, the smallest gap between an angle and an edge in rad, the gap of the distances to their cutoffs, sum over
    centres of n_b (n_b - 1) / 2 or n_b n_c)."""
    numbers, species, cell, x, cut = _random_frame()
    t = accumulator_refs.adf((numbers, x, cell, (True, True, True)), species, adf_cutoffs(cut, species), bins)
    S = len(species)
    nsum = np.zeros((S, S, S), dtype=np.int64)
    for a, cnt in zip(accumulator_refs._slots(numbers, species), t["per_centre"]):
        for b in range(S):
            for c in range(S):
                nsum[a, b, c] += cnt[b] * (cnt[b] - 1) // 2 if b == c else cnt[b] * cnt[c]
    return t["angles"], t["coord"], t["gap_angle"], t["gap_r"], nsum


@functools.lru_cache(maxsize=None)
def _random_case(bins):
    numbers, species, cell, x, cut = _random_frame()
    return _one(1, bins, cut, numbers, species, cell, True, x), _brute(bins)


@pytest.mark.parametrize("bins", [36, 180])
def test_random_frame_against_arccos_brute_force(bins):
    t, (H, C, gap_angle, gap_r, _) = _random_case(bins)
    print("bins", bins, "angles", int(H.sum()), "gap to an edge", gap_angle, "rad; gap to a cutoff", gap_r)
    assert gap_angle >= 1e-9 and gap_r >= 1e-9   # (the seed's choice: the two rules cannot differ)
    assert H.sum() > 1000 and np.count_nonzero(H) > bins
    assert np.array_equal(t["angles"].astype(np.int64), H)
    assert np.array_equal(t["coord"].astype(np.int64), C)


def test_invariants_of_the_definition():
    t, (_, _, _, _, nsum) = _random_case(36)
    S = len(t["species"])
    for a in range(S):
        for b in range(S):
            assert t["coord"][a, b].sum() == t["samples"] * t["n"][a]
            n = np.arange(ADF_MAXCOORD)
            assert t["angles"][a, b, b].sum() == np.sum(t["coord"][a, b].astype(np.int64) * (n * (n - 1) // 2))   # (no centre at the clamp)
            for c in range(S):
                assert t["angles"][a, b, c].sum() == nsum[a, b, c]
                assert np.array_equal(t["angles"][a, b, c], t["angles"][a, c, b])
    assert t["coord"][:, :, ADF_MAXCOORD - 1].sum() == 0


def test_coordination_is_clamped():
    """A cutoff of 3.3 lattice constants on the cubic lattice: 146 neighbours, counted in the last entry; all pairs counted."""
    x, cell = _cubic(2, 2, 2)
    t = _one(1, 12, 6.7, np.full(8, 3), [3], cell, True, x)
    n = sum(1 for i in range(-4, 5) for j in range(-4, 5) for k in range(-4, 5) if 0 < 4.0 * (i * i + j * j + k * k) < 6.7 ** 2)
    assert n > ADF_MAXCOORD
    assert t["coord"][0, 0, ADF_MAXCOORD - 1] == 8 and t["coord"].sum() == 8
    assert t["angles"].sum() == 8 * n * (n - 1) // 2


def test_every_and_cutting_the_stream():
    numbers, species, cell, x, cut = _random_frame()
    rng = np.random.default_rng(3)
    frames = [x + 0.05 * k * rng.standard_normal(x.shape) for k in range(7)]
    tw = AdfCounts(3, 24, cut, numbers, species, cell, True)
    for f in frames:
        tw.add(f)
    t = tw.table()
    assert t["samples"] == 3 and t["next_due"] == 9 and t["every"] == 3 and t["bins"] == 24
    assert set(t) == {"angles", "coord", "species", "n", "samples", "next_due", "every", "bins", "cut"}
    assert t["angles"].shape == (2, 2, 2, 24) and t["angles"].dtype == np.uint64
    assert t["coord"].shape == (2, 2, ADF_MAXCOORD) and t["coord"].dtype == np.uint64
    assert list(t["species"]) == species and list(t["n"]) == [int(np.sum(numbers == z)) for z in species]
    assert np.array_equal(t["cut"], adf_cutoffs(cut, species))
    parts = [_one(1, 24, cut, numbers, species, cell, True, frames[k]) for k in (0, 3, 6)]
    assert np.array_equal(t["angles"], sum(p["angles"] for p in parts))
    assert np.array_equal(t["coord"], sum(p["coord"] for p in parts))
    # the holder adds the tables of several runs; one whose stream is cut at a multiple of `every` gives the same
    hold = Adf(3, 24, cut)
    for lo, hi in ((0, 3), (3, 7)):
        tw = AdfCounts(3, 24, cut, numbers, species, cell, True)
        for f in frames[lo:hi]:
            tw.add(f)
        hold.add(tw.table())
    assert hold.samples == 3 and np.array_equal(hold.angles, t["angles"]) and np.array_equal(hold.coord, t["coord"])
    with pytest.raises(ValueError):
        hold.add(_one(1, 12, cut, numbers, species, cell, True, x))
    th, P = angle_distribution(hold, 15, (16, 15), degrees=False)
    assert th.shape == (24,) and abs(P.sum() * np.pi / 24 - 1.0) < 1e-12
    th2, P2 = angle_distribution(hold, 15, (15, 16), degrees=False, solid_angle=True)
    assert np.allclose(P2 * np.sin(th2) / np.sum(P2 * np.sin(th2)), P / P.sum(), rtol=1e-12, atol=0)
    n, Pn, mean = coordination(hold, 16, 15)
    assert abs(Pn.sum() - 1.0) < 1e-12 and abs(mean - np.sum(n * hold.coord[1, 0]) / hold.coord[1, 0].sum()) < 1e-12


def test_edges_and_cutoff_tables():
    ct = adf_edges(180)
    assert ct[0] == 1.0 and ct[90] > 0.0 and ct[91] < 0.0 and np.all(np.diff(ct) < 0.0)   # (cos(pi / 2) rounds above 0: q == 0 passes edge 90)
    assert np.array_equal(adf_cutoffs(2.5, [3, 15, 16]), np.full((3, 3), 2.5))
    c = adf_cutoffs({(16, 15): 2.6, (3, 16): 3.0}, [3, 15, 16])
    assert np.array_equal(c, c.T) and c[1, 2] == 2.6 and c[0, 2] == 3.0 and c[0, 0] == c[0, 1] == c[1, 1] == c[2, 2] == 0.0
    with pytest.raises(ValueError):
        adf_cutoffs({(16, 14): 2.6}, [3, 15, 16])
    with pytest.raises(ValueError):
        adf_cutoffs({(16, 15): 2.6, (15, 16): 2.7}, [3, 15, 16])


def test_argument_errors():
    numbers, species, cell, x, cut = _random_frame()
    ok = dict(every=1, bins=10, cut=cut, numbers=numbers, species=species, cell=cell, pbc=True)
    AdfCounts(**ok)
    for bad in (dict(every=0), dict(bins=0), dict(bins=1025), dict(cut=0.0), dict(cut=-1.0), dict(cut=np.array([[1.0, 2.0], [3.0, 1.0]])),
                dict(cut={(15, 15): 0.0}), dict(numbers=np.where(numbers == 15, 14, numbers))):
        with pytest.raises(ValueError):
            AdfCounts(**{**ok, **bad})
    with pytest.raises(ValueError):
        Adf(1, 10)
    t = _one(1, 10, cut, numbers, species, cell, True, x)
    with pytest.raises(ValueError):
        angle_distribution(t, 14, (15, 16))
    with pytest.raises(ValueError):
        coordination(t, 15, 3)
