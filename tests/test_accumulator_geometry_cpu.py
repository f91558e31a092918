"""The host twins of the in-loop accumulators that do cell geometry of their own — workloads.RdfCounts, VanHoveCounts, AdfCounts,
SqRing (and MsdBlocks, which must not notice the cell) — against the independent references of accumulator_refs.py on the frames
of lattices.py: sheared, rotated and left-handed cells, atoms up to four cells outside, all eight periodicity patterns, one crystal
in five descriptions, a walk with an atom carried through a face, a cell thinner than the cut-off.  No GPU.  The comparison rule is
accumulator_refs.mismatch's: the near counts first (at most 1e-4 of the entries; printed, 0 on these inputs), then equality in
every bin without a near entry."""
import functools

import numpy as np
import pytest

import accumulator_refs as R
import lattices as L
from autoforce_amd import workloads as W

SPECIES = L.SPECIES
BINS, RMIN = 37, 0.3
FACTORS = (0.45, 0.9, 1.6)      # rmax over the smallest periodic height: R = 0, 1, 2 along that axis
ADF_CUT = {(3, 3): 2.6, (3, 16): L.RC, (16, 16): 2.8}
ADF_BINS = 36
HKL = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 2, 0), (0, 1, -3), (-5, 0, 7), (8, 0, 0), (0, -8, 0), (0, 0, 8), (-8, 8, -8),
                (7, -3, 5), (1, 1, 1), (-2, -3, -4), (3, 0, -1)])


def heights(cell):
    """1 / |column k of inv(cell)|: the distance between the cell's faces along direction k, by np.linalg.inv."""
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(cell, float).reshape(3, 3)), axis=0)


def smallest_periodic_height(frame):
    """(axis, height) of the smallest height along a periodic direction (over all three in a cell without one)."""
    h = heights(frame[2])
    k = min((k for k in range(3) if frame[3][k] or not any(frame[3])), key=lambda k: h[k])
    return k, float(h[k])


def rdf_against_reference(frame, rmax, label, pairs=None):
    """(message or None, twin, near entries) of RdfCounts against the all-images reference on one frame."""
    numbers, pos, cell, pbc = frame
    tw = W.RdfCounts(1, rmax, BINS, RMIN, numbers, SPECIES, cell, pbc)
    tw.add(pos)
    H, near = R.rdf(frame, SPECIES, RMIN, rmax, BINS, pairs)
    assert H.sum() > 0, label
    return R.mismatch(tw.table()["hist"], H, near, f"{L.describe(label, frame)} rmax {rmax:.3f}"), tw, int(near.sum())


RDF_FRAMES = [(name, variant, (True, True, True), None) for name in sorted(L.FAMILIES) for variant in L.VARIANTS] + \
             [("triclinic", variant, pbc, L.PBC_ATOMS) for variant in ("given", "left") for pbc in L.PBCS]


@pytest.mark.parametrize("name,variant,pbc,natoms", RDF_FRAMES, ids=lambda v: "".join("FT"[int(x)] for x in v) if isinstance(v, tuple) else str(v))
def test_rdf_twin_equals_the_all_images_reference(name, variant, pbc, natoms):
    frame = L.family(name, variant, pbc=pbc, natoms=natoms)
    axis, h = smallest_periodic_height(frame)
    assert np.abs(frame[1] @ np.linalg.inv(frame[2])).max() > 3.0          # (atoms up to four cells outside)
    nears, pairs = [], R.pair_distances(frame, max(FACTORS) * h)
    for want_R, f in enumerate(FACTORS):
        msg, tw, near = rdf_against_reference(frame, f * h, f"{name} {variant}", pairs)
        nears.append(near)
        assert tw.R[axis] == (want_R if frame[3][axis] else 0), (tw.R, axis, f)
        assert all(tw.R[k] == 0 for k in range(3) if not frame[3][k])
        assert msg is None, msg
    print(f"{name} {variant} pbc {frame[3]}: near entries {nears}")
    if any(frame[3]):
        with pytest.raises(NotImplementedError, match="at most 2"):
            W.RdfCounts(1, 2.6 * h, BINS, RMIN, frame[0], SPECIES, frame[2], frame[3])
    else:
        assert not W.RdfCounts(1, 2.6 * h, BINS, RMIN, frame[0], SPECIES, frame[2], frame[3]).R.any()


def test_a_transposed_inverse_is_seen_on_every_sheared_family_and_not_on_lips(monkeypatch):
    """The mutation the tests on diagonal cells cannot see: rdf_geometry returning the transposed inverse.  The comparison fails on
    every family of lattices.py (none is orthogonal) and still passes on a LiPS frame."""
    true = W.rdf_geometry

    def transposed(cell, pbc, rmax):
        inv, V, hgt, Rk = true(cell, pbc, rmax)
        return inv.T.copy(), V, hgt, Rk
    numbers, pos, cell, pbc = W.lips(5)
    lips = (numbers, pos, cell, tuple(bool(p) for p in pbc))
    species = [3, 15, 16]

    def lips_check():
        tw = W.RdfCounts(1, 0.9 * 13.6, BINS, RMIN, numbers, species, cell, pbc)
        tw.add(pos)
        H, near = R.rdf(lips, species, RMIN, 0.9 * 13.6, BINS)
        return R.mismatch(tw.table()["hist"], H, near, "lips")
    assert lips_check() is None
    monkeypatch.setattr(W, "rdf_geometry", transposed)
    assert lips_check() is None
    for name in sorted(L.FAMILIES):
        frame = L.family(name)
        msg, _, _ = rdf_against_reference(frame, 0.9 * smallest_periodic_height(frame)[1], name)
        assert msg is not None and "bins differ" in msg, name
    monkeypatch.setattr(W, "rdf_geometry", true)
    frame = L.family("triclinic")
    assert rdf_against_reference(frame, 0.9 * smallest_periodic_height(frame)[1], "triclinic")[0] is None


# ------------------------------------------------------------------------------------------------------------------ the walk
VH = dict(every=1, levels=2, rmax=0.2, rbins=10, tbins=4, pbins=6, dbins=23, dmax=(5.0, 8.0))


@functools.lru_cache(maxsize=None)
def _walk():
    frame, frames = L.walk_frames()
    return frame, frames[3:]       # nine configurations; the carried atom goes through its face at the fifth


def test_the_walk_is_what_it_claims():
    frame, frames = _walk()
    assert np.linalg.det(frame[2]) < 0 and len(frames) == 9
    jump = frames[L.WALK["carry_step"] - 3][L.WALK["carried"]] - frames[L.WALK["carry_step"] - 4][L.WALK["carried"]]
    assert np.linalg.norm(jump - frame[2][1]) < 2 * L.WALK["sigma"]
    h = heights(frame[2]).min()
    assert int(np.floor(VH["dmax"][0] / h + 0.5)) == 0 and int(np.floor(VH["dmax"][1] / h + 0.5)) == 1


def test_vanhove_twin_self_and_distinct_on_the_walk():
    (numbers, _, cell, pbc), frames = _walk()
    want_d = R.vanhove_distinct(frames, numbers, cell, pbc, SPECIES, VH["every"], VH["levels"], VH["dmax"], VH["dbins"])
    Hs, over, near, near_over, count = R.vanhove_self(frames, numbers, SPECIES, VH["every"], VH["levels"], VH["rmax"], VH["rbins"], VH["tbins"], VH["pbins"])
    for dmax in VH["dmax"]:
        tw = W.VanHoveCounts(VH["every"], VH["levels"], VH["rmax"], VH["rbins"], VH["tbins"], VH["pbins"], dmax, VH["dbins"], numbers, SPECIES, cell, pbc)
        for x in frames:
            tw.add(x)
        tab = tw.table()
        assert list(tw.R) == [int(dmax == VH["dmax"][1])] * 3
        assert np.array_equal(tab["count"], count) and list(count) == [8, 4]
        H, nd = want_d[dmax]
        print(f"van Hove dmax {dmax}: distinct entries {int(H.sum())}, near {int(nd.sum())}; self entries {int(Hs.sum())}, over {int(over.sum())}, near {int(near.sum())}")
        msg = R.mismatch(tab["distinct"], H, nd, f"distinct, dmax {dmax}")
        assert msg is None, msg
        msg = R.mismatch(tab["self"], Hs, near, "self")
        assert msg is None, msg
        assert near_over.sum() == 0 and np.array_equal(tab["over"], over)
    assert over.sum() == 2        # (the carried atom, once per level: a lattice vector is no displacement of rmax)
    assert np.count_nonzero(Hs.sum(axis=(0, 1, 2, 4))) == VH["tbins"] and np.count_nonzero(Hs.sum(axis=(0, 1, 2, 3))) == VH["pbins"]


@pytest.mark.parametrize("com", [False, True])
def test_msd_twin_on_the_walk(com):
    """The bound: a window's sums run over n <= 105 atoms, each term a few roundings: |d msd| <= 64 n 2^-52 mean |d|^2 and, the
    collective sum squared, |d smd| <= 64 n^2 2^-52 mean |d|^2 per window, with mean |d|^2 the largest raw value of the run (the
    carried atom's 17 A are in it); the sums of squares by d(a^2) = 2 a da."""
    (numbers, _, cell, pbc), frames = _walk()
    mass = np.array([W.MASS[int(z)] for z in numbers])
    tw = W.MsdBlocks(1, 3, com, mass, numbers, SPECIES)
    for x in frames:
        tw.add(x)
    tab, want = tw.table(), R.msd(frames, numbers, SPECIES, mass, 1, 3, com)
    _msd_within(tab, want, frames, len(numbers))


def _msd_within(tab, want, frames, n, every=1):
    scale = max(float(((np.asarray(frames[b]) - np.asarray(frames[a])) ** 2).sum(axis=1).mean()) for _, a, b in R.windows(len(frames), every, len(want["count"])))
    assert np.array_equal(tab["count"], want["count"]) and want["count"][0] > 0
    c = want["count"].max()
    tol = dict(msd=64 * n * 2.0 ** -52 * scale * c, smd=64 * n * n * 2.0 ** -52 * scale * c)
    tol["msd_sq"], tol["smd_sq"] = 2 * scale * tol["msd"] + tol["msd"] ** 2, 2 * n * scale * tol["smd"] + tol["smd"] ** 2
    for k, t in tol.items():
        dev = float(np.abs(tab[k] - want[k]).max())
        print(f"msd table {k}: largest deviation {dev:.3e}, bound {t:.3e}")
        assert dev <= t, (k, dev, t)
        assert np.abs(want[k]).max() > 1e3 * t


# ------------------------------------------------------------------------------------------------------------------ five descriptions
@functools.lru_cache(maxsize=None)
def _twins():
    return L.physics_twins()


def _adf_twin(frame, cut=ADF_CUT, bins=ADF_BINS):
    numbers, pos, cell, pbc = frame
    tw = W.AdfCounts(1, bins, cut, numbers, SPECIES, cell, pbc)
    tw.add(pos)
    return tw.table()


def adf_against_reference(frame, label, cut=ADF_CUT, bins=ADF_BINS):
    ctab = W.adf_cutoffs(cut, SPECIES)
    tab, want = _adf_twin(frame, cut, bins), R.adf(frame, SPECIES, ctab, bins)
    print(f"adf {label}: angles {int(want['angles'].sum())}, near {int(want['near'].sum())}, loose {want['loose']}, gaps {want['gap_angle']:.2e} rad {want['gap_r']:.2e} A")
    for k in ("angles", "coord"):
        msg = R.mismatch(tab[k], want[k], want["near"] if k == "angles" else np.zeros_like(want[k]), f"adf {label} {k}", loose=want["loose"])
        assert msg is None, msg
    return tab, want


def test_adf_twin_on_one_crystal_in_five_descriptions():
    tabs = {}
    for label, (frame, _, _) in _twins().items():
        tabs[label], want = adf_against_reference(frame, label)
        assert want["near"].sum() == 0 and want["loose"] == 0 and want["angles"].sum() > 1000
        assert np.array_equal(W.adf_cutoffs(ADF_CUT, SPECIES) <= L.RC, np.ones((2, 2), bool))
    for label, t in tabs.items():
        for k in ("angles", "coord"):
            assert np.array_equal(t[k], tabs["reduced"][k]), (label, k)


def test_the_thin_frame_has_its_height_below_the_cutoff_and_every_atom_sees_itself():
    from oracle import oracle as orc
    frame = numbers, pos, cell, pbc = L.thin_frame()
    h = heights(cell)
    assert 0.8 * L.RC < h.min() < L.RC and h.argmin() == 0 and abs(np.dot(cell[0], cell[1])) > 1.0   # (thin, and sheared)
    ptr, j, off = orc.neighbors(pos, cell, pbc, L.RC)
    for i in range(len(numbers)):
        own = j[ptr[i]:ptr[i + 1]] == i
        assert own.sum() >= 2 and np.all(off[ptr[i]:ptr[i + 1]][own].any(axis=1))
    assert L.gap_to_rc(frame, L.PHYS["dmin"]) > 0 and len(orc.neighbors(pos, cell, pbc, L.PHYS["dmin"])[1]) == 0
    tab, want = adf_against_reference(frame, "thin", cut=L.RC)
    assert want["near"].sum() == 0 and want["loose"] == 0 and tab["coord"][:, :, 0].sum() < len(numbers) * 2


def hkl_of(label, hkl=HKL):
    """The indices that name the same physical q in a description of physics_twins(): the cell U h has hkl U^T."""
    U = {"shear": L.SHEAR, "shear2": L.SHEAR @ L.SHEAR, "left": np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]])}.get(label, np.eye(3, dtype=int))
    return np.asarray(hkl) @ U.T


def sq_bounds(hmax, smax, nz, count):
    """The bound of test_sq_twin_cpu, restated: B_z = 128 hmax (1 + smax) n_z 2^-52, F = count (n_a B_b + n_b B_a + count n_a n_b 2^-52)."""
    n, c = np.asarray(nz, float), np.asarray(count, float)[:, None, None]
    B = 128.0 * hmax * (1.0 + smax) * n * 2.0 ** -52
    return B, c * (n[:, None] * B[None, :] + n[None, :] * B[:, None] + c * n[:, None] * n[None, :] * 2.0 ** -52)


def sq_within(tab, want, B, F, what):
    """f and mean of `tab` within (F, samples B) of `want`; returns the two largest ratios."""
    assert np.array_equal(tab["count"], want["count"]) and tab["samples"] == want["samples"], what
    df, dm = np.abs(tab["f"] - want["f"]).max(axis=1), np.abs(tab["mean"] - want["mean"]).max(axis=0)
    rf, rm = float(np.max(df[F > 0] / F[F > 0])), float(np.max(dm[B > 0] / (want["samples"] * B[B > 0])))
    print(f"sq {what}: max |df| / bound {rf:.3g}, max |dmean| / (samples B) {rm:.3g}")
    assert np.all(df <= F), (what, df, F)
    assert np.all(dm <= want["samples"] * B), (what, dm)
    return rf, rm


def test_sq_twin_on_one_crystal_in_five_descriptions():
    tabs, bounds = {}, {}
    rng = np.random.default_rng(4)
    step = 0.05 * rng.normal(size=_twins()["reduced"][0][1].shape)
    for label, (frame, _, Rot) in _twins().items():
        numbers, pos, cell, pbc = frame
        frames = [pos, pos + (step if Rot is None else step @ Rot)]
        hkl = hkl_of(label)
        q = W.sq_vectors(hkl, cell)
        q0 = W.sq_vectors(HKL, _twins()["reduced"][0][2])
        assert np.allclose(q, q0 if Rot is None else q0 @ Rot, rtol=0, atol=1e-12)
        tw = W.SqRing(1, hkl, 2, 1, numbers, SPECIES, cell, pbc)
        for x in frames:
            tw.add(x)
        tabs[label] = tw.table()
        bounds[label] = sq_bounds(np.abs(hkl).max(), tw.smax, tabs[label]["n"], tabs[label]["count"])
        sq_within(tabs[label], R.sq(frames, hkl, 1, 2, 1, numbers, SPECIES, cell), *bounds[label], f"{label} against the reference")
    for label in tabs:
        B, F = bounds[label][0] + bounds["reduced"][0], bounds[label][1] + bounds["reduced"][1]
        sq_within(tabs[label], tabs["reduced"], B, F, f"{label} against reduced")
    assert np.abs(tabs["reduced"]["f"]).min() > 1e-6
