"""GPU tests of the GEOMETRY of the accumulators inside the device MD loop — md_rdf_geometry (md_host.inc), the pair sweeps
md_rdf_pair_kernel<IMG> and md_vh_pair_kernel<IMG>, md_sq_part_kernel's scaled coordinates and md_adf_kernel's image codes — on
the frames of lattices.py: the left-handed rhombohedral walk frame (atoms four cells outside, one a lattice vector further), the
left-handed triclinic family under the six periodicity patterns with an open direction, one crystal in five descriptions, and a
sheared cell thinner than the cut-off.  Every other GPU test of the six accumulators runs on a diagonal right-handed LiPS cell.

Every case asserts three things of a table: it equals the host twin (workloads.py) fed the run's own recorded positions (integers
exactly, md_sq within test_hip_sq_device._within's bound); it passes accumulator_refs.mismatch against the independent
all-images reference computed from the same positions (the near counts are asserted and printed first; md_sq within the same
a-priori bound); and a second run gives the same bits.  test_accumulator_geometry_cpu.py holds the twins to the same references
without a GPU."""
import functools

import numpy as np
import pytest

import accumulator_refs as R
import lattices as L
from test_accumulator_geometry_cpu import HKL, heights, hkl_of, smallest_periodic_height, sq_bounds, sq_within

pytestmark = pytest.mark.gpu

SPECIES = L.SPECIES
EVALS = 13
EVERY = 3             # samples at the configurations 0, 3, 6, 9, 12: five all-images enumerations per reference
BINS, RMIN = 300, 0.3  # more than one pass of 256 threads over the table, and not a multiple of it
WORST_SQ = dict(twin=0.0, reference=0.0)


@functools.lru_cache(maxsize=None)
def _model():
    """One model for every frame of this file (two species, rc = 3): twelve environments of the physics frame, small weights."""
    from test_hip_list_geometry import physics_model
    m = L.PHYS["m"]
    mdl = physics_model(L.physics_frame())
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(2 * m, m)), rng.normal(size=2 * m))
    mdl.set_weights(0.02 * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
    return mdl


def _mass(numbers):
    from autoforce_amd.workloads import MASS
    return np.array([MASS[int(z)] for z in numbers])


def _v0(numbers, seed=11):
    from autoforce_amd.ase_shim import kB
    return np.random.default_rng(seed).normal(size=(len(numbers), 3)) * np.sqrt(kB * 600.0 / _mass(numbers)[:, None])


def run(frame, attach, read, evals=EVALS, v0=None, langevin=True):
    """`evals` evaluations of the device loop at 600 K on the frame (Langevin with the device's own deviates, or plain velocity
    Verlet), the positions recorded at every configuration; attach(mdl) attaches the accumulators before the first evaluation,
    read(mdl) reads them after the last.  A call that halts with code 2 (a list capacity outgrown) is repeated.  Returns (what
    read returned, positions [evals, N, 3])."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl = _model()
    numbers, pos, cell, pbc = frame
    v0 = _v0(numbers) if v0 is None else v0
    par = dict(friction=1e-3, kT=kB * 600.0, seed=11) if langevin else {}
    mdl.md_begin(numbers, pos, cell, pbc, _mass(numbers), v0, dt=FS, **par)
    mdl.md_record(1, velocities=False, results=False)
    attach(mdl)
    xs, index, done = [], [], 0
    for _ in range(8):
        sc, code = mdl.md_run(evals - done, None)
        assert code in (0, 2), code
        done += len(sc)
        f = mdl.md_frames()
        xs.append(f["positions"].copy())
        index.extend(int(k) for k in f["index"])
        if done == evals:
            break
    assert done == evals and index == list(range(evals)), (done, index)
    out = read(mdl)
    mdl.md_end()
    return out, np.concatenate(xs)


@functools.lru_cache(maxsize=None)
def _walk_start():
    """The walk frame with the positions of the walk's last step: atoms up to four cells outside, the carried atom one lattice
    vector further through its face; left-handed, sheared."""
    (numbers, _, cell, pbc), frames = L.walk_frames()
    assert np.linalg.det(cell) < 0 and np.abs(frames[-1] @ np.linalg.inv(cell)).max() > 4.0
    return numbers, frames[-1], cell, pbc


PAIRS = {}


def _pairs(key, frame, xs, rmax):
    """pair_distances of the run's samples at the largest rmax of a case, kept while the trajectory is the same one."""
    hit = PAIRS.get(key)
    if hit is None or hit[0] < rmax or not np.array_equal(hit[1], xs):
        numbers, _, cell, pbc = frame
        PAIRS[key] = hit = (rmax, xs.copy(), {n: R.pair_distances((numbers, xs[n], cell, pbc), rmax) for n in range(0, len(xs), EVERY)})
    return hit[2]


def rdf_checks(frame, rmax, label, top=None, bins=BINS, rmin=RMIN, v0=None, langevin=True):
    """The three assertions on md_rdf for one frame and rmax.  Returns (table, the twin, the reference's near table, positions)."""
    from autoforce_amd.workloads import RdfCounts
    from test_hip_rdf_device import _same
    numbers, pos, cell, pbc = frame
    attach = lambda mdl: mdl.md_rdf(EVERY, rmax, bins, rmin)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_rdf_table(), v0=v0, langevin=langevin)
    tw = RdfCounts(EVERY, rmax, bins, rmin, numbers, SPECIES, cell, pbc)
    for x in xs:
        tw.add(x)
    _same(tab, tw.table(), f"{label} against the twin")
    pairs = _pairs(label.split(",")[0], frame, xs, rmax if top is None else top)
    H, near = np.zeros_like(tab["hist"], dtype=np.int64), np.zeros_like(tab["hist"], dtype=np.int64)
    for n, p in pairs.items():
        h, e = R.rdf((numbers, xs[n], cell, pbc), SPECIES, rmin, rmax, bins, p)
        H, near = H + h, near + e
    print(f"{L.describe(label, frame)} rmax {rmax:.3f} R {list(tw.R)}: entries {int(H.sum())}, near {int(near.sum())}")
    assert H.sum() > 0
    msg = R.mismatch(tab["hist"], H, near, f"{L.describe(label, frame)} rmax {rmax:.3f} against the all-images reference")
    assert msg is None, msg
    again, xs2 = run(frame, attach, lambda mdl: mdl.md_rdf_table(), v0=v0, langevin=langevin)
    assert np.array_equal(xs2, xs) and np.array_equal(again["hist"], tab["hist"]), f"{label}: a second run changed the bits"
    return tab, tw, near, xs


# ------------------------------------------------------------------ (a) pair distances on the walk frame
@pytest.mark.parametrize("factor,want_R", [(0.45, 0), (0.9, 1), (1.6, 2)])
def test_rdf_on_the_left_handed_walk_frame(factor, want_R):
    """rmax at 0.45, 0.9 and 1.6 smallest heights: the single-image form, and the image block with R = 1 and 2."""
    frame = _walk_start()
    h = heights(frame[2]).min()
    _, tw, _, _ = rdf_checks(frame, factor * h, f"walk, {factor} heights", top=1.6 * h)
    assert list(tw.R) == [want_R] * 3


def test_rdf_refusal_beyond_two_images_leaves_the_handle_working():
    frame = _walk_start()
    h = heights(frame[2]).min()

    def attach(mdl):
        with pytest.raises(NotImplementedError, match="cell height"):
            mdl.md_rdf(EVERY, 2.6 * h, BINS, RMIN)
        mdl.md_rdf(EVERY, 0.45 * h, BINS, RMIN)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_rdf_table())
    plain, xs2 = run(frame, lambda mdl: mdl.md_rdf(EVERY, 0.45 * h, BINS, RMIN), lambda mdl: mdl.md_rdf_table())
    assert np.array_equal(xs, xs2) and np.array_equal(tab["hist"], plain["hist"]) and tab["hist"].sum() > 0


# ------------------------------------------------------------------ (b) open directions
OPEN = [pbc for pbc in L.PBCS if 0 < sum(pbc) < 3]


@pytest.mark.parametrize("pbc", OPEN, ids=lambda p: "".join("FT"[int(x)] for x in p))
def test_rdf_with_open_directions_in_a_left_handed_cell(pbc):
    """The reference has no image along an open direction: a device R other than 0 there, or a flag read for the wrong
    direction, changes the table (the three heights differ, and the atoms are spread over eight cells along every direction)."""
    frame = L.push_apart(L.family("triclinic", "left", pbc=pbc, natoms=L.PBC_ATOMS), L.PHYS["dmin"])
    axis, h = smallest_periodic_height(frame)
    _, tw, _, _ = rdf_checks(frame, 0.9 * h, f"triclinic left {''.join('FT'[int(x)] for x in frame[3])}")
    assert tw.R[axis] == 1 and all(tw.R[k] == 0 for k in range(3) if not frame[3][k])


# ------------------------------------------------------------------ (c) one crystal, five descriptions
RMAX5 = 10.0     # one image block [1, 2, 1] (the doubly sheared cell) beside [1, 1, 1]


def _sq_checks(tab, frame, hkl, lags, xs, label):
    """md_sq's table against the twin (test_hip_sq_device._within) and against the direct reference (the same a-priori bound).
    Returns the bound (B, F) of this description."""
    from autoforce_amd.workloads import SqRing
    from test_hip_sq_device import WORST, _within
    numbers, _, cell, pbc = frame
    tw = SqRing(EVERY, hkl, lags, 1, numbers, SPECIES, cell, pbc)
    for x in xs:
        tw.add(x)
    _within(tab, tw.table(), tw.smax, f"{label} against the twin")
    WORST_SQ["twin"] = max(WORST_SQ["twin"], WORST["f"], WORST["mean"])
    B, F = sq_bounds(np.abs(hkl).max(), tw.smax, tab["n"], tab["count"])
    WORST_SQ["reference"] = max(WORST_SQ["reference"], *sq_within(tab, R.sq(xs, hkl, EVERY, lags, 1, numbers, SPECIES, cell), B, F, f"{label} against the reference"))
    print(f"sq, worst deviation over bound so far: {WORST_SQ}")
    return (B, F), tw.smax


def test_rdf_and_sq_on_one_crystal_in_five_descriptions():
    """Plain velocity Verlet (the deviates of a thermostat do not turn with the cell) from the same velocities, turned with the
    rotated description: the five runs are one trajectory up to rounding.  The RDF tables are equal bit for bit — no distance is
    within 1e-9 bin widths of an edge in any description, asserted first —, the structure factors within the sum of two bounds."""
    from autoforce_amd.workloads import RdfCounts
    from test_hip_rdf_device import _same
    twins = L.physics_twins()
    v = _v0(twins["reduced"][0][0])
    rdf, sq, bounds, Rs = {}, {}, {}, {}
    for label, (frame, _, Rot) in twins.items():
        numbers, pos, cell, pbc = frame
        hkl = hkl_of(label)

        def attach(mdl):
            mdl.md_rdf(EVERY, RMAX5, BINS, RMIN)
            mdl.md_sq(EVERY, hkl, 2, 1)
        read = lambda mdl: (mdl.md_rdf_table(), mdl.md_sq_table())
        v0 = v if Rot is None else v @ Rot
        (rdf[label], sq[label]), xs = run(frame, attach, read, v0=v0, langevin=False)
        tw = RdfCounts(EVERY, RMAX5, BINS, RMIN, numbers, SPECIES, cell, pbc)
        for x in xs:
            tw.add(x)
        Rs[label] = list(tw.R)
        _same(rdf[label], tw.table(), f"five descriptions, {label}")
        H, near = R.rdf_run(xs, numbers, cell, pbc, SPECIES, EVERY, RMIN, RMAX5, BINS)
        print(f"five descriptions, {label}: R {Rs[label]}, entries {int(H.sum())}, near {int(near.sum())}")
        assert near.sum() == 0
        msg = R.mismatch(rdf[label]["hist"], H, near, f"five descriptions, {label}")
        assert msg is None, msg
        bounds[label], _ = _sq_checks(sq[label], frame, hkl, 2, xs, f"five descriptions, {label}")
        (again, sq2), xs2 = run(frame, attach, read, v0=v0, langevin=False)
        assert np.array_equal(xs, xs2) and np.array_equal(again["hist"], rdf[label]["hist"])
        assert np.array_equal(sq2["f"], sq[label]["f"]) and np.array_equal(sq2["mean"], sq[label]["mean"])
    assert len({tuple(r) for r in Rs.values()}) > 1, Rs          # (the descriptions do take different image blocks)
    for label in twins:
        assert np.array_equal(rdf[label]["hist"], rdf["reduced"]["hist"]), label
        B, F = bounds[label][0] + bounds["reduced"][0], bounds[label][1] + bounds["reduced"][1]
        sq_within(sq[label], sq["reduced"], B, F, f"{label} against reduced, on the device")


# ------------------------------------------------------------------ (d) van Hove on the walk frame
VH = dict(every=2, levels=2, rmax=0.06, rbins=10, tbins=4, pbins=6, dbins=23, dmax=(5.0, 8.0))


@functools.lru_cache(maxsize=None)
def _vh_reference(key):
    """The references of the trajectory kept under `key` in VH_XS: both dmax from one enumeration."""
    numbers, _, cell, pbc = _walk_start()
    xs = VH_XS[key]
    return (R.vanhove_distinct(xs, numbers, cell, pbc, SPECIES, VH["every"], VH["levels"], VH["dmax"], VH["dbins"]),
            R.vanhove_self(xs, numbers, SPECIES, VH["every"], VH["levels"], VH["rmax"], VH["rbins"], VH["tbins"], VH["pbins"]))


VH_XS = {}


@pytest.mark.parametrize("which,want_R", [(0, 0), (1, 1)])
def test_vanhove_self_and_distinct_on_the_walk_frame(which, want_R):
    """every = 2, two levels: at sample 2 both are due.  dmax = 5 A is the single-image form, 8 A the image block with R = 1; the
    distinct part against the ORDERED all-images reference (origin configuration first)."""
    from autoforce_amd.workloads import VanHoveCounts
    from test_hip_vanhove_device import _same
    frame = numbers, pos, cell, pbc = _walk_start()
    dmax = VH["dmax"][which]
    args = (VH["every"], VH["levels"], VH["rmax"], VH["rbins"], VH["tbins"], VH["pbins"], dmax, VH["dbins"])
    attach = lambda mdl: mdl.md_vanhove(*args)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_vanhove_table())
    tw = VanHoveCounts(*args, numbers, SPECIES, cell, pbc)
    for x in xs:
        tw.add(x)
    assert list(tw.R) == [want_R] * 3 and list(tw.count) == [6, 3]
    _same(tab, tw.table(), f"van Hove dmax {dmax} against the twin")
    if "walk" not in VH_XS or not np.array_equal(VH_XS["walk"], xs):
        VH_XS["walk"] = xs.copy()
        _vh_reference.cache_clear()
    want_d, (Hs, over, near, near_over, count) = _vh_reference("walk")
    H, nd = want_d[dmax]
    print(f"van Hove dmax {dmax}: distinct entries {int(H.sum())}, near {int(nd.sum())}; self entries {int(Hs.sum())}, over {int(over.sum())}, "
          f"near {int(near.sum())} + {int(near_over.sum())}")
    assert np.array_equal(tab["count"], count) and H.sum() > 0 and Hs.sum() > 0
    for k, want, e in (("distinct", H, nd), ("self", Hs, near), ("over", over, near_over)):
        msg = R.mismatch(tab[k], want, e, f"van Hove {k}, dmax {dmax}") if k != "over" else \
            (None if np.all(np.abs(tab[k].astype(np.int64) - want) <= e) else f"van Hove over: {tab[k]} against {want}")
        assert msg is None, msg
    again, xs2 = run(frame, attach, lambda mdl: mdl.md_vanhove_table())
    assert np.array_equal(xs, xs2) and all(np.array_equal(again[k], tab[k]) for k in ("self", "over", "distinct", "count"))


# ------------------------------------------------------------------ (e) bond angles
ADF_CUT = {(3, 16): L.RC, (16, 16): 2.8}      # (3, 3) is absent: the zero entry of the table
ADF_BINS = 36


@pytest.mark.parametrize("label", ["shear", "shear2", "left", "thin"])
def test_adf_in_sheared_cells_and_with_an_atoms_own_images_in_its_list(label):
    """md_adf_kernel rebuilds d from the step list's image codes and the cell: the sheared descriptions have codes the reduced
    cell does not, and in the thin cell (height below RC: test_accumulator_geometry_cpu.py) every atom's own images at +- the
    first cell vector are its neighbours, exactly 180 degrees apart."""
    from autoforce_amd.workloads import AdfCounts, adf_cutoffs
    from test_hip_adf_device import _same
    frame = numbers, pos, cell, pbc = L.thin_frame() if label == "thin" else L.physics_twins()[label][0]
    cut = L.RC if label == "thin" else ADF_CUT
    ctab = adf_cutoffs(cut, SPECIES)
    assert label == "thin" or (ctab[0, 0] == 0.0 and ctab.max() <= L.RC)
    attach = lambda mdl: mdl.md_adf(1, ADF_BINS, cut)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_adf_table())
    tw = AdfCounts(1, ADF_BINS, cut, numbers, SPECIES, cell, pbc)
    for x in xs:
        tw.add(x)
    _same(tab, tw.table(), f"adf {label} against the twin")
    want = R.adf_run(xs, numbers, cell, pbc, SPECIES, ctab, 1, ADF_BINS)
    print(f"adf {label}: angles {int(want['angles'].sum())}, near {int(want['near'].sum())}, loose {want['loose']}, smallest gaps "
          f"{want['gap_angle']:.2e} rad, {want['gap_r']:.2e} A")
    assert want["angles"].sum() > 1000
    for k in ("angles", "coord"):
        msg = R.mismatch(tab[k], want[k], want["near"] if k == "angles" else np.zeros_like(want[k]), f"adf {label} {k}", loose=want["loose"])
        assert msg is None, msg
    if label == "thin":
        assert tab["angles"][:, :, :, ADF_BINS - 1].sum() >= EVALS * len(numbers)      # (an atom's two images: one angle of pi per centre)
    again, xs2 = run(frame, attach, lambda mdl: mdl.md_adf_table())
    assert np.array_equal(xs, xs2) and np.array_equal(again["angles"], tab["angles"]) and np.array_equal(again["coord"], tab["coord"])


# ------------------------------------------------------------------ (f) structure factors on the walk frame
def _walk_hkl(top):
    return np.array([(-1, 2, 0), (0, 1, -3), (-5, 0, 7), (0, 0, 2), (0, 3, 0), (4, 0, 0), (top, 0, 0), (0, -top, 0), (0, 0, top), (-top, top, -top),
                     (top - 1, -3, 5), (1, 1, 1), (-2, -3, -4)])


@pytest.mark.parametrize("top", [16, 32])
def test_sq_on_the_left_handed_walk_frame(top):
    """Indices up to 16 and up to 32 (the two compiled forms), negative ones, a zero in each axis; the atoms are unwrapped, up to
    four and a half cells out."""
    frame = _walk_start()
    hkl = _walk_hkl(top)
    attach = lambda mdl: mdl.md_sq(EVERY, hkl, 3, 1)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_sq_table())
    _, smax = _sq_checks(tab, frame, hkl, 3, xs, f"walk, indices up to {top}")
    assert 3.5 < smax < 6.0, smax
    again, xs2 = run(frame, attach, lambda mdl: mdl.md_sq_table())
    assert np.array_equal(xs, xs2) and np.array_equal(again["f"], tab["f"]) and np.array_equal(again["mean"], tab["mean"])


def test_sq_on_a_partly_open_cell_takes_no_vector_along_the_open_direction():
    from autoforce_amd import SgprError
    from autoforce_amd.workloads import SqRing
    frame = L.push_apart(L.family("triclinic", "left", pbc=(True, False, True), natoms=L.PBC_ATOMS), L.PHYS["dmin"])
    numbers, pos, cell, pbc = frame
    open_axis = [k for k in range(3) if not pbc[k]]
    assert open_axis == [0]                           # (the left-handed twin swaps the first two flags)
    good = np.array([(0, 1, 0), (0, -2, 3), (0, 0, 5), (0, 16, -7)])
    bad = good.copy()
    bad[2, 0] = 1
    with pytest.raises(ValueError):
        SqRing(EVERY, bad, 2, 1, numbers, SPECIES, cell, pbc)

    def attach(mdl):
        with pytest.raises(SgprError, match="not periodic"):
            mdl.md_sq(EVERY, bad, 2, 1)
        mdl.md_sq(EVERY, good, 2, 1)
    tab, xs = run(frame, attach, lambda mdl: mdl.md_sq_table())
    _sq_checks(tab, frame, good, 2, xs, "triclinic left, first direction open")


# ------------------------------------------------------------------ (g) all six together
def test_all_six_accumulators_together_have_the_bits_each_has_alone():
    """md_msd and md_vacf do not read the cell: in the left-handed cell with unwrapped atoms they equal what they give alone, and
    md_msd its twin bit for bit and the plain reference within the bound of test_accumulator_geometry_cpu._msd_within."""
    from autoforce_amd.workloads import MsdBlocks
    from test_accumulator_geometry_cpu import _msd_within
    from test_hip_msd_device import _same as msd_same
    frame = numbers, pos, cell, pbc = _walk_start()
    h = heights(cell).min()
    vh = (VH["every"], VH["levels"], VH["rmax"], VH["rbins"], VH["tbins"], VH["pbins"], VH["dmax"][1], VH["dbins"])
    hkl = _walk_hkl(16)
    six = dict(
        msd=(lambda m: m.md_msd(1, 3, True), lambda m: m.md_msd_table(), ("count", "msd", "msd_sq", "smd", "smd_sq")),
        rdf=(lambda m: m.md_rdf(EVERY, 0.9 * h, BINS, RMIN), lambda m: m.md_rdf_table(), ("hist",)),
        vacf=(lambda m: m.md_vacf(1, 5, 2, True), lambda m: m.md_vacf_table(), ("tracer", "collective", "count")),
        vanhove=(lambda m: m.md_vanhove(*vh), lambda m: m.md_vanhove_table(), ("self", "over", "distinct", "count")),
        adf=(lambda m: m.md_adf(2, ADF_BINS, ADF_CUT), lambda m: m.md_adf_table(), ("angles", "coord")),
        sq=(lambda m: m.md_sq(EVERY, hkl, 3, 1), lambda m: m.md_sq_table(), ("f", "mean", "count")))
    together, xs = run(frame, lambda m: [a(m) for a, _, _ in six.values()], lambda m: {k: r(m) for k, (_, r, _) in six.items()})
    for name, (attach, read, keys) in six.items():
        alone, xs1 = run(frame, attach, read)
        assert np.array_equal(xs1, xs), name
        for k in keys:
            assert np.array_equal(alone[k], together[name][k]), (name, k)
            assert np.any(np.asarray(alone[k]) != 0), (name, k)
    tw = MsdBlocks(1, 3, True, _mass(numbers), numbers, SPECIES)
    for x in xs:
        tw.add(x)
    msd_same(together["msd"], tw.table(), "msd on the walk frame against the twin")
    _msd_within(together["msd"], R.msd(xs, numbers, SPECIES, _mass(numbers), 1, 3, True), xs, len(numbers))
