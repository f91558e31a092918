"""GPU tests of the GEOMETRY of the device neighbour list — the bin grid of nl_grid.inc (nl_make_grid, nl_place_axis,
nl_store_rec), nl_bin_kernel and the sweep of nl_fwd_kernel — on the frames of lattices.py: sheared, rotated and left-handed
cells with three to five bins per edge and atoms up to four cells outside, heights on a multiple of rc, cells on either side
of the `ortho` threshold, atoms on the faces and corners of the grid, pairs 1e-10 rc inside and outside the cut-off, atoms
tens of cells apart up to the image code's limit and the two refusals beyond it, one crystal in five descriptions, candidates
kept over a walk, the binning of the MD loop's last kernel, and a sharded build.  test_lattices_cpu.py proves with the oracle
alone that every frame is the edge it claims to be.

Every case asserts of the list: the lengths (ptr) equal the reference's, the set of (i, j, off) equals the reference's (no
tolerance: a pair is listed or it is not), every atom's list ascends strictly by (species slot, j, image), and a second
predict of the same frame (a step that reuses the candidates) returns the identical arrays.  The reference is
oracle.neighbors (all pairs over all images) unless a case says otherwise.  A failure names the frame, its handedness, the
periodicity pattern and the first missing and extra triple with its distance."""
import functools

import numpy as np
import pytest

import lattices as L
from lattices import RC
from test_hip_list_edges import ascending

pytestmark = pytest.mark.gpu

ETA = 4.0


def list_model(rc=RC, skin0=False):
    """A model without inducing points: predict builds the lists and returns zeros (test_hip_paths.test_degenerate_inputs)."""
    from autoforce_amd import SGPRModel, _lib
    mdl = SGPRModel(3, 3, ETA, rc, species=L.SPECIES)
    if skin0:
        _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 0))
    return mdl


class both_skins:
    """Two handles for one cut-off.  The bin grid is made for the CANDIDATE cut-off rc + skin (neighbor.hip): with skin 0 it is
    the grid of rc that lattices.grid_of states and the frames were built for — every sweep is a rebuild and prunes bins
    against rc itself; with the default skin of 0.5 A the same frames are binned more coarsely (grid_of at rc + 0.5) and the
    second predict of a frame is a step that reuses the candidates."""

    def __init__(self, rc=RC):
        self.rc = rc

    def __enter__(self):
        self.models = [("skin 0", list_model(self.rc, True)), ("skin 0.5", list_model(self.rc))]
        return self.models

    def __exit__(self, *exc):
        for _, m in self.models:
            m.close()


def brute(frame, rc):
    from oracle import oracle as orc
    _, pos, cell, pbc = frame
    return orc.neighbors(pos, cell, pbc, rc)


@functools.lru_cache(maxsize=None)
def family_reference(name, variant, pbc, natoms):
    frame = L.family(name, variant, pbc=pbc, natoms=natoms)
    return frame, brute(frame, RC)


def check_list(mdl, frame, want, label, marked=()):
    """The four assertions of this file on one frame, plus the marked pairs: listed or not, as the frame was built.  mdl: a
    handle, or the pairs (name, handle) of both_skins — each is checked."""
    if isinstance(mdl, list):
        return [check_list(m, frame, want, f"{label}, {name}", marked) for name, m in mdl][0]
    numbers, pos, cell, pbc = frame
    N = len(numbers)
    mdl.predict(numbers, pos, cell, pbc)
    got = mdl.neighbors(N)
    msg = L.list_diff(label, frame, got, want)
    assert msg is None, msg
    assert np.array_equal(got[0], want[0]), f"{L.describe(label, frame)}: list lengths differ (an entry listed twice?)"
    bad = ascending(mdl, numbers, *got)
    assert bad == [], f"{L.describe(label, frame)}: lists not ascending by (slot, j, image) at atoms {bad[:8]}"
    have = L.triples(*got)
    for t, listed in marked:
        assert (t in have) == listed, (f"{L.describe(label, frame)}: (i, j, off) = {t} at {L.distance(frame, t):.13f} A is "
                                       f"{'not ' if listed else ''}listed")
    mdl.predict(numbers, pos, cell, pbc)
    again = mdl.neighbors(N)
    for x, y in zip(got, again):
        assert np.array_equal(x, y), f"{L.describe(label, frame)}: the second predict of the frame changed the list"
    return got


# ------------------------------------------------------------------ (a) families
@pytest.mark.parametrize("name", sorted(L.FAMILIES))
def test_families_given_rotated_and_left_handed(name):
    """pbc TTT.  One handle takes the three descriptions one after the other: the cell changes, the crystal does not."""
    with both_skins() as mdl:
        for variant in L.VARIANTS:
            frame, want = family_reference(name, variant, (True, True, True), None)
            check_list(mdl, frame, want, f"{name} {variant}")


@pytest.mark.parametrize("variant", ["given", "left"])
@pytest.mark.parametrize("name", ["hex120", "triclinic"])
def test_families_under_all_eight_periodicity_patterns(name, variant):
    """Along an open direction the grid has one slab: 150 atoms spread over eight cell lengths fall into as few as one bin,
    whose capacity (64 to begin with) the call grows before it returns — the list is complete all the same."""
    with both_skins() as mdl:
        for pbc in L.PBCS:
            frame, want = family_reference(name, variant, pbc, L.PBC_ATOMS)
            check_list(mdl, frame, want, f"{name} {variant}")


# ------------------------------------------------------------------ (b) grid-count edges
@pytest.mark.parametrize("kind,k,side", L.GRID_EDGES)
def test_heights_on_a_multiple_of_rc(kind, k, side):
    """floor(height / rc) decides nb and ceil(rc nb / height) decides rng within an ulp of k rc: the list is the reference's
    whichever count the device lands on (the host's, by grid_of, is printed).  k = 16 and 17: the cap of 16 bins per edge."""
    e = L.grid_edge(kind, k, side)
    frame, rc = e["frame"], e["rc"]
    g = L.grid_of(frame[2], frame[3], rc)
    print(f"{kind} k={k} side={side:+d}: height - k rc = {(g['hgt'][0] - k * rc) / np.spacing(k * rc):+.1f} ulp, host nb {g['nb']}, rng {g['rng']}")
    with both_skins(rc) as mdl:
        check_list(mdl, frame, brute(frame, rc), f"grid edge {kind} k={k} side={side:+d}")


# ------------------------------------------------------------------ (c) the ortho threshold
@pytest.mark.parametrize("skin0", [False, True], ids=["skin", "noskin"])
@pytest.mark.parametrize("cos", L.ORTHO_COS)
def test_either_side_of_the_ortho_threshold(cos, skin0):
    """Pairs at rc (1 - 1e-10) whose bins are diagonal neighbours, the nearer atom rc (1 - 2e-10) from the shared corner: with
    no skin the sweep's bound on the distance to that bin is within 4e-10 of the cut-off it is compared with — Euclidean below
    a cosine of 1e-10 between plane normals, the largest plane gap above.  All of them are listed."""
    e = L.ortho_edge(cos)
    frame, rc = e["frame"], e["rc"]
    for t, _ in e["marked"]:
        assert np.longdouble(L.distance(frame, t)) < np.longdouble(rc)
    mdl = list_model(rc, skin0)
    check_list(mdl, frame, brute(frame, rc), f"ortho edge cos={cos:g}", marked=e["marked"])
    mdl.close()


# ------------------------------------------------------------------ (d) faces and corners
@pytest.mark.parametrize("turn", range(4))
@pytest.mark.parametrize("kind", sorted(L.FACE_CELLS))
def test_atoms_on_the_faces_and_corners_of_the_grid(kind, turn):
    """Fractional coordinates 0, 1, k / nb, -2^-60 and 1 - 2^-53 on all three axes at once (the clamp of nl_place_axis), each
    atom with a partner rc - 1e-5 away on either side."""
    e = L.face_frame(kind, turn)
    frame = e["frame"]
    with both_skins() as mdl:
        check_list(mdl, frame, brute(frame, RC), f"faces {kind} turn {turn}", marked=e["marked"])


# ------------------------------------------------------------------ (e) exactly at the cut-off
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("kind", sorted(L.FACE_CELLS) + ["self"])
def test_pairs_a_tenth_of_a_billionth_inside_and_outside_the_cutoff(kind, sign):
    """Pairs at rc (1 - 1e-10) are listed, at rc (1 + 1e-10) not: inside one image, across a cell face, across the cell's corner,
    across a corner of the bin grid, and ("self") every atom with its own image in a cell whose edge is rc (1 -+ 1e-10).
    The margin: with coordinates under 100 A a component of a displacement rounds by at most 2e-14 A, and the handful of
    operations of either side's formula keep the distance within 1e-13 rc — three orders below 1e-10.  The side of every
    marked pair is confirmed in extended precision first."""
    e = L.self_image_frame(sign) if kind == "self" else L.cutoff_frame(kind, sign)
    frame, rc = e["frame"], e["rc"]
    assert np.abs(frame[1]).max() < 100.0
    for t, listed in e["marked"]:
        assert (np.longdouble(L.distance(frame, t)) < np.longdouble(rc)) == listed == (sign < 0), t
    with both_skins() as mdl:
        check_list(mdl, frame, brute(frame, rc), f"cut-off {kind} sign {sign:+d}", marked=e["marked"])


# ------------------------------------------------------------------ (f) large, unequal displacements
def test_atoms_up_to_sixty_cells_away_each_by_its_own_amount():
    """relabel() on the sheared triclinic family and its left-handed twin: the reference is the base frame's brute-force list
    with every image triple shifted by n[i] - n[j] (test_lattices_cpu.py holds relabel against brute force at small shifts)."""
    rng = np.random.default_rng(60)
    with both_skins() as mdl:
        for variant in ("given", "left"):
            frame, base = family_reference("triclinic", variant, (True, True, True), None)
            n = rng.integers(-60, 61, size=(len(frame[0]), 3))
            moved, want = L.relabel(frame, n, base)
            assert np.abs(want[2]).max() > 100
            check_list(mdl, moved, want, f"triclinic {variant} relabelled by up to 60 cells")


def test_image_code_limit_and_the_two_refusals():
    """One atom moved until the image component to one of its neighbours is exactly 127 — the last value the packed code
    holds: listed.  At 128 the call refuses with the overflow code and tells the caller to wrap the positions; so it does
    with every atom 33000 cells from the origin (the wrap count beyond int16, all image components small).  After each
    refusal the handle predicts the unshifted frame and returns the list from before."""
    from autoforce_amd import SgprError, _lib
    frame, base = family_reference("triclinic", "given", (True, True, True), None)
    numbers, pos, cell, pbc = frame
    N, i = len(numbers), 5
    assert base[0][i + 1] > base[0][i]
    top = int(base[2][base[0][i]:base[0][i + 1], 0].max())
    n = np.zeros((N, 3), np.int64)
    n[i, 0] = 127 - top
    moved, want = L.relabel(frame, n, base)
    assert np.abs(want[2]).max() == 127
    n[i, 0] += 1
    over, _ = L.relabel(frame, n, base)
    far, _ = L.relabel(frame, np.tile([33000, 0, 0], (N, 1)), base)
    with both_skins() as models:
        for name, mdl in models:
            check_list(mdl, frame, base, f"triclinic, {name}")
            check_list(mdl, moved, want, f"triclinic, one image component at 127, {name}")
            for what, fr in (("an image component of 128", over), ("all atoms 33000 cells away", far)):
                with pytest.raises(SgprError) as err:
                    mdl.predict(*fr)
                assert err.value.code == _lib.E_OVERFLOW and "wrap the positions into the cell" in str(err.value), (what, name, str(err.value))
                check_list(mdl, frame, base, f"triclinic after the refusal of {what}, {name}")


# ------------------------------------------------------------------ (g) same crystal, five descriptions
def physics_model(frame):
    from autoforce_amd import Local, SGPRModel
    P = L.PHYS
    mdl = SGPRModel(3, 3, P["eta"], P["rc"], species=L.SPECIES)
    mdl.set_inducing([Local(z, b, r) for z, b, r in L.physics_inducing(frame, P["rc"], P["m"])])
    return mdl


def test_one_crystal_in_five_descriptions():
    """The 120-atom two-species frame in its reduced cell, in the cells U h and U^2 h (angles down to 28 degrees), left-handed
    and rotated: compare() of test_hip_paths.py with its own tolerances on each (K_mm, cov, energy, forces, stress, beta, the
    covloss bound — each description against the oracle on that description; test_lattices_cpu.py shows the oracle agrees
    with itself to 1e-14), and the device's lists map onto each other exactly through reshear's triple transform."""
    from test_hip_paths import compare
    P = L.PHYS
    twins = L.physics_twins()
    mdl, bare = physics_model(twins["reduced"][0]), list_model(P["rc"], skin0=True)
    mdl.set_weights(np.random.default_rng(9).normal(size=P["m"]))
    lists = {}
    for label, (frame, to_twin, R) in twins.items():
        numbers, pos, cell, pbc = frame
        want = brute(frame, P["rc"])
        lists[label] = check_list(mdl, frame, want, f"physics {label}")
        check_list(bare, frame, want, f"physics {label}, skin 0")
        compare(mdl, 3, 3, P["eta"], P["rc"], numbers, pos, cell, list(pbc), want)
    for label, (frame, to_twin, R) in twins.items():
        mapped = to_twin(L.sort_list(*lists["reduced"]))
        for x, y in zip(mapped, L.sort_list(*lists[label])):
            assert np.array_equal(x, y), L.list_diff(f"physics {label} against the mapped list of the reduced cell", frame, lists[label], mapped)
    mdl.close(); bare.close()


# ------------------------------------------------------------------ (h) candidates kept across steps
def test_candidates_kept_over_a_walk_in_a_sheared_left_handed_cell():
    """Twelve steps of 0.03 A moves, atoms up to four cells outside, one atom carried through a face by a lattice vector: at
    every step the list of a handle with the default skin equals that of a handle with skin 0 (array for array) and the
    oracle's; the candidates are rebuilt once after the first build — for the carried atom — and reused otherwise."""
    from oracle import oracle as orc
    W = L.WALK
    frame, frames = L.walk_frames()
    numbers, pos, cell, pbc = frame
    N = len(numbers)
    fast, slow = list_model(), list_model(skin0=True)
    for step, p in enumerate(frames):
        fr = (numbers, p, cell, pbc)
        want = brute(fr, RC) if step in (0, W["carry_step"], W["steps"] - 1) else orc.neighbors_cells(p, cell, pbc, RC)
        a = check_list(fast, fr, want, f"walk step {step}, default skin")
        b = check_list(slow, fr, want, f"walk step {step}, skin 0")
        for x, y in zip(a, b):
            assert np.array_equal(x, y), f"walk step {step}: the lists of the two handles differ"
        if step == 0:
            r0 = fast.list_rebuilds(), slow.list_rebuilds()
    print(f"rebuilds after the first build: default skin {fast.list_rebuilds() - r0[0]}, skin 0 {slow.list_rebuilds() - r0[1]}")
    assert fast.list_rebuilds() - r0[0] == 1, (r0, fast.list_rebuilds())
    assert slow.list_rebuilds() - r0[1] >= W["steps"] - 1
    fast.close(); slow.close()


# ------------------------------------------------------------------ (i) the last kernel's own binning
def test_md_loop_bins_the_walk_frame_for_itself():
    """Sixteen evaluations of the device Langevin loop at 600 K on the frame of (h): from the second on the atoms are binned
    by the step's last kernel (finalize_next_kernel, through nl_place_axis) in the left-handed sheared cell, with their wraps
    of up to four cells.  The list of the last evaluated configuration against oracle.neighbors on its positions."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    frame, _ = L.walk_frames()
    numbers, pos, cell, pbc = frame
    N, m = len(numbers), L.PHYS["m"]
    mdl = physics_model(frame)
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(2 * m, m)), rng.normal(size=2 * m))
    mdl.set_weights(0.02 * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
    mass = np.array([MASS[int(z)] for z in numbers])
    v0 = np.random.default_rng(11).normal(size=(N, 3)) * np.sqrt(kB * 600.0 / mass[:, None])
    mdl.md_begin(numbers, pos, cell, pbc, mass, v0, dt=FS, friction=1e-3, kT=kB * 600.0, seed=11)
    done = 0
    for _ in range(8):   # (halt code 2: a capacity was outgrown at evaluation `done`; the call is repeated)
        sc, code = mdl.md_run(16 - done, None)
        assert code in (0, 2), code
        done += len(sc)
        if done == 16:
            break
    assert done == 16
    st = mdl.md_state(which=-1)
    assert 0.005 < np.abs(st["positions"] - pos).max() < 1.0       # moved, and by thermal steps only
    fr = (numbers, st["positions"], cell, pbc)
    gap = L.gap_to_rc(fr, RC)
    print(f"MD: largest move {np.abs(st['positions'] - pos).max():.3f} A, gap to rc at the last configuration {gap:.2e} A")
    assert gap > 1e-9
    got = mdl.neighbors(N)
    want = brute(fr, RC)
    msg = L.list_diff("walk frame after 16 MD evaluations", fr, got, want)
    assert msg is None, msg
    assert np.array_equal(got[0], want[0]) and ascending(mdl, numbers, *got) == []
    mdl.md_end()
    mdl.close()


# ------------------------------------------------------------------ (j) sharded
def test_three_ranks_list_their_own_atoms_and_sum_to_the_whole():
    """World 3 on the sheared physics frame: each rank lists its own atoms, the union is the reference; the partial energies,
    forces, stress, beta and cov sum to the whole as in test_hip_parity.test_sharded_partials_sum_to_the_whole."""
    P = L.PHYS
    frame = numbers, pos, cell, pbc = L.physics_twins()["shear"][0]
    N = len(numbers)
    mdl = physics_model(L.physics_frame())
    mdl.set_weights(np.random.default_rng(9).normal(size=P["m"]))
    want = brute(frame, P["rc"])
    whole = mdl.predict(numbers, pos, cell, pbc, cov=True)
    union, acc, owners = set(), None, np.zeros(N, int)
    for r in range(3):
        part = mdl.predict(numbers, pos, cell, pbc, rank=r, world=3, cov=True)
        got = mdl.neighbors(N)
        owners += np.diff(got[0]) > 0
        mine = L.triples(*got)
        assert not (mine & union) and ascending(mdl, numbers, *got) == []
        union |= mine
        acc = {k: np.array(v, dtype=float) for k, v in part.items()} if acc is None else {k: acc[k] + part[k] for k in acc}
    assert union == L.triples(*want), L.list_diff("physics shear, union of three ranks", frame, _as_list(union, N), want)
    assert np.array_equal(owners, (np.diff(want[0]) > 0).astype(int))
    assert abs(acc["energy"] - whole["energy"]) <= 1e-12 * max(1.0, abs(whole["energy"]))
    for k in ("forces", "stress", "beta", "cov"):
        np.testing.assert_allclose(acc[k], whole[k], rtol=0, atol=1e-12 * max(1.0, np.abs(whole[k]).max()), err_msg=k)
    mdl.close()


def _as_list(trip, N):
    t = np.array(sorted(trip), np.int64).reshape(-1, 5)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(t[:, 0], minlength=N))])
    return ptr, t[:, 1].astype(np.int32), t[:, 2:].astype(np.int32)


# ------------------------------------------------------------------ the bound the sweep prunes bins by, in sheared cells
@pytest.mark.parametrize("name,skin", L.PRUNE_CASES)
def test_pairs_a_euclidean_bin_bound_would_drop(name, skin):
    """In a sheared cell the distance to a bin is bounded by the largest plane gap only (lb2 = gm * gm in nl_fwd_kernel).
    Sixteen pairs per frame (fewer with the default skin) sit across corners and edges of the grid this handle makes, where
    the Euclidean norm of the gaps exceeds rc + skin although the pair is inside rc: each must be listed.  Given, rotated
    and left-handed."""
    mdl = list_model(skin0=skin == 0.0)
    for variant in L.VARIANTS:
        e = L.prune_frame(name, variant, skin)
        assert e["pairs"] >= 3
        check_list(mdl, e["frame"], brute(e["frame"], RC), f"prune {name} {variant}, skin {skin}", marked=e["marked"])
    mdl.close()
