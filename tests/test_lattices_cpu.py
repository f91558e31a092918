"""The preconditions of test_hip_list_geometry.py, proved with the CPU oracle alone: every frame of lattices.py is the edge
it claims to be (bins per edge, handedness, the side of a threshold, the side of the cut-off of every constructed pair), the
oracle's two list builders agree on it, the maps relabel / reshear / variant_map predict the brute-force list exactly, and the
oracle computes the same physics on every description of one crystal.  Nothing here touches the device.  Every case prints
its figures (pytest -s)."""
import numpy as np
import pytest

import lattices as L
from lattices import RC

LD = np.longdouble


def _lists(frame, rc):
    """Brute force and linked cells, asserted equal; returns the list."""
    from oracle import oracle as orc
    _, pos, cell, pbc = frame
    a, b = orc.neighbors(pos, cell, pbc, rc), orc.neighbors_cells(pos, cell, pbc, rc)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    return a


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _report(label, frame, rc, nl):
    g, gs = L.grid_of(frame[2], frame[3], rc), L.grid_of(frame[2], frame[3], rc + L.SKIN)
    gap = L.gap_to_rc(frame, rc)
    print(f"{L.describe(label, frame)}: {len(frame[0])} atoms, nb {g['nb']}, rng {g['rng']}, ortho {g['ortho']}, height / rc "
          f"{np.array2string(g['ratio'], precision=4)}, longest list {int(np.diff(nl[0]).max())}, gap to rc {gap:.2e} A; "
          f"with the default skin nb {gs['nb']}, rng {gs['rng']}")
    return g, gap


# ------------------------------------------------------------------ families
@pytest.mark.parametrize("variant", L.VARIANTS)
@pytest.mark.parametrize("name", sorted(L.FAMILIES))
def test_family_frames_are_what_they_claim(name, variant):
    frame = numbers, pos, cell, pbc = L.family(name, variant)
    nl = _lists(frame, RC)
    g, gap = _report(f"{name} {variant}", frame, RC, nl)
    assert 50 <= len(numbers) <= 150 and set(numbers.tolist()) == set(L.SPECIES)
    assert all(3 <= n <= 5 for n in g["nb"]) and g["rng"] == [1, 1, 1] and g["ortho"] == 0
    assert np.abs(g["ratio"] - np.rint(g["ratio"])).min() > 1e-3            # no height on a multiple of rc
    assert (g["det"] < 0) == (variant == "left")
    frac = pos @ np.linalg.inv(cell)
    assert frac.min() < -3.0 and frac.max() > 4.0 and frac.min() >= -3.5 - 1e-9 and frac.max() < 4.5 + 1e-9
    assert gap > 1e-6
    assert 0 < np.diff(nl[0]).max() < 64 and (nl[2] != 0).any()
    # the three descriptions are one crystal: the list of the given frame, mapped, is this frame's
    base = L.family(name, "given")
    assert _same(L.variant_map(_lists(base, RC), variant), nl)
    if variant == "rotated":
        assert np.abs(cell[np.triu_indices(3, 1)]).min() > 0.1           # general orientation: no zero component left


@pytest.mark.parametrize("name", ["hex120", "triclinic"])
@pytest.mark.parametrize("pbc", L.PBCS, ids=lambda p: "".join("FT"[int(x)] for x in p))
def test_family_frames_under_every_periodicity(name, pbc):
    """Open directions: one slab of bins, the atoms spread over eight cell lengths along them (few pairs there; the periodic
    directions keep theirs)."""
    frame = L.family(name, "given", pbc=pbc, natoms=L.PBC_ATOMS)
    nl = _lists(frame, RC)
    g, gap = _report(name, frame, RC, nl)
    assert [n == 1 for n in g["nb"]] == [not p for p in pbc] and gap > 1e-6
    assert not nl[2][:, [not p for p in pbc]].any()
    assert len(nl[1]) > 0 or not any(pbc)      # (all open: a gas, eight cell lengths wide — the list may be empty)


# ------------------------------------------------------------------ relabel, reshear
def test_relabel_predicts_the_brute_force_list():
    """Shifts of up to three cells per atom and direction, on a sheared cell and on its left-handed twin: the sign of
    off' = off + n[i] - n[j] is fixed here against oracle.neighbors."""
    rng = np.random.default_rng(3)
    for variant in ("given", "left"):
        frame = L.family("triclinic", variant, spread=(0.0, 1.0))
        nl = _lists(frame, RC)
        n = rng.integers(-3, 4, size=(len(frame[0]), 3))
        moved, want = L.relabel(frame, n, nl)
        got = _lists(moved, RC)
        assert _same(got, want), L.list_diff(f"triclinic {variant} relabelled", moved, got, want)
        assert not _same(got, nl)
    # open directions take no shift
    frame = L.family("hex120", pbc=(True, False, True), spread=(0.0, 1.0))
    n = rng.integers(-3, 4, size=(len(frame[0]), 3)) * np.array([1, 0, 1])
    moved, want = L.relabel(frame, n, _lists(frame, RC))
    assert _same(_lists(moved, RC), want)


def test_reshear_predicts_the_brute_force_list():
    twins = L.physics_twins()
    base = _lists(twins["reduced"][0], RC)
    for label, (frame, to_twin, R) in twins.items():
        got = _lists(frame, RC)
        want = to_twin(base)
        assert _same(got, want), L.list_diff(label, frame, got, want)
        g, gap = _report(f"physics {label}", frame, RC, got)
        print(f"    cell angles {np.round(L.cell_angles(frame[2]), 1)}")
        assert gap > 1e-6
    assert L.grid_of(twins["left"][0][2], [True] * 3, RC)["det"] < 0
    assert min(L.cell_angles(twins["shear2"][0][2])) < 30.0
    assert not _same(_lists(twins["shear"][0], RC), base)


# ------------------------------------------------------------------ the oracle on the twins
def _voigt_to_matrix(s):
    return np.array([[s[0], s[5], s[4]], [s[5], s[1], s[3]], [s[4], s[3], s[2]]])


def test_oracle_gives_one_physics_for_every_description():
    """Energy, forces and stress of the physics frame by oracle.frame on the reduced cell and on each twin (forces and
    stress of the rotated twin turned back).  The descriptions differ in how the same displacement is spelt (image triple
    and cell), so the results differ by rounding only: asserted at 1e-11 of the largest component, a thousandth of what
    compare() of test_hip_paths.py allows between the device and the oracle (1e-9 energy, 1e-8 forces and stress)."""
    from oracle import oracle as orc
    P = L.PHYS
    twins = L.physics_twins()
    base = twins["reduced"][0]
    numbers = base[0]
    X = L.physics_inducing(base, P["rc"], P["m"])
    species = np.array(L.SPECIES, np.int32)
    ind_z = np.array([x[0] for x in X], np.int32)
    ind_ptr = np.concatenate([[0], np.cumsum([len(x[1]) for x in X])])
    Pm, nnm = orc.inducing_descriptors(3, 3, P["rc"], species, ind_z, ind_ptr, np.concatenate([x[1] for x in X]),
                                       np.concatenate([x[2] for x in X]))
    Lc, _ = orc.jitcholesky(orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, P["eta"]))
    choli = orc.tril_inverse(Lc)
    mu = np.random.default_rng(9).normal(size=len(X))
    ref = {}
    for label, (frame, _, R) in twins.items():
        _, pos, cell, pbc = frame
        nl = orc.neighbors(pos, cell, pbc, P["rc"])
        out = orc.frame(3, 3, P["rc"], P["eta"], species, numbers, pos, cell, nl, ind_z, nnm, Pm, mu, choli=choli, want_p=False)
        F, S = out["forces"], _voigt_to_matrix(out["stress"])
        if R is not None:
            F, S = F @ R.T, R @ S @ R.T
        ref[label] = (out["energy"], F, S, out["beta"])
    E0, F0, S0, b0 = ref["reduced"]
    assert np.abs(F0).max() > 0.1 and np.abs(S0).max() > 0
    for label, (E, F, S, b) in ref.items():
        de = abs(E - E0) / max(1.0, abs(E0))
        df, ds, db = np.abs(F - F0).max() / np.abs(F0).max(), np.abs(S - S0).max() / np.abs(S0).max(), np.abs(b - b0).max()
        print(f"oracle on {label} vs reduced: energy {de:.2e}, forces {df:.2e} of the largest, stress {ds:.2e} of the largest, beta {db:.2e}")
        assert de <= 1e-11 and df <= 1e-11 and ds <= 1e-11 and db <= 1e-9, label


# ------------------------------------------------------------------ the walk
def test_walk_keeps_its_candidates_and_carries_one_atom_through_a_face():
    W = L.WALK
    frame, frames = L.walk_frames()
    numbers, pos, cell, pbc = frame
    g = L.grid_of(cell, pbc, RC)
    assert g["det"] < 0 and g["ortho"] == 0 and min(g["nb"]) >= 3
    frac = pos @ np.linalg.inv(cell)
    assert frac.min() < -3.0 and frac.max() > 4.0
    assert len(frames) == W["steps"] == 12 and np.array_equal(frames[0], pos)
    from oracle import oracle as orc
    assert len(orc.neighbors_cells(pos, cell, pbc, L.PHYS["dmin"])[1]) == 0
    for step, p in enumerate(frames):
        base = pos.copy()
        if step >= W["carry_step"]:
            base[W["carried"]] += cell[1]
        drift = np.linalg.norm(p - base, axis=1).max()
        assert drift < 0.24, (step, drift)           # (a skin of 0.5 A rebuilds beyond 0.25)
        if step:
            moved = np.linalg.norm(p - frames[step - 1], axis=1)
            moved[W["carried"]] = 0.03 if step == W["carry_step"] else moved[W["carried"]]
            assert np.allclose(moved, 0.03, rtol=1e-9)
        fr = (numbers, p, cell, pbc)
        gap = L.gap_to_rc(fr, RC)
        print(f"walk step {step}: largest drift {drift:.3f} A, gap to rc {gap:.2e} A")
        assert gap > 1e-6
        if step in (0, W["steps"] - 1):
            _lists(fr, RC)


# ------------------------------------------------------------------ constructed edges
@pytest.mark.parametrize("kind,k,side", L.GRID_EDGES)
def test_grid_edges_sit_on_their_side_of_k_rc(kind, k, side):
    e = L.grid_edge(kind, k, side)
    frame, rc = e["frame"], e["rc"]
    nl = _lists(frame, rc)
    g, gap = _report(f"grid edge {kind} k={k} side={side:+d}", frame, rc, nl)
    h = g["hgt"][0]
    print(f"    height {h!r}, k rc {k * rc!r}: (height - k rc) / ulp = {(h - k * rc) / np.spacing(k * rc):+.1f}; host nb {g['nb']}")
    # the height the host computes is on the side the case names, within a few ulp of k rc; "on" k rc is the nearest height
    # one scale factor reaches (the sheared cell with k = 16 stops one ulp below: the host then counts 15 bins)
    assert abs(h - k * rc) <= 8 * np.spacing(k * rc)
    assert np.sign(h - k * rc) == side if side else abs(h - k * rc) <= np.spacing(k * rc)
    assert g["nb"][0] == min(16, k - (h < k * rc)) and g["ortho"] == (kind == "ortho")
    assert g["nb"][1] == g["nb"][2] == min(16, k)
    assert len(frame[0]) == (80 if k == 3 else 400) and gap > 1e-6
    assert np.diff(nl[0]).min() >= 1
    if k >= 16:
        assert g["nbins"] == 4096 or (k == 16 and h < k * rc and g["nbins"] == 15 * 256)


@pytest.mark.parametrize("cos", L.ORTHO_COS)
def test_ortho_threshold_frames(cos):
    e = L.ortho_edge(cos)
    frame, rc = e["frame"], e["rc"]
    nl = _lists(frame, rc)
    g, _ = _report(f"ortho edge cos={cos:g}", frame, rc, nl)
    print(f"    cosines between plane normals {g['cos']}")
    assert g["nb"] == [4, 4, 4] and g["rng"] == [1, 1, 1]
    assert abs(g["cos"].max() / cos - 1.0) < 1e-3
    if cos != 1e-10:
        assert g["ortho"] == (cos < 1e-10)
    marked = {t for t, _ in e["marked"]}
    near = L.near_rc(frame, rc)
    assert {t[:5] for t in near} == marked and len(marked) == 60
    got = L.triples(*nl)
    for t in near:
        assert -2e-10 * rc < t[5] < -0.5e-10 * rc and t[:5] in got, t
    # the corner pairs sit in bins diagonal to each other: all three plane gaps count
    b = L.bins_of(frame, rc)
    for a in range(e["corner_pairs"]):
        d = (b[a] - b[30 + a]) % 4
        assert np.all((d == 1) | (d == 3)), (a, b[a], b[30 + a])


@pytest.mark.parametrize("turn", range(4))
@pytest.mark.parametrize("kind", sorted(L.FACE_CELLS))
def test_face_frames(kind, turn):
    e = L.face_frame(kind, turn)
    frame, rc = e["frame"], e["rc"]
    nl = _lists(frame, rc)
    g, _ = _report(f"faces {kind} turn {turn}", frame, rc, nl)
    frac = e["frac"]
    n = len(frac)
    assert n == g["nbins"] == (64 if kind == "ortho" else 27) and tuple(frac[0]) == (L.FACE_REPS[turn],) * 3
    for k in range(3):
        assert set(L.FACE_REPS) <= set(frac[:, k].tolist())
        assert set(frac[:, k].tolist()) <= set(L.FACE_REPS) | {c / g["nb"][k] for c in range(1, g["nb"][k])}
    # no two of them on one lattice point
    d = (frac[:, None] - frac[None]) - np.rint(frac[:, None] - frac[None])
    assert (np.abs(d).max(axis=2) + np.eye(n) > 0.1).all()
    got = L.triples(*nl)
    assert len(e["marked"]) == 4 * n
    for t, listed in e["marked"]:
        r = L.distance(frame, t)
        assert listed and abs(r - L.FACE_DIST) < 1e-12 and t in got, (t, r)
    assert all(abs(t[5]) > 1e-9 for t in L.near_rc(frame, rc, 1e-6))


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("kind", sorted(L.FACE_CELLS))
def test_cutoff_frames(kind, sign):
    e = L.cutoff_frame(kind, sign)
    frame, rc = e["frame"], e["rc"]
    nl = _lists(frame, rc)
    _report(f"cut-off {kind} sign {sign:+d}", frame, rc, nl)
    _check_marked(e, nl, sign)
    # how many cells each atom of a pair is wrapped by: the same, one apart along one direction, one apart along all three
    w = np.floor(frame[1][:8] @ np.linalg.inv(frame[2])).astype(int)
    dw = np.abs(w[:4] - w[4:])
    assert dw[0].tolist() == [0, 0, 0] and dw[1].tolist() == [1, 0, 0] and dw[2].tolist() == [1, 1, 1] and dw[3].tolist() == [0, 0, 0]
    b = L.bins_of(frame, rc)
    assert np.all(b[3] != b[7])                # ... and across a corner of the bin grid


@pytest.mark.parametrize("sign", [-1, 1])
def test_self_image_frames(sign):
    e = L.self_image_frame(sign)
    nl = _lists(e["frame"], e["rc"])
    g, _ = _report(f"self image sign {sign:+d}", e["frame"], e["rc"], nl)
    assert g["nb"][0] == 1 and g["rng"][0] == (2 if sign < 0 else 1)
    _check_marked(e, nl, sign)
    assert len(nl[1]) == (12 if sign < 0 else 0)


def _check_marked(e, nl, sign):
    """Every marked pair is rc (1 + sign 1e-10) long in extended precision, on the side `listed` says, the oracle lists it
    accordingly, and nothing else of the frame is within 1e-6 A of rc."""
    frame, rc = e["frame"], e["rc"]
    got = L.triples(*nl)
    for t, listed in e["marked"]:
        r = L.distance(frame, t)
        assert abs((r - rc) / rc - sign * 1e-10) < 1e-13, (t, r)
        assert listed == (sign < 0) == (t in got) == (LD(r) < LD(rc)), (t, r)
    assert {t[:5] for t in L.near_rc(frame, rc)} == {t for t, _ in e["marked"]}


@pytest.mark.parametrize("name,skin", L.PRUNE_CASES)
def test_prune_frames_hold_pairs_a_euclidean_bound_would_drop(name, skin):
    """Every marked pair is closer than rc, its atoms sit in bins one apart along two or three directions of the grid made
    for rc + skin, the Euclidean norm of the plane gaps from the first atom to the second's bin exceeds rc + skin, and no
    single gap reaches rc: a sweep that took the Euclidean bound in this cell would not look into that bin."""
    for variant in L.VARIANTS:
        e = L.prune_frame(name, variant, skin)
        frame, rc, n = e["frame"], e["rc"], e["pairs"]
        nl = _lists(frame, rc)
        g = L.grid_of(frame[2], frame[3], rc + skin)
        print(f"{L.describe(f'prune {name} {variant} skin {skin}', frame)}: {n} pairs, nb {g['nb']}, ortho {g['ortho']}")
        assert g["ortho"] == 0 and n >= 3 and (skin > 0 or n == 16)
        got = L.triples(*nl)
        for a in range(n):
            o, gaps = L.plane_gaps(frame, rc + skin, a, n + a)
            assert np.count_nonzero(o) >= 2 and (gaps ** 2).sum() > (rc + skin) ** 2 * (1 + 1e-6) and gaps.max() < rc
        for t, listed in e["marked"]:
            assert listed and t in got and 0.96 * rc < L.distance(frame, t) < 0.9995 * rc
        assert L.gap_to_rc(frame, rc) > 1e-6
