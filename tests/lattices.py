"""Frames for the geometry tests of the device neighbour list (test_lattices_cpu.py proves their properties with the oracle
alone, test_hip_list_geometry.py hands them to the library): sheared, rotated and left-handed cells large enough for a bin
grid of three to five bins per edge, atoms up to four cells outside, and the exact maps between the lists of one crystal in
two descriptions.  Plain numpy.

A frame is the tuple (numbers, pos, cell, pbc).  A list is (ptr, j, off) as oracle.neighbors returns it: for atom i the
entries ptr[i] .. ptr[i + 1] - 1, ordered by (j, off lexicographic); pair rule |pos[j] + off @ cell - pos[i]| < rc."""
import numpy as np

RC = 3.0
SKIN = 0.5              # the library's default skin: its candidates, and its bin grid, are made for rc + skin
DENSITY = 0.03          # atoms per cubic Angstrom of the list-only frames
SPECIES = [3, 16]

# name: (a, b, c, alpha, beta, gamma).  Every periodic height gives three to five bins at rc = 3 (test_lattices_cpu.py).
FAMILIES = {
    "hex120": (14.0, 14.0, 13.0, 90.0, 90.0, 120.0),
    "hex60": (14.0, 14.0, 13.0, 90.0, 90.0, 60.0),
    "rhombo60": (17.0, 17.0, 17.0, 60.0, 60.0, 60.0),
    "bccprim": (15.0, 15.0, 15.0, 109.4712, 109.4712, 109.4712),
    "mono130": (13.0, 10.0, 17.0, 90.0, 130.0, 90.0),
    "triclinic": (15.0, 16.0, 19.0, 62.0, 71.0, 118.0),
    "flat150": (25.0, 25.0, 10.0, 90.0, 90.0, 150.0),
}
VARIANTS = ("given", "rotated", "left")
PBC_ATOMS = 150        # atoms of the frames run under all eight periodicity patterns (sparse along the open directions)
PBCS = [(bool(k & 4), bool(k & 2), bool(k & 1)) for k in range(8)]


def rotation(seed):
    """A seeded random proper rotation (Q of a normal matrix, columns signed so that Q is unique and det Q = +1)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def cell_from(a, b, c, alpha, beta, gamma, rotate=None, left=False):
    """Rows = cell vectors of lengths a, b, c with angles alpha (b, c), beta (a, c), gamma (a, b) in degrees: a along x, b in
    the xy plane, right-handed.  rotate = seed: the cell turned rigidly by rotation(seed); left: the first two vectors
    swapped (the same lattice with det < 0)."""
    ca, cb, cg = (np.cos(np.radians(x)) for x in (alpha, beta, gamma))
    sg = np.sin(np.radians(gamma))
    cy = (ca - cb * cg) / sg
    cell = np.array([[a, 0.0, 0.0], [b * cg, b * sg, 0.0], [c * cb, c * cy, c * np.sqrt(1.0 - cb * cb - cy * cy)]])
    if rotate is not None:
        cell = cell @ rotation(rotate)
    if left:
        cell = cell[[1, 0, 2]]
    return cell


def grid_of(cell, pbc, rc):
    """The host statement of nl_make_grid's rule (nl_grid.inc) for a cell without zero vectors: plane normals by cross
    products, heights V / |normal|, nb = floor(height / rc) in 1 .. 16 and rng = ceil(rc nb / height) along periodic
    directions (1 and 0 along open ones), ortho = every squared cosine between two plane normals below 1e-20.  The same
    operations in the same order in float64; the device may contract a product and a sum into one rounding, so at a height
    of k rc to the last bit the two may land on different sides — `ratio` = height / rc says how close a frame is.
    The device makes its grid for the cut-off of the CANDIDATES, rc + skin (neighbor.hip: launch_neighbor_bin): `rc` here is
    the model's cut-off for a handle with skin 0, and 0.5 A more (SKIN) for a handle with the default skin."""
    h = np.asarray(cell, float).reshape(3, 3)
    p, q, r = h
    bc, ca, ab = np.cross(q, r), np.cross(r, p), np.cross(p, q)
    V = abs(float(np.dot(p, bc)))
    nrm = [bc, ca, ab]
    n2 = [float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) for v in nrm]
    hgt = np.array([V / np.sqrt(x) for x in n2])
    nb, rng = [], []
    for k in range(3):
        if pbc[k]:
            n = min(max(int(np.floor(hgt[k] / rc)), 1), 16)
            nb.append(n)
            rng.append(int(np.ceil(rc * n / hgt[k])))
        else:
            nb.append(1)
            rng.append(0)
    cos2 = [float(np.dot(nrm[a], nrm[b])) ** 2 / (n2[a] * n2[b]) for a, b in ((0, 1), (0, 2), (1, 2))]
    return dict(hgt=hgt, ratio=hgt / rc, nb=nb, rng=rng, ortho=int(all(x < 1e-20 for x in cos2)), cos=np.sqrt(cos2),
                det=float(np.linalg.det(h)), nbins=nb[0] * nb[1] * nb[2])


def family(name, variant="given", pbc=(True, True, True), seed=0, natoms=None, spread=(-3.5, 4.5)):
    """One crystal per (name, seed), described three ways.  50 to 150 atoms at DENSITY, fractional coordinates uniform in
    `spread` — up to four cells outside, each atom by its own amount — along every direction (periodic or not).  "rotated"
    turns cell and positions by one rotation; "left" swaps the first two cell vectors (and the periodicity flags with
    them) and leaves the positions: the lists map onto the given frame's by variant_map()."""
    prm = FAMILIES[name]
    cell = cell_from(*prm)
    rng = np.random.default_rng([seed, sorted(FAMILIES).index(name)])
    n = int(np.clip(round(DENSITY * abs(np.linalg.det(cell))), 50, 150)) if natoms is None else natoms
    frac = rng.uniform(spread[0], spread[1], size=(n, 3))
    numbers = rng.choice(SPECIES, size=n).astype(np.int32)
    numbers[:2] = SPECIES               # (both slots occupied whatever the draw)
    pos = frac @ cell
    pbc = tuple(bool(x) for x in pbc)
    if variant == "rotated":
        R = rotation(17 + seed)
        cell, pos = cell @ R, pos @ R
    elif variant == "left":
        cell, pbc = cell[[1, 0, 2]], (pbc[1], pbc[0], pbc[2])
    elif variant != "given":
        raise ValueError(variant)
    return numbers, pos, cell, pbc


def variant_map(nl, variant):
    """The list of family(name, variant) from the list of family(name, "given"): a rotation changes nothing, the left-handed
    twin lists every pair under the image triple with its first two components swapped."""
    if variant != "left":
        return nl
    return sort_list(nl[0], nl[1], nl[2][:, [1, 0, 2]])


def sort_list(ptr, j, off):
    """A list in the oracle's order: within an atom by (j, off lexicographic)."""
    ptr, j, off = np.asarray(ptr, np.int64), np.asarray(j, np.int32), np.asarray(off, np.int32).reshape(-1, 3)
    i = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    order = np.lexsort((off[:, 2], off[:, 1], off[:, 0], j, i))
    return ptr, j[order], off[order]


def relabel(frame, n, nl):
    """Atom i moved by the integer lattice vector n[i] @ cell (n: [N, 3] integers, zero along open directions).  Returns the
    frame and the exact list it must have, from the list `nl` of the frame as it was: the image of j that i sees moves with
    both, pos[j] + n[j] @ cell + off' @ cell - pos[i] - n[i] @ cell is the old displacement when off' = off + n[i] - n[j].
    The shift depends on (i, j) only, so the order within an atom's list stays."""
    numbers, pos, cell, pbc = frame
    n = np.asarray(n, np.int64).reshape(len(numbers), 3)
    assert not n[:, [not p for p in pbc]].any()
    ptr, j, off = nl
    i = np.repeat(np.arange(len(numbers)), np.diff(ptr))
    return (numbers, pos + n.astype(float) @ cell, cell, pbc), (ptr, j, (off + n[i] - n[j]).astype(np.int32))


SHEAR = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 1]])


def reshear(frame, U):
    """The same crystal in the cell U @ cell, U an integer matrix with |det U| = 1; positions unchanged, all directions
    periodic.  Returns the frame and T with off' = off @ T (T = U^-1, integers): off @ cell = off' @ (U @ cell)."""
    numbers, pos, cell, pbc = frame
    U = np.asarray(U, np.int64).reshape(3, 3)
    T = np.rint(np.linalg.inv(U)).astype(np.int64)
    assert all(pbc) and np.array_equal(U @ T, np.eye(3, dtype=np.int64))
    return (numbers, pos, U.astype(float) @ cell, pbc), T


def map_triples(nl, T):
    """The list of reshear's frame from the list of the frame it was made of."""
    ptr, j, off = nl
    return sort_list(ptr, j, np.asarray(off, np.int64) @ T)


def triples(ptr, j, off):
    i = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return set(map(tuple, np.column_stack([i, j, np.asarray(off).reshape(-1, 3)]).tolist()))


def distance(frame, t):
    """|pos[j] + off @ cell - pos[i]| of the triple t = (i, j, o0, o1, o2), in extended precision."""
    _, pos, cell, _ = frame
    LD = np.longdouble
    d = pos[t[1]].astype(LD) + np.array(t[2:], LD) @ cell.astype(LD) - pos[t[0]].astype(LD)
    return float(np.sqrt((d * d).sum()))


def gap_to_rc(frame, rc, nb=None):
    """Smallest | |r| - rc | over the pairs within rc + 0.5 (by the oracle's linked cells), in extended precision."""
    from oracle import oracle as orc
    _, pos, cell, pbc = frame
    ptr, j, off = orc.neighbors_cells(pos, cell, pbc, rc + 0.5)
    if len(j) == 0:
        return np.inf
    LD = np.longdouble
    i = np.repeat(np.arange(len(pos)), np.diff(ptr))
    d = pos[j].astype(LD) + off.astype(LD) @ cell.astype(LD) - pos[i].astype(LD)
    return float(np.abs(np.sqrt((d * d).sum(axis=1)) - LD(rc)).min())


def describe(label, frame, pbc=None):
    """'frame, handedness, pbc pattern' for a failure message."""
    _, _, cell, p = frame
    return f"{label} [{'left' if np.linalg.det(cell) < 0 else 'right'}-handed, pbc {''.join('FT'[int(x)] for x in p)}]"


def list_diff(label, frame, got, want):
    """None if the two lists hold the same triples, else a message naming the frame, its handedness and pbc pattern and the
    first missing and the first extra (i, j, off) with its distance."""
    a, b = triples(*got), triples(*want)
    if a == b:
        return None
    msg = describe(label, frame) + f": {len(b - a)} missing, {len(a - b)} extra"
    for word, s in (("missing", b - a), ("extra", a - b)):
        if s:
            t = min(s)
            msg += f"; first {word} (i, j, off) = ({t[0]}, {t[1]}, {t[2:]}) at {distance(frame, t):.12f} A"
    return msg


# ---------------------------------------------------------------------------- the frame of the physics and walk cases
PHYS = dict(name="triclinic", natoms=120, dmin=1.4, m=12, rc=RC, eta=4.0, seed=5)


def push_apart(frame, dmin):
    """Close pairs pushed apart until none is left within dmin, as test_hip_paths.random_frame does."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc = frame
    pos = pos.copy()
    for _ in range(300):
        ptr, j, off = orc.neighbors(pos, cell, pbc, dmin)
        if len(j) == 0:
            break
        i = np.repeat(np.arange(len(numbers)), np.diff(ptr))
        d = pos[j] - pos[i] + off.astype(float) @ cell
        np.add.at(pos, i, -0.2 * d / np.linalg.norm(d, axis=1, keepdims=True))
    return numbers, pos, cell, pbc


def physics_frame():
    """Two species, 120 atoms in the reduced triclinic cell (inside it), at least 1.4 A apart."""
    return push_apart(family(PHYS["name"], natoms=PHYS["natoms"], seed=PHYS["seed"], spread=(0.0, 1.0)), PHYS["dmin"])


def physics_twins():
    """{label: (frame, map)}: the physics frame, its reshear by SHEAR and SHEAR squared, its left-handed and its rotated
    twin.  map(list of the reduced frame) is the twin's list; "rotated" carries the rotation its forces turn by."""
    base = physics_frame()
    numbers, pos, cell, pbc = base
    out = {"reduced": (base, lambda nl: nl, None)}
    for label, U in (("shear", SHEAR), ("shear2", SHEAR @ SHEAR)):
        fr, T = reshear(base, U)
        out[label] = (fr, (lambda nl, T=T: map_triples(nl, T)), None)
    fr, T = reshear(base, [[0, 1, 0], [1, 0, 0], [0, 0, 1]])
    out["left"] = (fr, (lambda nl, T=T: map_triples(nl, T)), None)
    R = rotation(23)
    out["rotated"] = ((numbers, pos @ R, cell @ R, pbc), lambda nl: nl, R)
    return out


def cell_angles(cell):
    a, b, c = cell
    ang = lambda u, v: float(np.degrees(np.arccos(np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v))))
    return ang(b, c), ang(a, c), ang(a, b)


def physics_inducing(frame, rc, m, seed=2):
    """m environments of the frame with a little noise (as test_hip_paths.build draws them), as (number, species, r)."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc = frame
    rng = np.random.default_rng(seed)
    ptr, j, off = orc.neighbors(pos, cell, pbc, rc)
    out = []
    for a in rng.choice(len(numbers), size=m, replace=False):
        s = slice(ptr[a], ptr[a + 1])
        r = pos[j[s]] - pos[a] + off[s].astype(float) @ cell + 0.03 * rng.normal(size=(ptr[a + 1] - ptr[a], 3))
        keep = np.linalg.norm(r, axis=1) < rc - 1e-3
        out.append((int(numbers[a]), numbers[j[s]][keep], r[keep]))
    return out


# ---------------------------------------------------------------------------- the walk of the reuse and MD cases
WALK = dict(name="rhombo60", seed=3, steps=12, sigma=0.03, carried=0, carry_step=7)


def walk_frames():
    """The left-handed rhombohedral family cell, its atoms at least 1.4 A apart (the MD case integrates them) and then moved
    up to four cells outside, each by its own lattice vector; and a walk of 12 steps, every atom moving 0.03 A in a random
    direction per step (test_lattices_cpu.py: no atom drifts 0.24 A from its start, so a skin of 0.5 A keeps the candidates);
    from step `carry_step` on atom `carried` sits one full lattice vector further, through a face."""
    numbers, pos, cell, pbc = push_apart(family(WALK["name"], "left", seed=WALK["seed"], spread=(0.0, 1.0)), PHYS["dmin"])
    rng = np.random.default_rng(41)
    pos = pos + rng.integers(-4, 5, size=pos.shape).astype(float) @ cell
    frames, p = [], pos.copy()
    for step in range(WALK["steps"]):
        if step:
            u = rng.normal(size=pos.shape)
            p = p + WALK["sigma"] * u / np.linalg.norm(u, axis=1, keepdims=True)
        if step == WALK["carry_step"]:
            p[WALK["carried"]] += cell[1]
        frames.append(p.copy())
    return (numbers, pos, cell, pbc), frames


# ---------------------------------------------------------------------------- a cell thinner than the cut-off
THIN = dict(cell=(2.9, 12.0, 13.0, 75.0, 80.0, 70.0), natoms=20, seed=9)


def thin_frame():
    """Twenty atoms of two species, at least 1.4 A apart, in a sheared cell whose first vector is 2.9 A long: the height along it
    lies between 0.8 RC and RC (test_accumulator_geometry_cpu.py), so every atom's own images at +- that vector stand in its
    list at RC."""
    cell = cell_from(*THIN["cell"])
    rng = np.random.default_rng(THIN["seed"])
    n = THIN["natoms"]
    numbers = np.array(SPECIES * (n // 2), np.int32)
    return push_apart((numbers, rng.random((n, 3)) @ cell, cell, (True, True, True)), PHYS["dmin"])


# ---------------------------------------------------------------------------- constructed edges
# Each returns dict(frame=, rc=, marked=[((i, j, o0, o1, o2), listed)], ...): `marked` are the pairs the frame was built
# for, with whether the list must hold them.
def bins_of(frame, rc):
    """[N, 3] bin indices by nl_place_axis's rule on grid_of's grid (host float64)."""
    _, pos, cell, pbc = frame
    g = grid_of(cell, pbc, rc)
    fr = pos @ np.linalg.inv(cell)
    fr = fr - np.floor(fr)
    b = np.clip((fr * np.array(g["nb"])).astype(int), 0, np.array(g["nb"]) - 1)
    return np.where(np.array(pbc), b, 0)


def unit(rng, n, lo=0.0):
    """n random unit vectors whose components are all at least `lo` in size."""
    out = []
    while len(out) < n:
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if np.abs(u).min() >= lo:
            out.append(u)
    return np.array(out)


def with_partners(rng, cell, n, lo, hi):
    """n atoms uniform in the cell and a partner for each at a distance uniform in [lo, hi), any direction: every atom has a
    neighbour, many of them in another bin."""
    a = rng.random((n, 3)) @ cell
    return np.vstack([a, a + unit(rng, n) * rng.uniform(lo, hi, size=(n, 1))])


def scaled_to_height(cell, axis, target):
    """The cell times one factor, chosen so that grid_of's height along `axis` is `target` (or the nearest value a factor
    reaches: the factor is walked ulp by ulp).  Returns (cell, the height reached)."""
    cell = np.asarray(cell, float)
    pbc = (True, True, True)
    s = target / grid_of(cell, pbc, 1.0)["hgt"][axis]
    best = None
    for _ in range(64):
        h = grid_of(cell * s, pbc, 1.0)["hgt"][axis]
        if best is None or abs(h - target) < abs(best[0] - target):
            best = (h, s)
        if h == target:
            break
        s = np.nextafter(s, np.inf if h < target else -np.inf)
    return cell * best[1], best[0]


GRID_EDGES = [(kind, k, side) for kind in ("ortho", "sheared") for k in (3, 16, 17) for side in (-1, 0, 1)]


def grid_edge(kind, k, side):
    """A cell whose height along its first vector is k rc (1 + side 2^-50): floor(height / rc) decides nb by an ulp.  k = 3
    at rc = 3 with 80 atoms; k = 16 and 17 at rc = 2 with 400 sparse atoms: 16 bins per edge (the cap) and the whole 4096-bin
    table.  The other two heights are 7 and 13 % longer."""
    rc = 3.0 if k == 3 else 2.0
    target = k * rc * (1.0 + side * 2.0 ** -50)
    base = np.diag([1.0, 1.07, 1.13]) if kind == "ortho" else cell_from(1.0, 1.12, 1.2, 78.0, 81.0, 74.0)
    cell, reached = scaled_to_height(base, 0, target)
    rng = np.random.default_rng([k, side + 1, kind == "ortho"])
    n = 40 if k == 3 else 200
    pos = with_partners(rng, cell, n, 0.4 * rc, 0.98 * rc)
    numbers = rng.choice(SPECIES, size=2 * n).astype(np.int32)
    numbers[:2] = SPECIES
    return dict(frame=(numbers, pos, cell, (True, True, True)), rc=rc, target=target, reached=reached, marked=[])


ORTHO_COS = (1e-12, 1e-11, 1e-10, 1e-9, 1e-6)
ORTHO_RC = 2.9    # four bins of exactly 3 A per 12 A edge whichever way a height of 12 (1 - 1e-12) rounds


def ortho_edge(cos):
    """The cubic 12 A cell with its third vector tilted towards the first, so that the cosine between two plane normals is
    `cos`: nl_make_grid calls the cell orthogonal below 1e-10 and bounds the distance to a bin by the Euclidean norm of the
    three plane gaps, otherwise by the largest.  Marked pairs at rc (1 - 1e-10) across bin corners, edges and faces: atom A
    sits rc (1 - 2e-10) from a corner of the grid, B 1e-10 rc beyond the corner on the same line, inside the bin diagonal to
    A's — with no skin the bin whose Euclidean bound is the first to reach the cut-off.  40 more atoms with partners."""
    rc = ORTHO_RC
    cell = np.array([[12.0, 0.0, 0.0], [0.0, 12.0, 0.0], [12.0 * cos, 0.0, 12.0]])
    rng = np.random.default_rng(77)
    corners = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    corners = corners[rng.permutation(len(corners))[:30]]
    u = unit(rng, 30, lo=0.3) * rng.choice([-1.0, 1.0], size=(30, 3))
    u[20:25, 0] = 0.0                    # across an edge of the grid: two gaps
    u[25:30, :2] = 0.0                   # across a face: one gap
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = (corners / 4.0) @ cell
    A, B = c - rc * (1.0 - 2e-10) * u, c + rc * 1e-10 * u
    pos = np.vstack([A, B, with_partners(rng, cell, 20, 0.4 * rc, 0.9 * rc)])
    numbers = rng.choice(SPECIES, size=len(pos)).astype(np.int32)
    numbers[:2] = SPECIES
    frame = (numbers, pos, cell, (True, True, True))
    return dict(frame=frame, rc=rc, marked=[(t, True) for t in _triples_of(frame, np.arange(30), np.arange(30, 60))],
                corner_pairs=20)


def _triples_of(frame, ia, ib):
    """(i, j, off) and (j, i, -off) of the pairs (ia[k], ib[k]) under the nearest image."""
    _, pos, cell, pbc = frame
    out = []
    for a, b in zip(ia, ib):
        f = (pos[b] - pos[a]) @ np.linalg.inv(cell)
        o = np.where(np.array(pbc), -np.rint(f), 0).astype(int)
        out += [(int(a), int(b), int(o[0]), int(o[1]), int(o[2])), (int(b), int(a), int(-o[0]), int(-o[1]), int(-o[2]))]
    return out


FACE_REPS = (0.0, 1.0, -2.0 ** -60, 1.0 - 2.0 ** -53)
FACE_CELLS = {"ortho": np.diag([12.5, 13.0, 14.0]), "sheared": cell_from(*FAMILIES["triclinic"])}
FACE_DIST = RC - 1e-5


def face_frame(kind, turn):
    """Atoms whose three fractional coordinates are each on a face of the grid: a cell face (0, 1, -2^-60 or 1 - 2^-53,
    all the same plane of the crystal) or k / nb, k = 1 .. nb - 1 — every combination of the nb planes per axis once (64
    atoms in the orthogonal cell, 27 in the sheared one), no
    two atoms on one lattice point.  Which of the four spellings of the cell face an atom takes turns with `turn` (0 .. 3)
    and from atom to atom; the first atom takes the same one on all three axes: (0, 0, 0), (1, 1, 1), ...  Two partners per atom, rc - 1e-5 away on
    either side along a random direction."""
    cell = FACE_CELLS[kind]
    nb = grid_of(cell, (True, True, True), RC)["nb"]
    rng = np.random.default_rng(5 + turn)
    frac = []
    for cls in np.stack(np.meshgrid(*[np.arange(n) for n in nb], indexing="ij"), -1).reshape(-1, 3):
        frac.append([FACE_REPS[(turn + (1, 3, 1)[k] * int(cls.sum())) % 4] if c == 0 else c / nb[k] for k, c in enumerate(cls)])
    frac = np.array(frac)
    a = frac @ cell
    u = unit(rng, len(a), lo=0.2) * rng.choice([-1.0, 1.0], size=(len(a), 3))
    pos = np.vstack([a, a + FACE_DIST * u, a - FACE_DIST * u])
    numbers = rng.choice(SPECIES, size=len(pos)).astype(np.int32)
    numbers[:2] = SPECIES
    frame = (numbers, pos, cell, (True, True, True))
    n = len(a)
    marked = _triples_of(frame, np.r_[:n, :n], np.r_[n:2 * n, 2 * n:3 * n])
    return dict(frame=frame, rc=RC, frac=frac, marked=[(t, True) for t in marked])


def cutoff_frame(kind, sign):
    """Pairs at rc (1 + sign 1e-10): inside one cell image, across one cell face, across the cell's corner (image (1, 1, 1))
    and across a corner of the bin grid, plus 30 atoms with partners.  sign = -1: listed; +1: not."""
    cell = FACE_CELLS[kind]
    nb = np.array(grid_of(cell, (True, True, True), RC)["nb"])
    rng = np.random.default_rng(13)
    centres = np.array([[0.4, 0.45, 0.55], [0.0, 0.5, 0.25], [0.0, 0.0, 0.0], np.array([1, 2, 1]) / nb]) @ cell
    u = unit(rng, 4, lo=0.3)
    d = RC * (1.0 + sign * 1e-10)
    pos = np.vstack([centres - 0.5 * d * u, centres + 0.5 * d * u, with_partners(rng, cell, 15, 0.4 * RC, 0.9 * RC)])
    numbers = rng.choice(SPECIES, size=len(pos)).astype(np.int32)
    numbers[:2] = SPECIES
    frame = (numbers, pos, cell, (True, True, True))
    return dict(frame=frame, rc=RC, marked=[(t, sign < 0) for t in _triples_of(frame, np.arange(4), np.arange(4, 8))])


def self_image_frame(sign):
    """A cell whose first edge is rc (1 + sign 1e-10), the others 12.5 and 13 A: every atom is rc (1 + sign 1e-10) from its
    own image (+-1, 0, 0).  Six atoms more than rc apart in the plane of the long edges."""
    cell = np.diag([RC * (1.0 + sign * 1e-10), 12.5, 13.0])
    frac = np.array([[0.1, 0.1, 0.1], [0.6, 0.45, 0.15], [0.3, 0.8, 0.2], [0.9, 0.15, 0.6], [0.2, 0.5, 0.65], [0.5, 0.85, 0.7]])
    pos = frac @ cell
    numbers = np.array(SPECIES * 3, np.int32)
    marked = [((i, i, s, 0, 0), sign < 0) for i in range(6) for s in (-1, 1)]
    return dict(frame=(numbers, pos, cell, (True, True, True)), rc=RC, marked=marked)


def near_rc(frame, rc, width=1e-6):
    """The triples (i, j, o0, o1, o2, |r| - rc) of all pairs within `width` of rc, distances in extended precision."""
    from oracle import oracle as orc
    _, pos, cell, pbc = frame
    ptr, j, off = orc.neighbors_cells(pos, cell, pbc, rc + 0.5)
    LD = np.longdouble
    i = np.repeat(np.arange(len(pos)), np.diff(ptr))
    d = pos[j].astype(LD) + off.astype(LD) @ cell.astype(LD) - pos[i].astype(LD)
    gap = np.sqrt((d * d).sum(axis=1)) - LD(rc)
    k = np.flatnonzero(np.abs(gap) < width)
    return [(int(i[t]), int(j[t]), int(off[t, 0]), int(off[t, 1]), int(off[t, 2]), float(gap[t])) for t in k]


def plane_gaps(frame, rc_grid, ia, ib):
    """What the sweep of nl_fwd_kernel knows of atom ib's bin when it builds atom ia's candidates (host float64): the bin
    offset o [3] from ia's bin to ib's (positions taken as they are, not wrapped: for pairs a bin apart) and the gaps [3]
    between ia and that bin along the three plane normals, in Angstrom.  The distance to the bin is at least the largest
    gap; only in an orthogonal cell is it at least the Euclidean norm of the three."""
    _, pos, cell, pbc = frame
    g = grid_of(cell, pbc, rc_grid)
    nb, w = np.array(g["nb"]), g["hgt"] / np.array(g["nb"])
    fa, fb = (pos[ia] @ np.linalg.inv(cell)) * nb, (pos[ib] @ np.linalg.inv(cell)) * nb
    o = (np.floor(fb) - np.floor(fa)).astype(int)
    tb = fa - np.floor(fa)
    return o, np.where(o > 0, o - tb, np.where(o < 0, tb - o - 1.0, 0.0)) * w


def prune_frame(name, variant, skin, want=16):
    """Pairs that a Euclidean bound on the distance to a bin would lose in a sheared cell: A and B less than rc apart on
    either side of a corner or an edge of the bin grid (the grid a handle with this skin makes: cut-off rc + skin), placed so
    that the Euclidean norm of A's plane gaps to B's bin EXCEEDS rc + skin — the bound the sweep takes in orthogonal cells —
    while each single gap, the bound it must take here, is below.  Up to `want` such pairs found by a seeded search, plus 20
    atoms with partners.  marked: all listed."""
    numbers, _, cell, pbc = family(name, variant)
    rl = RC + skin
    g = grid_of(cell, pbc, rl)
    nb = np.array(g["nb"])
    rng = np.random.default_rng([11, sorted(FAMILIES).index(name), int(skin > 0)])
    A, B = [], []
    for _ in range(8000):
        if len(A) == want:
            break
        c = (rng.integers(0, nb + 1) / nb) @ cell
        u = unit(rng, 1)[0]
        d = RC * rng.uniform(0.97, 0.999)
        s = rng.uniform(0.5, 0.98)
        a, b = c - s * d * u, c + (1.0 - s) * d * u
        o, gaps = plane_gaps((None, np.array([a, b]), cell, pbc), rl, 0, 1)
        if np.count_nonzero(o) >= 2 and np.abs(o).max() == 1 and (gaps ** 2).sum() > rl * rl * (1.0 + 1e-6) and gaps.max() < RC:
            A.append(a)
            B.append(b)
    n = len(A)
    pos = np.vstack(A + B + [with_partners(rng, cell, 10, 0.4 * RC, 0.9 * RC)]) if n else with_partners(rng, cell, 10, 0.4 * RC, 0.9 * RC)
    numbers = rng.choice(SPECIES, size=len(pos)).astype(np.int32)
    numbers[:2] = SPECIES
    frame = (numbers, pos, cell, pbc)
    return dict(frame=frame, rc=RC, pairs=n, marked=[(t, True) for t in _triples_of(frame, np.arange(n), np.arange(n, 2 * n))])


# (family, skin) with pairs to find.  With the default skin the bins of the hexagonal and rhombohedral cells are too wide
# against pairs of 3 A for more than a few (4 to 4.6 A: the search finds none to six).
PRUNE_CASES = [(name, skin) for skin in (0.0, SKIN) for name in sorted(FAMILIES)
               if skin == 0.0 or name not in ("hex120", "hex60", "rhombo60")]
