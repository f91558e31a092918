"""Frames whose neighbour-list lengths are exact, for the tests of the list / descriptor kernels at their size edges
(test_islands_cpu.py proves the lengths with the oracle alone, test_hip_list_edges.py runs the library on them).

A cubic periodic cell holds well-separated "islands": n atoms inside a ball whose diameter is just under the cut-off, on a
cubic grid whose pitch exceeds diameter + cut-off (+ skin).  Every atom of an island then has exactly n - 1 neighbours, and
no island sees another one or an image.  With the diameter just under rc + skin instead ("shell" islands) the CANDIDATE
counts are exact while the hit counts are lower and differ from atom to atom.

Every island holds every species of the table, and the whole frame is shifted by a fixed vector and wrapped back into the
cell, so that islands straddle the periodic boundaries (non-zero images in their lists)."""
import functools

import numpy as np

# the twelve elements autoforce_amd.workloads.MASS knows, so every table drawn from here can go through the MD loops
# (H first: its length unit is 0.5, every other one 1.0)
SPECIES = [1, 3, 8, 9, 11, 12, 14, 15, 16, 17, 40, 57]

SKIN = 0.5   # the library's default Verlet skin (option skin_milliangstrom = 500)

# frame A: list lengths {47, 48, 49, 63, 64, 65, 127, 128, 129}
A_SIZES = (48, 49, 50, 64, 65, 66, 128, 129, 130)
A = dict(rc=10.0, diameter=9.95, dmin=1.45, pitch=22.0, seed=1)
# frame B: list lengths {255, 256, 257} around the sortable part of a list (NL_SORT_MAX = 256)
B_SIZES = (256, 257, 258)
B = dict(rc=12.0, diameter=11.95, dmin=1.3, pitch=26.0, seed=2)
# shell islands: candidate counts {63, 64, 65, 127, 128, 129} at rc + skin = 10.5; the diameter leaves 0.06 A for the walk
# of shell_walk (every atom stays within 0.02 A of where it started, a pair distance changes by 0.04 A at the most).  The seed
# is one at which the 65-candidate island has atoms with 63 hits (one tile) and with 65 (two)
SHELL_SIZES = (64, 65, 66, 128, 129, 130)
SHELL = dict(rc=10.0, diameter=10.44, dmin=1.45, pitch=22.0, seed=6)


def _ball_points(rng, n, radius, dmin):
    """n points uniform in the ball, each at least dmin from the ones before it (rejection sampling)."""
    pts = np.empty((n, 3))
    k = 0
    for _ in range(200000):
        p = rng.uniform(-radius, radius, 3)
        if p @ p > radius * radius:
            continue
        if k and ((pts[:k] - p) ** 2).sum(1).min() < dmin * dmin:
            continue
        pts[k] = p
        k += 1
        if k == n:
            return pts
    raise RuntimeError(f"could not place {n} points at {dmin} A in a ball of radius {radius} A")


@functools.lru_cache(maxsize=None)
def _geometry(sizes, diameter, dmin, pitch, seed):
    """Positions (wrapped into the cell), island of every atom, cell edge: islands on the first len(sizes) sites of the
    smallest cubic grid that holds them (x fastest), atoms shuffled so that neighbouring atom numbers mix islands."""
    rng = np.random.default_rng(seed)
    g = 1
    while g ** 3 < len(sizes):
        g += 1
    L = g * pitch
    pos, isl = [], []
    for k, n in enumerate(sizes):
        centre = (np.array([k % g, (k // g) % g, k // (g * g)]) + 0.5) * pitch
        pos.append(centre + _ball_points(rng, n, 0.5 * diameter, dmin))
        isl.append(np.full(n, k))
    pos, isl = np.concatenate(pos), np.concatenate(isl)
    order = rng.permutation(len(pos))
    pos = (pos[order] + np.array([0.31, 0.47, 0.59]) * pitch) % L     # the islands of the last grid layers straddle the cell faces
    return pos, isl[order], L


def island_frame(sizes, rc, diameter, dmin, pitch, seed, species):
    """numbers, positions, cell, pbc, island_of_atom.  The positions depend on the seed alone, not on the species table.
    Inside an island the species go round the table from a start that differs by island, so every island holds every
    species (sizes >= len(species)) and the species-sorted order of the device mixes the islands."""
    assert pitch > diameter + rc + SKIN and diameter < rc + SKIN
    pos, isl, L = _geometry(tuple(sizes), diameter, dmin, pitch, seed)
    S = len(species)
    num = np.empty(len(pos), int)
    for k in range(len(sizes)):
        mine = np.flatnonzero(isl == k)
        num[mine] = (np.arange(len(mine)) + 5 * k) % S
    return np.asarray(species, np.int32)[num], pos.copy(), np.eye(3) * L, [True] * 3, isl.copy()


def frame_a(species, sizes=A_SIZES):
    return island_frame(sizes, species=species, **A)


def frame_b(species):
    return island_frame(B_SIZES, species=species, **B)


def shell_frame(species):
    return island_frame(SHELL_SIZES, species=species, **SHELL)


SHELL_STEPS, SHELL_REBUILD = 9, 4


def shell_walk(pos, cell, seed=4):
    """The positions of the reuse test, step by step: every atom within 0.02 A of its start (so a handle with the default skin
    keeps its candidates and every candidate count stays what it was), except that before step SHELL_REBUILD atom 0 is
    carried through the cell — the same geometry, and a rebuild."""
    rng = np.random.default_rng(seed)
    base = pos.copy()
    frames = []
    for step in range(SHELL_STEPS):
        if step == SHELL_REBUILD:
            base[0] = base[0] + cell[0]
        d = rng.normal(size=pos.shape)
        d *= (0.02 * rng.random(len(pos)) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        frames.append(base + (d if step else 0.0))
    return frames


def inducing(numbers, pos, cell, pbc, rc, m, seed):
    """m environments cut from the frame (the species of the frame in turn, atoms drawn at random: every species has one as
    long as m >= the number of species) and rattled by 0.03 A, in the style of test_hip_paths.build."""
    from autoforce_amd import Local
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    ptr, j, off = orc.neighbors_cells(pos, cell, pbc, rc)
    zs = np.unique(numbers)
    taken, X = set(), []
    for q in range(m):
        pool = [a for a in np.flatnonzero(numbers == zs[q % len(zs)]) if a not in taken]
        a = int(rng.choice(pool))
        taken.add(a)
        s = slice(ptr[a], ptr[a + 1])
        r = pos[j[s]] - pos[a] + off[s].astype(float) @ cell + 0.03 * rng.normal(size=(ptr[a + 1] - ptr[a], 3))
        keep = np.linalg.norm(r, axis=1) < rc - 1e-3
        X.append(Local(int(numbers[a]), numbers[j[s]][keep], r[keep]))
    return X


def inducing_arrays(X):
    """ind_z, ind_ptr, neighbour species, neighbour vectors: what oracle.inducing_descriptors takes."""
    ind_z = np.array([x.number for x in X], np.int32)
    ind_ptr = np.concatenate([[0], np.cumsum([len(x._b) for x in X])])
    return ind_z, ind_ptr, np.concatenate([x._b for x in X]), np.concatenate([x._r for x in X])


# one case per instantiation that the library's dispatch on (lmax, nmax, species slots) can select: (lmax, nmax, species)
FORMS = ([(3, 3, s) for s in (1, 2, 3, 4, 6, 12)] + [(l, l, s) for l in (2, 4) for s in (2, 4, 6)] +
         [(l, n, s) for l, n in ((2, 3), (2, 4), (3, 2), (3, 4), (4, 2), (4, 3)) for s in (3, 6)])
SPREAD_FORMS = [(3, 3, 3), (4, 4, 2), (2, 2, 6), (3, 3, 12)]          # the sharded form and the training rows
ROWS16_SIZES = [(48, 49, 64), (48, 49, 64, 65), (48, 49, 64, 65, 66)]  # longest list 63, 64, 65
MD_SIZES = (49, 65, 129)
MD_FORMS = [(4, 4, 2), (2, 2, 6), (3, 3, 12)]
