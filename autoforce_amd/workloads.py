"""Synthetic workloads of BASELINE.json (recipes: SURVEY.md §8d).  Host-side numpy only.

The reference ships no structure files for these systems, so frames are generated from fixed
seeds: simple-cubic sites, shuffled species, Gaussian rattle with a minimum-distance rejection.
"""
import numpy as np

from .model import Local


def _rattled_lattice(shape, spacing, sigma, rng, dmin=1.6):
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3) * spacing
    pos = g.astype(float)
    cell = np.diag([n * spacing for n in shape]).astype(float)
    # rattle with rejection: a displacement is redrawn until no lattice neighbour (pre-rattle
    # distance = spacing) can come closer than dmin; cheap sufficient test per atom
    out = np.empty_like(pos)
    lim = (spacing - dmin) / 2.0
    for i in range(len(pos)):
        while True:
            d = sigma * rng.normal(size=3)
            if np.linalg.norm(d) <= lim:
                break
        out[i] = pos[i] + d
    return out, cell


def lips(n_side=16, seed=0, sigma=0.15):
    """C3/C4: "LiPS" 16^3 = 4096 simple-cubic sites, 2.72 A, 1536 Li / 512 P / 2048 S."""
    rng = np.random.default_rng(seed)
    dims = tuple(n_side) if np.ndim(n_side) else (n_side,) * 3  # (32, 32, 16): the 16384 atoms of config 5
    N = int(np.prod(dims))
    nLi, nP = 3 * N // 8, N // 8
    numbers = rng.permutation(np.array([3] * nLi + [15] * nP + [16] * (N - nLi - nP))).astype(np.int32)
    pos, cell = _rattled_lattice(dims, 2.72, sigma, rng)
    return numbers, pos, cell, np.array([True, True, True])


def si_diamond(reps=(2, 2, 1), seed=0, sigma=0.05):
    """C1: diamond Si a=5.431, 8-atom cubic x (2,2,1) = 32 atoms; L_z = 5.431 < rc: atoms meet their own images."""
    rng = np.random.default_rng(seed)
    a = 5.431
    base = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75],
                     [.75, .25, .75], [.75, .75, .25]]) * a
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in reps], indexing="ij"), -1).reshape(-1, 3) * a
    pos = (cells[:, None, :] + base[None]).reshape(-1, 3) + sigma * rng.normal(size=(len(cells) * 8, 3))
    cell = np.diag([n * a for n in reps]).astype(float)
    return np.full(len(pos), 14, np.int32), pos, cell, np.array([True, True, True])


def li_bcc(reps=(8, 4, 4), seed=0, sigma=0.10):
    """C2: bcc Li a=3.49, 2-atom cubic x reps = 256 atoms."""
    rng = np.random.default_rng(seed)
    a = 3.49
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]]) * a
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in reps], indexing="ij"), -1).reshape(-1, 3) * a
    pos = (cells[:, None, :] + base[None]).reshape(-1, 3) + sigma * rng.normal(size=(len(cells) * 2, 3))
    cell = np.diag([n * a for n in reps]).astype(float)
    return np.full(len(pos), 3, np.int32), pos, cell, np.array([True, True, True])


def oxide(shape=(32, 32, 16), seed=0, sigma=0.15):
    """C5: 16384 sites, 4 species 2:1:1:4 (Li, Zr, La, O)."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    counts = [2 * N // 8, N // 8, N // 8]
    z = [3] * counts[0] + [40] * counts[1] + [57] * counts[2]
    z += [8] * (N - len(z))
    numbers = rng.permutation(np.array(z)).astype(np.int32)
    pos, cell = _rattled_lattice(shape, 2.72, sigma, rng)
    return numbers, pos, cell, np.array([True, True, True])


def oxide_ordered(shape=(32, 32, 16), seed=0, sigma=0.05):
    """C5 for on-the-fly MD: the same 4 species and 2:1:1:4 stoichiometry (Li, Zr, La, O) on the same 2.72 A sites, but
    ORDERED — a rocksalt-type arrangement, O on the odd-parity sublattice, Zr / La / Li / Li on the four sites of the
    even one inside every 2x2x2 cube.  Its environments repeat, so a learner can cover them with ~10^3 inducing LCEs:
    in the randomly shuffled `oxide` every atom is its own environment (active.py:631-654 keeps every LCE whose
    similarity to the kept ones is below 0.95) and the reference's sampling loop would never stop adding."""
    rng = np.random.default_rng(seed)
    if any(n % 2 for n in shape):
        raise ValueError("even numbers of sites per direction")
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    par = g % 2
    even = par.sum(1) % 2 == 0
    key = par[:, 0] * 4 + par[:, 1] * 2 + par[:, 2]      # even sites: 0 (000), 3 (011), 5 (101), 6 (110)
    numbers = np.full(len(g), 8, np.int32)
    numbers[even & (key == 0)] = 40
    numbers[even & (key == 6)] = 57
    numbers[even & ((key == 3) | (key == 5))] = 3
    pos = g * 2.72 + sigma * rng.normal(size=(len(g), 3))
    return numbers, pos, np.diag([n * 2.72 for n in shape]).astype(float), np.array([True, True, True])


class PairTeacher:
    """Stand-in for the ab initio teacher of an on-the-fly run (a real run passes any ASE calculator: VASP, GPAW, ...):
    phi(r) = eps [(1 - e^{-a (r - r0)})^2 - 1] (1 - (r/rc)^2)^2 summed over the pairs of the DEVICE neighbour list,
    analytic forces and stress, ASE-calculator protocol (get_property(name, atoms))."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, species, rc=5.0, eps=0.25, a=1.4, r0=2.8, device=0):
        from .model import SGPRModel
        self.rc, self.eps, self.a, self.r0 = rc, eps, a, r0
        self.nl = SGPRModel(3, 3, 4, rc, species=species, device=device)  # used for its neighbour list only
        self.calls, self.seconds, self.results, self._key = 0, 0.0, {}, None

    def calculate(self, atoms):
        import time
        t0 = time.time()
        self.calls += 1
        pos = np.asarray(atoms.positions, float)
        cell = np.asarray(getattr(atoms.cell, "array", atoms.cell), float)
        N = len(pos)
        self.nl.predict(atoms.numbers, pos, cell, atoms.pbc, beta=False)
        ptr, j, off = self.nl.neighbors(N)
        i = np.repeat(np.arange(N), np.diff(ptr))
        d = pos[j] - pos[i] + off @ cell
        r = np.linalg.norm(d, axis=1)
        x = np.exp(-self.a * (r - self.r0))
        m_, dm = self.eps * ((1 - x) ** 2 - 1), self.eps * 2 * (1 - x) * self.a * x
        s = 1 - (r / self.rc) ** 2
        phi, dphi = m_ * s * s, dm * s * s - m_ * 4 * s * r / self.rc ** 2
        g = (dphi / r)[:, None] * d
        F = np.stack([np.bincount(i, weights=g[:, k], minlength=N) for k in range(3)], axis=1)
        vir = 0.5 * np.einsum("pa,pb->ab", d, g)
        stress = (vir / abs(np.linalg.det(cell)))[[0, 1, 2, 1, 0, 0], [0, 1, 2, 2, 2, 1]]
        self.results = dict(energy=0.5 * phi.sum(), forces=F, stress=stress, free_energy=0.5 * phi.sum())
        self.seconds += time.time() - t0

    def get_property(self, name, atoms=None):
        key = None if atoms is None else atoms.positions.tobytes()
        if atoms is not None and key != self._key:
            self.calculate(atoms)
            self._key = key
        return self.results[name]

    def close(self):
        self.nl.close()


FS = 0.09822694788464063  # ase.units.fs: 1 fs in A sqrt(amu/eV)
# hbar in eV (A sqrt(amu/eV)), from the CODATA-2014 numbers of ase.units: h / 2 pi / e * 1e10 sqrt(e / amu) (md_pimd.inc: PIMD_HBAR)
HBAR = 0.06465415105180661
MASS = {1: 1.008, 3: 6.94, 8: 15.999, 9: 18.998, 11: 22.99, 12: 24.305, 14: 28.085, 15: 30.974, 16: 32.06, 17: 35.45,
        40: 91.224, 57: 138.905}


def fixed_mask(fixed, N):
    """A held-component mask as the device loops take it (sgpr_md_fix): None, or an [N] (whole atoms: ase.constraints.FixAtoms)
    or [N, 3] (single Cartesian components: FixCartesian) array, True = held -> None when nothing is held, else bool [N, 3]."""
    if fixed is None:
        return None
    m = np.asarray(fixed)
    if m.shape == (N,):
        m = np.repeat(m.reshape(N, 1), 3, axis=1)
    if m.shape != (N, 3):
        raise ValueError(f"fixed: an [N] or [N, 3] array for N = {N} atoms, not {m.shape}")
    m = m != 0
    return m if m.any() else None


class FilterState:
    """What ActiveCalculator.run_md(ml_filter=) reads at its start and fills at its end: the shrink factor and the accumulators
    (None: zeros) as the run's last configuration found them — the next run_md handed the same holder evaluates that
    configuration again and goes on.  pushes: how many update jumps the device loops were handed."""

    def __init__(self, shrink, f=None, s=None):
        self.shrink, self.f, self.s, self.pushes = float(shrink), f, s, 0


class DeltaFilter:
    """The reference's FilterDeltas (calculator/active.py:47-76; `ml_filter` of cl/md.py:76-79) written by evaluation index, as
    the device loop applies it (sgpr_md_filter) — once per configuration n, with `deltas` what the calculator published there:
        A_f <- (A_f + deltas["forces"]) shrink,  F_seen = F - clip(A_f, -1, 1);   A_s <- (A_s + deltas["stress"]) shrink,  stress - A_s
    f, s: the accumulators; `before`: (f, s) as the configuration evaluated last found them — what filter_init= takes to
    evaluate that configuration again (SGPRModel.md_filter_state returns the same), so that a run cut there goes on bit for bit."""

    def __init__(self, shrink, init=None, N=None):
        if not 0.0 < float(shrink) < 1.0:
            raise ValueError("ml_filter: a shrink factor with 0 < shrink < 1")
        f0, s0 = (None, None) if init is None else init
        self.shrink = float(shrink)
        self.f = np.zeros((N, 3)) if f0 is None else np.array(f0, float)
        self.s = np.zeros(6) if s0 is None else np.array(s0, float)
        self.before = (self.f, self.s)

    def forces(self, F, deltas):
        self.before = (self.f, self.before[1])
        f = self.f + deltas["forces"] if deltas else self.f
        self.f = f * self.shrink
        return F - np.clip(self.f, -1.0, 1.0)

    def stress(self, S, deltas):
        self.before = (self.before[0], self.s)
        a = self.s + deltas["stress"] if deltas else self.s
        self.s = a * self.shrink
        return S - self.s


def _wave_order_sum(v):
    """fin_wave_sum (api.hip) of 64 values: the DPP network's order — lanes ^ 1, lanes ^ 2, the half row mirrored, the row
    mirrored — and the four rows as a pairwise tree."""
    v = np.asarray(v, float).reshape(64)
    i = np.arange(64)
    v = v + v[i ^ 1]
    v = v + v[i ^ 2]
    v = v + v[(i & ~7) | (7 - (i & 7))]
    v = v + v[(i & ~15) | (15 - (i & 15))]
    return float((v[0] + v[16]) + (v[32] + v[48]))


def _block_order_sum(p256):
    """The sum of a workgroup's 256 per-thread values as md_meta_kernel forms it: fin_wave_sum per wave, the waves pairwise."""
    w = [_wave_order_sum(p256[64 * k:64 * (k + 1)]) for k in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


META_TRIP = 1024   # hills per trip of md_meta_kernel's strided sum (four partial sums per thread)


META_QL_MAXT = 256   # selected neighbours of all qlvar components together (md_meta.inc: one thread each)
META_QL_MAXL = 12


def meta_cv_dim(cvs):
    return sum(1 if c[0] == "distance" else len(c[4]) if c[0] == "qlvar" else 3 for c in cvs)


def ql_environment(numbers, x, cell, pbc, index, zj, cutoff, order=None, nl=None):
    """The environment of a qlvar in the order of the device's neighbour list: the neighbours t of atom `index` that have species zj
    and r_t < cutoff, r_t = (x_j - x_index) + ((s0 a + s1 b) + s2 c) with the image triple s of the entry — sorted by the position
    of j in the library's species-sorted atom order (`order`: sorted -> caller; None: caller order), then by the image triple,
    as the forward kernel sorts an atom's list (descriptor.hip: key = neighbour | image).  nl: a neighbour list with
    get_neighbors(i) -> (indices, offsets) (the reference's interface; entries beyond cutoff are dropped); None: every image
    inside the cutoff along the periodic directions, by enumeration.  Returns (j [T], shifts [T, 3], r [T, 3], |r| [T])."""
    numbers = np.asarray(numbers)
    x = np.asarray(x, float)
    N = len(numbers)
    h = np.asarray(cell, float).reshape(3, 3)
    rank = np.arange(N)
    if order is not None:
        rank = np.empty(N, int)
        rank[np.asarray(order)] = np.arange(N)
    cand = []
    if nl is not None:
        jj, off = nl.get_neighbors(index)
        cand = [(int(j), int(o[0]), int(o[1]), int(o[2])) for j, o in zip(np.asarray(jj), np.asarray(off).reshape(-1, 3))]
    else:
        per = np.zeros(3, bool) if pbc is None else np.broadcast_to(np.asarray(pbc, bool), (3,))
        inv = np.linalg.inv(h) if per.any() else np.zeros((3, 3))
        reach = [cutoff * float(np.linalg.norm(inv[:, k])) for k in range(3)]   # cutoff over the height along axis k
        # (atom j under image s can be inside the cutoff only where |df_k + s_k| <= reach_k along every periodic axis)
        js = np.nonzero(numbers == zj)[0]
        df = (x[js] - x[index]) @ inv
        lo = np.where(per, np.ceil(-np.asarray(reach) - df - 1e-9), 0.0).astype(int)
        hi = np.where(per, np.floor(np.asarray(reach) - df + 1e-9), 0.0).astype(int)
        if len(js):
            for s0 in range(lo[:, 0].min(), hi[:, 0].max() + 1):
                for s1 in range(lo[:, 1].min(), hi[:, 1].max() + 1):
                    for s2 in range(lo[:, 2].min(), hi[:, 2].max() + 1):
                        s = np.array([s0, s1, s2])
                        cand += [(int(j), s0, s1, s2) for j in js[((lo <= s) & (s <= hi)).all(axis=1)]]
    ent = []
    for j, s0, s1, s2 in cand:
        if numbers[j] != zj or (j == index and s0 == 0 and s1 == 0 and s2 == 0):
            continue
        r = (x[j] - x[index]) + ((float(s0) * h[0] + float(s1) * h[1]) + float(s2) * h[2])
        ln = float(np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]))
        if ln < cutoff:
            ent.append((int(rank[j]), s0, s1, s2, j, r, ln))
    ent.sort(key=lambda e: e[:4])
    T = len(ent)
    return (np.array([e[4] for e in ent], int), np.array([e[1:4] for e in ent], int).reshape(T, 3),
            np.array([e[5] for e in ent], float).reshape(T, 3), np.array([e[6] for e in ent], float))


QL_TINY_ANGLE = 1e-2   # the reference's split_and_rotate_tiny_if_too_close_to_zaxis (descriptor/ylm.py:10-23)


def ql_rows(r, ln, cutoff):
    """The rows of a qlvar: (u, w, w', rhat, vlen, eps) — weights w = (1 - r / cutoff)^2 and their derivatives
    -2 (1 - r / cutoff) / cutoff from the lengths as they are, rhat = r / |r|, and the directions u = v / |v| the harmonics see:
    the reference's Ylm shears the WHOLE environment, v = (x, y - eps z, eps y + z) with eps = 1e-2, when any selected neighbour
    lies inside the cone |x|, |y| < eps |z| around the z axis (its Q_l then differs from the unsheared one by up to a few 1e-5: x
    keeps its scale, y and z gain sqrt(1 + eps^2)); eps = 0 otherwise, and then v is r, bit for bit."""
    tol = QL_TINY_ANGLE * np.abs(r[:, 2])
    eps = QL_TINY_ANGLE if bool(((np.abs(r[:, 0]) < tol) & (np.abs(r[:, 1]) < tol)).any()) else 0.0
    v = np.stack([r[:, 0], r[:, 1] - eps * r[:, 2], eps * r[:, 1] + r[:, 2]], axis=1)
    vlen = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    a = 1.0 - ln / cutoff
    return v / vlen[:, None], a * a, -((2.0 * a) / cutoff), r / ln[:, None], vlen, eps


def ql_dim(l, u, wt, wp, rhat, vlen, eps, base=0):
    """Q_l of one environment and dQ_l / dr_t [T, 3] in the operations and the order of md_meta.inc's meta_ql_dim (the definition):
    Q_l^2 = S / W^2, S = sum_t w_t A_t, A_t = sum_t' w_t' P_l(c), B_t = sum_t' w_t' P_l'(c) (u_t' - c u_t), c = u_t . u_t' — the
    addition theorem, P_l and P_l' by the three-term recurrence —,
        dQ_l^2 / dr_t = 2 (w'_t rhat_t A_t + w_t B_t / r_t) / W^2 - 2 Q_l^2 w'_t rhat_t / W,   dQ_l / dr_t = dQ_l^2 / dr_t / (2 Q_l)
    (u, rhat, vlen, eps of ql_rows: with the reference's shear, B_t / |v_t| is the derivative by v_t and goes through the shear).
    The pair sums of a row are formed by K = min(64, 256 / T rounded up to a power of two) lanes — lane k adds t' = k, k + K, ...
    one after the other, the K partial sums meet in a butterfly (^ 1, ^ 2, ...) —, S and W over the workgroup in fin_wave_sum's
    tree with row t in thread base + t.  An empty environment, or Q_l^2 <= 0: Q_l = 0 and no gradient (the reference: NaN)."""
    T = len(vlen)
    if T == 0:
        return 0.0, np.zeros((0, 3))
    Tp = 1
    while Tp < T:
        Tp <<= 1
    K = min(64, 256 // Tp)
    c = (u[:, None, 0] * u[None, :, 0] + u[:, None, 1] * u[None, :, 1]) + u[:, None, 2] * u[None, :, 2]
    p0, p1, e1 = np.ones_like(c), c.copy(), np.ones_like(c)
    if l == 0:
        p1, e1 = np.ones_like(c), np.zeros_like(c)
    for n in range(2, l + 1):
        pn = ((float(2 * n - 1) * c) * p1 - float(n - 1) * p0) / float(n)
        en = float(n) * p1 + c * e1
        p0, p1, e1 = p1, pn, en
    we = wt[None, :] * e1
    nit = -(-T // K)
    terms = np.zeros((T, nit * K, 4))
    terms[:, :T, 0] = wt[None, :] * p1
    for k in range(3):
        terms[:, :T, 1 + k] = we * (u[None, :, k] - c * u[:, None, k])
    acc = np.zeros((T, K, 4))
    for it in range(nit):
        acc = acc + terms[:, it * K:(it + 1) * K]
    lanes, m = np.arange(K), 1
    while m < K:
        acc = acc + acc[:, lanes ^ m]
        m <<= 1
    A, B = acc[:, 0, 0], acc[:, 0, 1:]
    v = np.zeros((256, 2))
    v[base:base + T, 0] = wt * A
    v[base:base + T, 1] = wt
    S, W = _block_order_sum(v[:, 0]), _block_order_sum(v[:, 1])
    W2 = W * W
    Q2 = S / W2
    if not Q2 > 0.0:
        return 0.0, np.zeros((T, 3))
    Q = float(np.sqrt(Q2))
    wu = wp[:, None] * rhat
    ang = (wt[:, None] * B) / vlen[:, None]   # d / dv; d / dr is its product with the shear from the right
    ang = np.stack([ang[:, 0], ang[:, 1] + eps * ang[:, 2], ang[:, 2] - eps * ang[:, 1]], axis=1)
    t1 = wu * A[:, None] + ang
    return Q, ((2.0 * t1) / W2 - ((2.0 * Q2) * wu) / W) / (2.0 * Q)


def meta_table(hills, sigma, merge):
    """The hills merged by bin, as the merged form of the bias holds them (md_meta_merge_kernel; the reference's Gaussian_kde keeps
    a counter per occupied bin): with B = (H // merge) * merge, the rows [0, B) of `hills` [H, D] become one entry per distinct
    centre (floor(c / sigma) + 0.5) sigma — compared by bits, which is one distinct bin floor(c / sigma) per dimension — that
    carries the block key floor(c / (5 sigma)) of the FIRST row that occupied it and the number of its rows as a double (an exact
    integer: no order of counting changes its bits).  Entries stand in the order of the first row that occupied them.
    Returns (centres [T, D], keys [T, D], counts [T], B)."""
    H = np.zeros((0, np.size(sigma))) if (hills is None or np.size(hills) == 0) else np.asarray(hills, float)
    H = H.reshape(len(H), -1) if H.ndim != 2 else H
    D = H.shape[1]
    merge = int(merge)
    if merge < 1:
        raise ValueError(f"meta_table: merge is a chunk length >= 1, not {merge}")
    B = (len(H) // merge) * merge
    sg = np.broadcast_to(np.asarray(sigma, float).reshape(-1), (D,)).astype(float)
    centre = np.ascontiguousarray((np.floor(H[:B] / sg) + 0.5) * sg)
    key = np.clip(np.floor(H[:B] / (5.0 * sg)), -1e9, 1e9)
    where, first, counts = {}, [], []
    for r in range(B):
        k = centre[r].tobytes()
        q = where.get(k)
        if q is None:
            where[k] = len(first)
            first.append(r)
            counts.append(1.0)
        else:
            counts[q] += 1.0
    first = np.asarray(first, int)
    return centre[first].reshape(-1, D), key[first].reshape(-1, D), np.asarray(counts, float), B


def meta_density(c, sigma, w, hills, tem=None, merge=None):
    """The bias on a given CV value c [D] — the one host statement of the hill rule, in md_meta_kernel's operations and order
    (meta_bias has the scheme): returns (V, dV/dc [D], kde).  sigma [D]; hills [H, D] CV values as deposited (None: none).
      merge = CH (a chunk length >= 1; None: every hill on its own, today's bits): the merged form of the device bias
    (sgpr_md_meta_merge).  The rows [0, B), B = (H // CH) * CH, are summed as the entries of meta_table — entry k adds cnt e to S
    and (cnt e) t_d to A_d, with near, t and e as for a hill, from the entry's centre and key — and the rows [B, H) one by one as
    before.  The order is a function of (rows, CH) alone: the entries first, entry k in the partial sum (k % 256, (k // 256) % 4),
    trip after trip of 1024; then the tail rows, row B + r into the partial sum (r % 256, (r // 256) % 4) of the SAME
    accumulators, trip after trip; then the four partial sums of a thread as (0 + 1) + (2 + 3) and fin_wave_sum's tree over
    the workgroup.  No product is contracted with a sum."""
    from .ase_shim import kB
    c = np.asarray(c, float).reshape(-1)
    D = len(c)
    sg = np.broadcast_to(np.asarray(sigma, float).reshape(-1), (D,)).astype(float)
    sg5 = 5.0 * sg
    kx = np.clip(np.floor(c / sg5), -1e9, 1e9)   # (the kernel's keys are ints, clamped there)
    H = np.zeros((0, D)) if (hills is None or np.size(hills) == 0) else np.asarray(hills, float).reshape(-1, D)
    S = np.zeros(1 + D)
    if len(H) and merge is not None:
        tc, tk, cnt, B = meta_table(H, sg, merge)
        groups = []
        for centre, key, n in ((tc, tk, cnt), ((np.floor(H[B:] / sg) + 0.5) * sg, np.clip(np.floor(H[B:] / sg5), -1e9, 1e9), None)):
            near = (np.abs(key - kx) <= 1).all(axis=1)
            t = (c - centre) / sg
            d2 = np.zeros(len(centre))
            for d in range(D):
                d2 = d2 + t[:, d] * t[:, d]
            e = np.where(near, np.exp(-0.5 * d2), 0.0)
            if n is not None:
                e = n * e
            terms = np.concatenate([e[:, None], e[:, None] * t], axis=1)
            terms[~near] = 0.0
            groups += [terms, np.zeros(((-len(terms)) % META_TRIP, 1 + D))]   # (each of the two starts its own trips)
        trips = np.concatenate(groups).reshape(-1, 4, 256, 1 + D)
        acc = np.zeros((4, 256, 1 + D))
        for tr in trips:
            acc = acc + tr
        per = (acc[0] + acc[1]) + (acc[2] + acc[3])
        S = np.array([_block_order_sum(per[:, d]) for d in range(1 + D)])
    elif len(H):
        centre = (np.floor(H / sg) + 0.5) * sg
        key = np.clip(np.floor(H / sg5), -1e9, 1e9)
        near = (np.abs(key - kx) <= 1).all(axis=1)
        t = (c - centre) / sg
        d2 = np.zeros(len(H))
        for d in range(D):
            d2 = d2 + t[:, d] * t[:, d]
        e = np.where(near, np.exp(-0.5 * d2), 0.0)
        terms = np.concatenate([e[:, None], e[:, None] * t], axis=1)   # [H, 1 + D]
        terms[~near] = 0.0
        pad = (-len(H)) % META_TRIP
        trips = np.concatenate([terms, np.zeros((pad, 1 + D))]).reshape(-1, 4, 256, 1 + D)
        acc = np.zeros((4, 256, 1 + D))
        for tr in trips:
            acc = acc + tr
        per = (acc[0] + acc[1]) + (acc[2] + acc[3])
        S = np.array([_block_order_sum(per[:, d]) for d in range(1 + D)])
    norm = 1.0
    for d in range(D):
        norm = norm * float(np.sqrt(2.0 * np.pi))
    kde = S[0] / norm
    V, fac = w * kde, w
    if tem is not None:
        gamma = 1.0 / (kB * tem)
        a_ = 1.0 + V * gamma
        V = float(np.log(a_)) / gamma
        fac = w / a_
    g = -(fac * ((S[1:] / sg) / norm))
    return float(V), g, float(kde)


def meta_bias(cvs, sigma, w, numbers, positions, cell, hills, tem=None, species=None, merge=None, pbc=None, rc=None, nl=None):
    """The bias potential of metadynamics at one configuration, in the operations of the device loop's md_meta_kernel
    (md_meta.inc; SGPRModel.md_meta) — the reference's calculator/meta.py (Meta.energy over analysis/kde.py's Gaussian_kde)
    restated for the built-in collective variables.  This function is the definition:
      cvs: components concatenated like the reference's Catvar, ("distance", i, j) = |x_j - x_i| and ("posvar", index, select)
    = x_index - (1/n) sum_{k in sel, k != index} x_k with sel all atoms (select None) or the atoms of species `select`, n = |sel|
    (the index atom counts in n where it is in sel: the reference's Posvar) — raw coordinates, no minimum image;
    ("qlvar", index, j, cutoff, (l, ...)) = the Steinhardt bond-order parameters Q_l of atom `index` over its neighbours of
    species j with r < cutoff (the reference's Qlvar over descriptor/ql.py), one dimension per l, 0 <= l <= 12 — ql_environment
    has the environment and its order, ql_dim the sums; it needs pbc and rc, the model's cutoff: the device reads the model's
    own list, which ends at rc where the weight (1 - r / cutoff)^2 is not zero, so cutoff <= rc (ValueError otherwise).  Unlike
    the reference, an empty environment gives Q_l = 0 with zero gradient (there: NaN), and so does Q_l = 0 (there: NaN, zeroed
    by nan_to_num).  Atom j_t takes -G_t = -sum_d dV/dQ_d dQ_d/dr_t once per image it stands under, the index atom the sum over
    the rows of the other atoms (its own images cancel), and the virial is sum_t r_t (x) G_t over the images — not the
    raw-coordinate -sum x (x) F of the other kinds, which an atom that stands under several images makes wrong;  nl: a
    neighbour list for the qlvars (the reference's interface) in place of the enumeration;
      a hill deposited at c (a row of `hills` [H, D]) is centred at (floor(c / sigma) + 0.5) sigma and carries the key
    floor(c / (5 sigma)) — 5 sigma a product, the divisions IEEE —; kde(x) = sum exp(-|(x - centre) / sigma|^2 / 2) / sqrt(2 pi)^D
    over the hills whose key differs from floor(x / (5 sigma)) by at most 1 in every dimension; sigma a scalar or [D];
      V = w kde, or with tem (K) log(1 + w kde gamma) / gamma, gamma = 1 / (kB tem).
    The sums run in the kernel's order (hill h in the partial sum (h % 256, (h // 256) % 4); the mean of a posvar over the
    atoms in the library's species-sorted order, `species` = the model's table, 256 strided partial sums; fin_wave_sum's
    tree); exp and log are this host's, so the device agrees to rounding, not bit for bit.
      merge = CH: the merged form (meta_density has the rule and the order; meta_table the entries); None: today's bits.
    Returns dict(cv [D], energy, forces [N, 3] = -dV/dx, stress [6] = Voigt of -(1/V_cell) sum_i x_i (x) F_i — formed as the
    kernel forms it: d (x) F_i for a distance, cv (x) dV/dcv for a posvar —, virial [9], dcv [D] = dV/dcv, kde, and margin:
    the smallest distance, in units of sigma, of a CV component from a bin edge k sigma or a block edge k 5 sigma — a
    comparison between two implementations means something only where a last-bit difference cannot move a hill by a bin)."""
    from .ase_shim import kB
    numbers = np.asarray(numbers)
    x = np.asarray(positions, float)
    N = len(numbers)
    D = meta_cv_dim(cvs)
    sg = np.broadcast_to(np.asarray(sigma, float).reshape(-1), (D,)).astype(float) if np.size(sigma) == 1 else np.asarray(sigma, float).reshape(D)
    sg5 = 5.0 * sg
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    c = np.zeros(D)
    parts = []   # per component: (kind, d0, ...) what the forces need
    d0 = 0
    qbase = 0    # rows of the qlvars that stand
    for comp in cvs:
        if comp[0] == "distance":
            i, j = int(comp[1]), int(comp[2])
            d = x[j] - x[i]
            r = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            c[d0] = r
            parts.append(("distance", d0, i, j, d, r))
            d0 += 1
        elif comp[0] == "posvar":
            idx, select = int(comp[1]), comp[2]
            insel = np.ones(N, bool) if select is None else (numbers == int(select))
            n = float(insel.sum())
            if n == 0:
                raise ValueError(f"meta_bias: no atom of species {select} (the mean of nothing)")
            a = insel.copy()
            a[idx] = False
            xs = np.where(a[order][:, None], x[order], 0.0)   # (an atom outside the mean adds nothing: the kernel skips it)
            pad = (-N) % 256
            rows = np.concatenate([xs, np.zeros((pad, 3))]).reshape(-1, 256, 3)
            p = np.zeros((256, 3))
            for r_ in rows:
                p = p + r_
            mean_sum = np.array([_block_order_sum(p[:, k]) for k in range(3)])
            c[d0:d0 + 3] = x[idx] - mean_sum / n
            parts.append(("posvar", d0, idx, a, n))
            d0 += 3
        elif comp[0] == "qlvar":
            idx, zj, cut, ls = int(comp[1]), int(comp[2]), float(comp[3]), [int(l) for l in comp[4]]
            if pbc is None or rc is None:
                raise ValueError("meta_bias: a qlvar needs pbc= and rc=, the model's cutoff")
            if not 0.0 < cut <= float(rc):
                raise ValueError(f"meta_bias: qlvar cutoff {cut}; the model's list ends at rc = {rc}, where the weight is not zero: 0 < cutoff <= rc")
            if not ls or any(l < 0 or l > META_QL_MAXL for l in ls):
                raise ValueError(f"meta_bias: qlvar l = {ls}; one or more of 0 ... {META_QL_MAXL}")
            jn, sh, r, ln = ql_environment(numbers, x, cell, pbc, idx, zj, cut, order=order, nl=nl)
            keep = min(len(ln), META_QL_MAXT - qbase)
            jn, sh, r, ln = jn[:keep], sh[:keep], r[:keep], ln[:keep]
            u, wt, wp, rhat, vlen, eps = ql_rows(r, ln, cut)
            dq = []
            for k, l in enumerate(ls):
                c[d0 + k], dql = ql_dim(l, u, wt, wp, rhat, vlen, eps, qbase)
                dq.append(dql)
            parts.append(("qlvar", d0, idx, jn, r, dq, qbase))
            qbase += keep
            d0 += len(ls)
        else:
            raise ValueError(f"meta_bias: a component is ('distance', i, j), ('posvar', index, select) or ('qlvar', index, j, cutoff, l), not {comp!r}")
    V, g, kde = meta_density(c, sg, w, hills, tem=tem, merge=merge)
    F = np.zeros((N, 3))
    vir = np.zeros(9)
    qvir = np.zeros(9)
    for part in parts:
        if part[0] == "qlvar":
            _, q, idx, jn, r, dq, base = part
            T = len(jn)
            G = np.zeros((T, 3))
            for k, dql in enumerate(dq):
                G = G + g[q + k] * dql
            other = jn != idx
            v = np.zeros((256, 3))
            v[base:base + T] = np.where(other[:, None], G, 0.0)
            F[idx] = F[idx] + np.array([_block_order_sum(v[:, k]) for k in range(3)])
            for t in np.nonzero(other)[0]:
                F[jn[t]] = F[jn[t]] - G[t]
            for a in range(3):
                v = np.zeros((256, 3))
                v[base:base + T] = r[:, a:a + 1] * G
                qvir[3 * a:3 * a + 3] = qvir[3 * a:3 * a + 3] + np.array([_block_order_sum(v[:, b]) for b in range(3)])
        elif part[0] == "distance":
            _, q, i, j, d, r = part
            fi = (g[q] * d) / r
            F[i] = F[i] + fi
            F[j] = F[j] - fi
            vir = vir + np.outer(d, fi).reshape(9)
        else:
            _, q, idx, a, n = part
            F[idx] = F[idx] - g[q:q + 3]
            F[a] = F[a] + g[q:q + 3] / n
            vir = vir + np.outer(c[q:q + 3], g[q:q + 3]).reshape(9)
    if qbase or any(part[0] == "qlvar" for part in parts):
        vir = vir + qvir
    cl = np.asarray(cell, float).reshape(3, 3)
    vol = abs(float(np.linalg.det(cl)))
    if not vol > 0.0:
        vol = -2.0   # (calculator/active.py:606-609)
    u = c / sg
    u5 = c / sg5
    margin = float(min(np.min(np.minimum(u - np.floor(u), np.ceil(u) - u)), 5.0 * np.min(np.minimum(u5 - np.floor(u5), np.ceil(u5) - u5)))) if D else np.inf
    return dict(cv=c, energy=float(V), forces=F, stress=vir[[0, 4, 8, 5, 2, 1]] / vol, virial=vir, dcv=g, kde=float(kde), margin=margin)


def langevin_nvt(calc, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, friction=1e-3, seed=1, vel=None, rng=None, fixed=None,
                 ml_filter=None, filter_init=None, meta=None):
    """BAOAB Langevin dynamics in numpy around any calculator with the ASE surface; parameters as the reference's
    driver (cl/md.py:31,70-74: dt = 1 fs, friction 1e-3 per ASE time unit, T = 600 K; Maxwell-Boltzmann start as
    util/aseutil.py:11-20, or the velocities handed over).  Generator: yields (step, energy, temperature, wall seconds,
    positions, velocities) after every step.  With ASE installed, ase.md.langevin.Langevin drives the same calculator.
      fixed: held components (fixed_mask: [N] or [N, 3], True = held), the rules of the device loop (sgpr_md_fix): the integrator
    sees F = 0 there (the calculator's results stay raw), the velocity is exactly 0 from the start (the caller's value is
    dropped), the deviate of a held component is drawn — one rng.normal(size=(N, 3)) per step as ever, so the free components
    consume what they consume without a mask — and not used, and the next coordinate is the current one, selected.  The
    temperature is over the g = 3N - n_fixed remaining degrees of freedom (atoms.get_temperature() under constraints).  None
    or nothing held: today's loop, bit for bit.
      ml_filter: the shrink factor of the filter of model-update jumps (DeltaFilter: calc.deltas is read after every evaluation;
    the device loop's sgpr_md_filter), filter_init: (f, s) its accumulators at the first configuration.  The integrator then
    sees F - clip(A_f, -1, 1) (a held component 0 as before); energies and the calculator's results stay raw.  Every yield
    gains a last entry, (f, s) as this configuration found the accumulators.  None: today's loop, bit for bit.
      meta: an autoforce_amd.meta.Meta — metadynamics by evaluation index, the device loop's sgpr_md_meta: configuration n is
    evaluated with the bias of the hills deposited by the configurations before it (energy + V, forces - dV/dx, added before
    the filter and the mask see them), then deposits its own when n % meta.pace == 0 (the reference's dyn.attach(meta.update)).
    For a calculator that does not add the bias itself (an ActiveCalculator(meta=) does: hand this loop meta=None then and
    call meta.update() per step).  None: today's loop, bit for bit."""
    import time
    from .ase_shim import Atoms, constraints_from_mask, kB
    rng = np.random.default_rng(seed) if rng is None else rng
    N = len(numbers)
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    kT = kB * temperature
    if vel is None:
        vel = rng.normal(size=(N, 3)) * np.sqrt(kT / mass)
        vel -= (mass * vel).sum(0) / mass.sum()
    vel = np.array(vel, float)
    fx = fixed_mask(fixed, N)
    cons = constraints_from_mask(fx)
    dof = 3 * N if fx is None else 3 * N - int(fx.sum())
    if fx is not None:
        vel[fx] = 0.0
    dt = dt_fs * FS
    c1 = np.exp(-friction * dt)
    c2 = np.sqrt(1 - c1 * c1)
    pos = np.array(pos, float)
    flt = None if ml_filter is None else DeltaFilter(ml_filter, filter_init, N)
    tail = (lambda: ()) if flt is None else (lambda: (flt.before,))

    def forces(p, v):
        # (the atoms carry the constraints, as the Atoms of an ASE loop around the calculator do: a calculator that learns takes
        # its copies — and its teacher's labels — from them; the forces taken here are the calculator's own)
        at = Atoms(numbers, p, cell, pbc, velocities=v, masses=mass[:, 0], constraint=cons)
        at.calc = calc
        F = at.get_forces(apply_constraint=False)
        E = at.get_potential_energy()
        if meta is not None:   # (the bias of this configuration, then its own hill)
            V, Fb, _ = meta.bias(p, cell, numbers, pbc=pbc)
            F, E = F + Fb, E + V
            meta.update()
        if flt is not None:   # (once per configuration)
            F = flt.forces(F, getattr(calc, "deltas", None))
        return F, E

    def seen(F):   # the forces the integrator sees
        return F if fx is None else np.where(fx, 0.0, F)

    t0 = time.time()
    F, E = forces(pos, vel)
    yield (0, E, float((mass * vel ** 2).sum() / (dof * kB)), time.time() - t0, pos, vel) + tail()
    for step in range(1, steps + 1):
        t0 = time.time()
        held = pos
        vel += 0.5 * dt * seen(F) / mass
        pos = pos + 0.5 * dt * vel
        xi = rng.normal(size=(N, 3))
        if fx is not None:
            xi = np.where(fx, 0.0, xi)
        vel = c1 * vel + c2 * np.sqrt(kT / mass) * xi
        pos = pos + 0.5 * dt * vel
        if fx is not None:   # (selected, not computed)
            pos = np.where(fx, held, pos)
            vel = np.where(fx, 0.0, vel)
        F, E = forces(pos, vel)
        vel += 0.5 * dt * seen(F) / mass
        yield (step, E, float((mass * vel ** 2).sum() / (dof * kB)), time.time() - t0, pos, vel) + tail()


def _device_order_sum(x):
    """Sum of x in the order of md_nh_kernel (api.hip): 256 strided partial sums (thread t adds the elements t, t + 256, ...
    one after the other), then a pairwise tree in natural order."""
    x = np.asarray(x, float)
    pad = (-len(x)) % 256
    rows = np.concatenate([x, np.zeros(pad)]).reshape(-1, 256)
    p = np.zeros(256)
    for r in rows:
        p = p + r
    while len(p) > 1:
        p = p[0::2] + p[1::2]
    return float(p[0])


def nose_hoover_nvt(calc, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, tdamp_fs=25.0, vel=None, seed=1, species=None,
                    fixed=None, ml_filter=None, filter_init=None, meta=None):
    """Nose-Hoover NVT in numpy around any calculator with the ASE surface: the reference's DEFAULT dynamics —
    md(dynamics="NPT", bulk_modulus=None) = ase.md.npt.NPT(pfactor=None, ttime=tdamp fs), cl/md.py:17, :131-166 — restated
    from ASE's published algorithm (Melchionna, Ciccotti, Holian 1993; ASE is absent here):
        x_(n+1) = (2 x_n - x_(n-1) (1 - b) + dt^2 F_n / m) / (1 + b),  b = dt zeta_n / 2,  v_n = (x_(n+1) - x_(n-1)) / 2 dt
        zeta_(n+1) = zeta_(n-1) + 2 dt tfact (KE_n - 1.5 (N - 1) kT),  tfact = 2 / (3 N kT ttime^2)
    started with x_(-1) = x_0 - dt v_0 + dt^2 F_0 / 2m, zeta_0 = 0, zeta_(-1) = -dt tfact (KE_0 - ...).  The host twin of the
    device loop (sgpr_md_thermostat): same operations in the same order, bit for bit (the kinetic energy is summed over the
    atoms in the library's species-sorted order: `species` = the model's table, default the sorted atomic numbers).  Yields
    (step, energy, temperature, wall seconds, positions, velocities, zeta, integral of zeta) per evaluated configuration.
      fixed: held components (fixed_mask), the rules of the device loop (sgpr_md_fix): F = 0 for the integrator, centred
    velocity exactly 0, the next coordinate the current one — selected: x (1 + b) / (1 + b) is not x bit for bit.  With
    g = 3N - n_fixed > 0 held components the thermostat works on the remaining degrees of freedom: tfact = 2 / (g kT ttime^2),
    K0 = g kT / 2 (no centre-of-mass degree removed: momentum is not conserved beside a held atom), temperature
    sum m v^2 / (g kB); conserved: E + KE + zeta^2 / tfact + 2 K0 int zeta dt, today's expression when nothing is held.  This
    is the project's own definition — ase.md.npt.NPT takes no constraints at all.  None or nothing held: today's loop, bit for
    bit.
      ml_filter, filter_init: the filter of model-update jumps, as in langevin_nvt (the filtered force, then the mask); every
    yield gains a last entry, (f, s) as this configuration found the accumulators.  None: today's loop, bit for bit.
      meta: metadynamics by evaluation index, as in langevin_nvt (the bias, then the filter, then the mask).  None: today's loop."""
    import time
    from .ase_shim import Atoms, constraints_from_mask, kB
    N = len(numbers)
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    kT = kB * temperature
    if vel is None:
        rng = np.random.default_rng(seed)
        vel = rng.normal(size=(N, 3)) * np.sqrt(kT / mass)
        vel -= (mass * vel).sum(0) / mass.sum()
    v0 = np.array(vel, float)
    fx = fixed_mask(fixed, N)
    cons = constraints_from_mask(fx)
    if fx is not None:
        v0[fx] = 0.0
    dof = float(3 * N) if fx is None else float(3 * N - int(fx.sum()))
    dt = dt_fs * FS
    hdt = 0.5 * dt
    dt = 2.0 * hdt
    ttime = tdamp_fs * FS
    tfact = 2.0 / (dof * kT * ttime * ttime)
    c1, c2, K0 = dt * tfact, 2.0 * dt * tfact, (1.5 * float(N - 1) * kT if fx is None else 0.5 * dof * kT)
    x = np.array(pos, float)
    xp = None
    zeta, zint = {0: 0.0}, {0: 0.0}
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    flt = None if ml_filter is None else DeltaFilter(ml_filter, filter_init, N)

    def forces(p, v):
        # (the atoms carry the constraints, as the Atoms of an ASE loop around the calculator do: a calculator that learns takes
        # its copies — and its teacher's labels — from them; the forces taken here are the calculator's own)
        at = Atoms(numbers, p, cell, pbc, velocities=v, masses=mass[:, 0], constraint=cons)
        at.calc = calc
        F, E = at.get_forces(apply_constraint=False), at.get_potential_energy()
        if meta is not None:   # (the bias of this configuration, then its own hill)
            V, Fb, _ = meta.bias(p, cell, numbers, pbc=pbc)
            F, E = F + Fb, E + V
            meta.update()
        return F, E

    for n in range(steps + 1):
        t0 = time.time()
        F, E = forces(x, v0 if n == 0 else v)   # (the velocities the integrator holds when it asks for forces: v_(n-1))
        if flt is not None:   # (once per configuration)
            F = flt.forces(F, getattr(calc, "deltas", None))
        if fx is not None:
            F = np.where(fx, 0.0, F)
        a = ((dt * dt) * F) / mass
        if n == 0:
            xp = (x - dt * v0) + 0.5 * a
        b = hdt * zeta[n]
        xn = (((2.0 * x) - xp * (1.0 - b)) + a) / (1.0 + b)
        v = v0 if n == 0 else (xn - xp) / (2.0 * dt)
        if fx is not None:   # (selected, not computed)
            xn = np.where(fx, x, xn)
            v = np.where(fx, 0.0, v)
        ke3 = mass * (v * v)
        ke_atom = (ke3[:, 0] + ke3[:, 1]) + ke3[:, 2]
        KE = 0.5 * _device_order_sum(ke_atom[order])
        d = KE - K0
        zprev = -(c1 * d) if n == 0 else zeta[n - 1]
        zeta[n + 1] = zprev + c2 * d
        zint[n + 1] = zint[n] + dt * zeta[n + 1]
        yield (n, E, float(2.0 * KE / ((3 * N if fx is None else dof) * kB)), time.time() - t0, x, v, zeta[n], zint[n]) + (
            () if flt is None else (flt.before,))
        xp, x = x, xn


# ---- the moving-cell scheme of npt.py in the device's operations (npt_moving_cell, and what md_npt_kernel / the MODE 3 last
# kernel of api.hip compute): 3 x 3 matrices as nested lists of floats, every product and sum spelled out in one fixed order
def _m3_mul(a, b):
    """a b, every entry (a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c."""
    return [[(a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c] for c in range(3)] for r in range(3)]


def _m3_inv_upper(h):
    """Inverse of an upper-triangular matrix in closed form (true divisions)."""
    i00, i11, i22 = 1.0 / h[0][0], 1.0 / h[1][1], 1.0 / h[2][2]
    i01 = -((h[0][1] * i00) * i11)
    i12 = -((h[1][2] * i11) * i22)
    i02 = ((h[0][1] * h[1][2] - h[0][2] * h[1][1]) * i00) * (i11 * i22)
    return [[i00, i01, i02], [0.0, i11, i12], [0.0, 0.0, i22]]


def _row_mul(q, m):
    """Row vectors times a matrix: out[:, c] = (q[:, 0] m_0c + q[:, 1] m_1c) + q[:, 2] m_2c."""
    return np.stack([(q[:, 0] * m[0][c] + q[:, 1] * m[1][c]) + q[:, 2] * m[2][c] for c in range(3)], axis=1)


def _npt_deta(fdt, pfact, h, stress6, ext6, mask, frac):
    """npt.NPT._deta: -fdt pfact det(h) (stress - external) as a strain-rate increment, with the mask or the trace /
    traceless split applied.  det of an upper-triangular h: (h00 h11) h22."""
    c = fdt * (pfact * ((h[0][0] * h[1][1]) * h[2][2]))
    de = [-(c * (stress6[k] - ext6[k])) for k in range(6)]
    u = [[de[0], de[5], de[4]], [0.0, de[1], de[3]], [0.0, 0.0, de[2]]]
    if frac == 1.0:
        return [[mask[r][c_] * u[r][c_] for c_ in range(3)] for r in range(3)]
    tr = ((u[0][0] + u[1][1]) + u[2][2]) / 3.0
    return [[(tr if r == c_ else 0.0) + frac * (u[r][c_] - (tr if r == c_ else 0.0)) for c_ in range(3)] for r in range(3)]


def _npt_matrices(dt, h, eta, zeta):
    """What the per-atom update of a configuration in the cell h needs: h^-1, B - 1 and (B + 1)^-1 with
    B = dt h ((eta + zeta/2 1) h^-1) (npt.NPT._q_future)."""
    hinv = _m3_inv_upper(h)
    hz = 0.5 * zeta
    g = [[eta[r][c] + (hz if r == c else 0.0) for c in range(3)] for r in range(3)]
    gh = _m3_mul(h, _m3_mul(g, hinv))
    b = [[dt * gh[r][c] for c in range(3)] for r in range(3)]
    bm1 = [[b[r][c] - (1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    bp1 = [[b[r][c] + (1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    return hinv, bm1, _m3_inv_upper(bp1)


def _npt_q_next(dt, F, mass, q, q_prev, hinv, bm1, bp1inv):
    """npt.NPT._q_future: (2 q + q_prev (B - 1) + dt^2 (F / m) h^-1) (B + 1)^-1."""
    a = ((dt * dt) * F) / mass
    return _row_mul(((2.0 * q) + _row_mul(q_prev, bm1)) + _row_mul(a, hinv), bp1inv)


def npt_moving_cell(calc, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, tdamp_fs=25.0, pfactor=None,
                    externalstress=0.0, mask=None, iso=False, vel=None, species=None, ml_filter=None, filter_init=None):
    """Nose-Hoover / Parrinello-Rahman dynamics with a moving cell in numpy around any calculator with the ASE surface: npt.NPT
    (ase.md.npt.NPT restated; what cl/md.py:131-166 runs when a bulk modulus is given) written by evaluation index, in the
    operations and the order of the device loop (sgpr_md_barostat: md_npt_kernel and the moving-cell form of the step's last
    kernel, api.hip) — its host twin, bit for bit.  No BLAS / LAPACK call (they fix no order of operations): the 3 x 3 algebra
    is spelled out (_m3_mul, _m3_inv_upper — h, eta and B are upper triangular —, _row_mul), sums over the atoms go through
    _device_order_sum in the library's species-sorted order (`species`: the model's table, default the sorted numbers).
    pfactor and externalstress in eV, Angstrom, amu units (npt.GPA, FS); externalstress a scalar pressure or six Voigt
    components; mask 3 or 3 x 3; iso: npt.NPT.set_fraction_traceless(0).  The cell must be upper triangular
    (npt.make_cell_upper_triangular).  pfactor = None: no barostat, the recurrence of nose_hoover_nvt.
      Blocks, by the lines of npt.py they restate:
        * the mean momentum removed (NPT.__init__, :133-134): npt.zero_mean_momentum;
        * constants tfact, pfact, desiredEkin (_constants, :174-178);
        * the start (initialize, :230-252): h_(-1), eta_(-1), zeta_(-1) by half increments, q_(-1) by the backward step that
          is corrected twice;
        * per evaluation n: the ideal-gas part of the stress (_stress, :194-201), eta_(n+1), zeta_(n+1), h_(n+2) (step,
          :259-261, with _deta, :212-221), q_(n+1) (_q_future, :223-228) and the centred velocity (:272), the positions of
          configuration n + 1 in ITS cell (_set_box_and_positions, :203-209).
    Yields (step, energy, temperature, wall seconds, positions, centred velocities, cell, eta, zeta, integral of zeta) per
    evaluated configuration (the velocities of configuration 0 are the ones handed over).
      ml_filter, filter_init: the filter of model-update jumps (DeltaFilter; sgpr_md_filter on the device): once per configuration
    the forces are reduced by the clamped force accumulator and, with a barostat, the stress by the stress accumulator — what
    npt.NPT(npt.FilterDeltas(atoms, shrink)) does, which calls the getters more than once at configuration 0 only (the same
    whenever the accumulators are zero there).  Every yield gains a last entry, (f, s) as this configuration found the
    accumulators.  None: today's loop, bit for bit."""
    import time
    from .ase_shim import Atoms, kB
    from .npt import zero_mean_momentum
    N = len(numbers)
    mass = np.array([MASS[int(z)] for z in numbers])[:, None]
    kT = kB * temperature
    if vel is None:
        rng = np.random.default_rng(1)
        vel = rng.normal(size=(N, 3)) * np.sqrt(kT / mass)
        vel -= (mass * vel).sum(0) / mass.sum()
    v0 = zero_mean_momentum(vel, mass[:, 0])
    hdt = 0.5 * (dt_fs * FS)
    dt = 2.0 * hdt
    ttime = tdamp_fs * FS
    tfact = 2.0 / (float(3 * N) * kT * ttime * ttime)
    c1, c2, K0 = dt * tfact, 2.0 * dt * tfact, 1.5 * float(N - 1) * kT
    h0 = [[float(v) for v in row] for row in np.asarray(cell, float).reshape(3, 3)]
    if not (h0[1][0] == 0.0 and h0[2][0] == 0.0 and h0[2][1] == 0.0):
        raise ValueError("the cell must be upper triangular (npt.make_cell_upper_triangular)")
    baro = pfactor is not None
    pfact = 1.0 / (float(pfactor) * ((h0[0][0] * h0[1][1]) * h0[2][2])) if baro else 0.0
    ext = np.asarray(externalstress, float)
    ext6 = [-float(ext)] * 3 + [0.0] * 3 if ext.ndim == 0 else [float(v) for v in ext.reshape(6)]
    mk = np.ones(3) if mask is None else np.asarray(mask)
    mk = np.not_equal(mk, 0)
    mk = (np.outer(mk, mk) if mk.shape == (3,) else mk).astype(float).tolist()
    frac = 0.0 if iso else 1.0
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    zero3 = [[0.0] * 3 for _ in range(3)]

    flt = None if ml_filter is None else DeltaFilter(ml_filter, filter_init, N)

    def evaluate(x, h, v):
        at = Atoms(numbers, x, np.array(h), pbc, velocities=v, masses=mass[:, 0])
        at.calc = calc
        F, E, S6 = np.asarray(at.get_forces(), float), float(at.get_potential_energy()), (np.asarray(at.get_stress(), float) if baro else np.zeros(6))
        if flt is not None:   # (once per configuration)
            d = getattr(calc, "deltas", None)
            F = flt.forces(F, d)
            if baro:
                S6 = flt.stress(S6, d)
        return F, E, S6

    def sums(v):
        ke3 = mass * (v * v)
        KE = 0.5 * _device_order_sum(((ke3[:, 0] + ke3[:, 1]) + ke3[:, 2])[order])
        S = [_device_order_sum((mass[:, 0] * (v[:, a] * v[:, b]))[order]) for a, b in VOIGT] if baro else [0.0] * 6
        return KE, S

    def sigma(stress6, S, h):
        vol = abs((h[0][0] * h[1][1]) * h[2][2])
        return [stress6[k] - S[k] / vol for k in range(6)]

    h, eta, zeta, zint = {0: h0}, {0: zero3}, {0: 0.0}, {0: 0.0}
    x = np.array(pos, float)
    q, qp = None, None
    for n in range(steps + 1):
        t0 = time.time()
        F, E, stress6 = evaluate(x, h[n], v0 if n == 0 else v)
        if n == 0:
            # ---- initialize(): eta_0 = 0, zeta_0 = 0
            hinv, bm1, bp1inv = _npt_matrices(dt, h[0], eta[0], zeta[0])
            q = _row_mul(x, hinv) - 0.5
            he = _m3_mul(h[0], eta[0])
            h[-1] = [[h[0][r][c] - dt * he[r][c] for c in range(3)] for r in range(3)]
            KE, S = sums(v0)
            d0 = _npt_deta(dt, pfact, h[0], sigma(stress6, S, h[0]), ext6, mk, frac) if baro else zero3
            eta[-1] = [[eta[0][r][c] - d0[r][c] for c in range(3)] for r in range(3)]
            zeta[-1] = zeta[0] - c1 * (KE - K0)
            vb = v0
            for _ in range(2):
                qp = q - dt * _row_mul(vb, hinv)
                qn = _npt_q_next(dt, F, mass, q, qp, hinv, bm1, bp1inv)
                vc = _row_mul(qn - qp, h[0]) / (2.0 * dt)
                if sums(vc)[0] / N < 1e-5:
                    break
                vb = (v0 - vc) + v0
            he = _m3_mul(h[0], eta[0])
            h[1] = [[h[-1][r][c] + (2.0 * dt) * he[r][c] for c in range(3)] for r in range(3)]
            v = v0
        else:
            hinv, bm1, bp1inv = _npt_matrices(dt, h[n], eta[n], zeta[n])
        qn = _npt_q_next(dt, F, mass, q, qp, hinv, bm1, bp1inv)
        if n > 0:
            v = _row_mul(qn - qp, h[n]) / (2.0 * dt)
        # ---- what the one-workgroup launch behind evaluation n computes: zeta, eta of n + 1, the cell of n + 2
        KE, S = sums(v)
        d = _npt_deta(2.0 * dt, pfact, h[n], sigma(stress6, S, h[n]), ext6, mk, frac) if baro else zero3
        eta[n + 1] = [[eta[n - 1][r][c] + d[r][c] for c in range(3)] for r in range(3)]
        zeta[n + 1] = zeta[n - 1] + c2 * (KE - K0)
        zint[n + 1] = zint[n] + dt * zeta[n + 1]
        he = _m3_mul(h[n + 1], eta[n + 1])
        h[n + 2] = [[h[n][r][c] + (2.0 * dt) * he[r][c] for c in range(3)] for r in range(3)]
        yield (n, E, float(2.0 * KE / (3 * N * kB)), time.time() - t0, x, v, np.array(h[n]), np.array(eta[n]), zeta[n], zint[n]) + (
            () if flt is None else (flt.before,))
        x = _row_mul(qn + 0.5, h[n + 1])
        qp, q = q, qn


# ---- FIRE relaxation of positions (and cell) in the device's operations (fire_relax; md_relax.inc: md_fire_kernel and
# md_fire_move_kernel)
FIRE_DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)   # ase/optimize/fire.py, ASE 3.22


def _m3_inv(d):
    """Inverse of a general 3 x 3 matrix in closed form: cofactors over the determinant (true divisions)."""
    c00 = d[1][1] * d[2][2] - d[1][2] * d[2][1]
    c01 = d[1][0] * d[2][2] - d[1][2] * d[2][0]
    c02 = d[1][0] * d[2][1] - d[1][1] * d[2][0]
    det = (d[0][0] * c00 - d[0][1] * c01) + d[0][2] * c02
    return [[c00 / det, (d[0][2] * d[2][1] - d[0][1] * d[2][2]) / det, (d[0][1] * d[1][2] - d[0][2] * d[1][1]) / det],
            [-c01 / det, (d[0][0] * d[2][2] - d[0][2] * d[2][0]) / det, (d[0][2] * d[1][0] - d[0][0] * d[1][2]) / det],
            [c02 / det, (d[0][1] * d[2][0] - d[0][0] * d[2][1]) / det, (d[0][0] * d[1][1] - d[0][1] * d[1][0]) / det]]


def _m3_mul_t(a, b):
    """a b^T, every entry (a_r0 b_c0 + a_r1 b_c1) + a_r2 b_c2."""
    return [[(a[r][0] * b[c][0] + a[r][1] * b[c][1]) + a[r][2] * b[c][2] for c in range(3)] for r in range(3)]


def _cell_volume(c):
    """|det| of a cell as sgpr_stress_from_virial takes it."""
    return abs(c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0])
               + c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]))


def fire_relax(calc, numbers, pos, cell, pbc, steps, fmax, cell_relax=False, mask=None, species=None, reset_at=(), fixed=None, **fire):
    """FIRE (ase/optimize/fire.py, ASE 3.22, LGPL, as cl/relax.py::FIRE restates it) on the positions — and, with cell_relax,
    on the cell through ase.constraints.UnitCellFilter(atoms, mask=mask) (cl/relax.py::UnitCellFilter) — in numpy around any
    calculator with the ASE surface, written by evaluation index in the operations and the summation order of the device loop
    (sgpr_md_relax: md_fire_kernel and md_fire_move_kernel, md_relax.inc): its host twin, bit for bit.  The state is the
    generalised coordinate vector X = [r ; c D] (r: positions referred to the cell h0 of the start, D: the deformation gradient,
    c = N) and its velocity.  Per evaluation n, with G = [F D ; (W D^-T o M) / c], W = -V stress:
        max over rows |G_row|^2 < fmax^2:  converged, nothing moves
        first evaluation (or the first after a reset):  alpha = 0,  beta = dt
        P = G.v > 0:   alpha = 1 - a,  beta = a |v| / |G| + dt   (then, if nsteps > nmin: dt = min(dt finc, dtmax), a *= fa — ASE
                       raises dt BEFORE the step that uses it; nsteps += 1)
        else:          alpha = 0,  a = astart,  dt *= fdec,  nsteps = 0,  beta = dt
        v = alpha v + beta G;  |v|^2 = alpha^2 v.v + 2 alpha beta G.v + beta^2 G.G  (closed form: no second reduction);
        X += s dt v  with  s = maxstep / (dt |v|) when dt |v| > maxstep, else 1
    — ASE's `(1 - a) v + a |v| / |G| G` followed by `v += dt G` with the two multiples of G added first: the order of rounding
    only.  Dots run over all 3N (+ 9) components: the atoms' part through _device_order_sum in the library's species-sorted
    order (`species`: the model's table), the three cell rows added behind it.  No BLAS call.  reset_at: evaluation indices in
    front of which the optimizer is re-initialised (optimizer.initialize(): v = 0, dt, a, nsteps as at the start).
      fixed: held components (fixed_mask), the rules of the device loop (sgpr_md_fix): the optimizer sees F = 0 there and the
    component of G = F D is zero in all three sums and in max |G_row|^2 (convergence is judged on the free components; the cell
    rows are unchanged), its velocity is 0 and its coordinate r is handed on as it is, selected: at constant cell x = r keeps its
    bits, with cell_relax r is what is held and x = r D^T follows the cell — ase.constraints.FixAtoms inside UnitCellFilter.
    None or nothing held: today's loop, bit for bit.
      Yields a dict per evaluated configuration: n, energy, positions, cell, D, gmax2 (largest |G_row|^2), P (G.v; 0 for a
    first evaluation), dt and a as used for the move out of this configuration (as they stand when it has converged), nsteps
    behind that move, converged.  The generator ends behind a converged configuration."""
    from .ase_shim import Atoms, constraints_from_mask
    p = dict(FIRE_DEFAULTS)
    p.update(fire)
    N = len(numbers)
    cf = float(N)
    h0 = [[float(v) for v in row] for row in np.asarray(cell, float).reshape(3, 3)]
    if mask is None:
        mask = [1.0] * 6
    mk6 = [1.0 if float(v) != 0.0 else 0.0 for v in np.asarray(mask, float).reshape(6)]
    M = [[mk6[0], mk6[5], mk6[4]], [mk6[5], mk6[1], mk6[3]], [mk6[4], mk6[3], mk6[2]]]
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    r = np.array(pos, float)
    x = r.copy()
    Xc = [[cf * eye[a][b] for b in range(3)] for a in range(3)]     # the cell rows of X: c D
    D, h = eye, h0
    v, vc = np.zeros_like(r), [[0.0] * 3 for _ in range(3)]
    dt, a, nsteps, fresh = float(p["dt"]), float(p["astart"]), 0, True
    fmax2 = float(fmax) * float(fmax)
    fx = fixed_mask(fixed, N)
    cons = constraints_from_mask(fx)   # (the atoms handed to the calculator carry them, as in an ASE loop)

    def dot(u, w, uc, wc):
        t = u * w
        s = _device_order_sum(((t[:, 0] + t[:, 1]) + t[:, 2])[order])
        if cell_relax:
            rows = [(uc[k][0] * wc[k][0] + uc[k][1] * wc[k][1]) + uc[k][2] * wc[k][2] for k in range(3)]
            s = s + ((rows[0] + rows[1]) + rows[2])
        return s

    for n in range(steps + 1):
        if n in reset_at:
            v, vc = np.zeros_like(r), [[0.0] * 3 for _ in range(3)]
            dt, a, nsteps, fresh = float(p["dt"]), float(p["astart"]), 0, True
        at = Atoms(numbers, x, np.array(h), pbc, constraint=cons)
        at.calc = calc
        F, E = np.asarray(at.get_forces(apply_constraint=False), float), float(at.get_potential_energy())
        if fx is not None:
            F = np.where(fx, 0.0, F)
        Gc = [[0.0] * 3 for _ in range(3)]
        if cell_relax:
            s6 = [float(t) for t in np.asarray(at.get_stress(), float)]
            vol = _cell_volume(h)
            w6 = [-(vol * t) for t in s6]
            W = [[w6[0], w6[5], w6[4]], [w6[5], w6[1], w6[3]], [w6[4], w6[3], w6[2]]]
            T = _m3_mul_t(W, _m3_inv(D))
            Gc = [[(T[a_][b] * M[a_][b]) / cf for b in range(3)] for a_ in range(3)]
            G = _row_mul(F, D)
            if fx is not None:
                G = np.where(fx, 0.0, G)
        else:
            G = F
        g2 = G * G
        g2 = (g2[:, 0] + g2[:, 1]) + g2[:, 2]
        gmax2 = float(g2.max()) if N else 0.0
        if cell_relax:
            gmax2 = max(gmax2, max((Gc[k][0] * Gc[k][0] + Gc[k][1] * Gc[k][1]) + Gc[k][2] * Gc[k][2] for k in range(3)))
        P = 0.0 if fresh else dot(G, v, Gc, vc)
        out = dict(n=n, energy=E, positions=x, cell=np.array(h), D=np.array(D), gmax2=gmax2, P=P)
        if gmax2 < fmax2:
            out.update(dt=dt, a=a, nsteps=nsteps, converged=True)
            yield out
            return
        GG = dot(G, G, Gc, Gc)
        vv = 0.0
        if fresh:
            alpha, beta = 0.0, dt
            fresh = False
        elif P > 0.0:
            vv = dot(v, v, vc, vc)
            alpha = 1.0 - a
            gamma = (a * np.sqrt(vv)) / np.sqrt(GG)
            if nsteps > p["nmin"]:
                dt = min(dt * p["finc"], p["dtmax"])
                a = a * p["fa"]
            nsteps += 1
            beta = gamma + dt
        else:
            alpha, a, nsteps = 0.0, float(p["astart"]), 0
            dt = dt * p["fdec"]
            beta = dt
        nv2 = ((alpha * alpha) * vv + (2.0 * (alpha * beta)) * P) + (beta * beta) * GG
        drn = dt * float(np.sqrt(nv2))
        cd = dt * (p["maxstep"] / drn) if drn > p["maxstep"] else dt
        out.update(dt=dt, a=a, nsteps=nsteps, converged=False)
        yield out
        v = alpha * v + beta * G
        if fx is None:
            r = r + cd * v
        else:   # (selected, not computed)
            v = np.where(fx, 0.0, v)
            r = np.where(fx, r, r + cd * v)
        if cell_relax:
            vc = [[alpha * vc[a_][b] + beta * Gc[a_][b] for b in range(3)] for a_ in range(3)]
            Xc = [[Xc[a_][b] + cd * vc[a_][b] for b in range(3)] for a_ in range(3)]
            D = [[Xc[a_][b] / cf for b in range(3)] for a_ in range(3)]
            h = _m3_mul_t(h0, D)
            x = _row_mul(r, [[D[b][a_] for b in range(3)] for a_ in range(3)])
        else:
            x = r


# ---- limited-memory BFGS on the same generalised coordinates in the device's operations (lbfgs_relax; md_lbfgs.inc:
# md_lbfgs_dots_kernel, md_lbfgs_solve_kernel, md_lbfgs_dir_kernel and md_lbfgs_move_kernel)
LBFGS_DEFAULTS = dict(memory=100, maxstep=0.2, alpha=70.0, damping=1.0)   # ase/optimize/lbfgs.py, ASE 3.22
LBFGS_MAX_MEMORY = 128   # pairs kept at most (md_lbfgs.inc: one thread of the one-workgroup kernel per pair)


def _block_partials(vals):
    """Per-row values [..., N] in sorted atom order -> [..., B]: one sum per workgroup of 256 rows, each _block_order_sum
    (zeros beyond N), for all leading indices at once — the same operations element by element."""
    vals = np.asarray(vals, float)
    pad = (-vals.shape[-1]) % 256
    if pad:
        vals = np.concatenate([vals, np.zeros(vals.shape[:-1] + (pad,))], axis=-1)
    v = vals.reshape(vals.shape[:-1] + (-1, 4, 64))
    i = np.arange(64)
    v = v + v[..., i ^ 1]
    v = v + v[..., i ^ 2]
    v = v + v[..., (i & ~7) | (7 - (i & 7))]
    v = v + v[..., (i & ~15) | (15 - (i & 15))]
    w = (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _index_order_sum(parts):
    """Per-workgroup partial sums [..., B] added one after the other in index order, from zero."""
    parts = np.asarray(parts, float)
    acc = np.zeros(parts.shape[:-1])
    for w in range(parts.shape[-1]):
        acc = acc + parts[..., w]
    return acc


def _rows3(u, w):
    """The three-component dot of every row: (u0 w0 + u1 w1) + u2 w2."""
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


class LbfgsTwin:
    """The history of the device's L-BFGS (md_lbfgs.inc) and the product p = H G in its compact form (Byrd, Nocedal & Schnabel,
    Math. Program. 63, 129 (1994)), operation for operation.  Everything is indexed by evaluation: pair i (formed at evaluation
    i: s_i = X_i - X_(i-1), y_i = G_(i-1) - G_i) lives in slot i % memory of S and Y, column i of R^-1 and row / column i of
    Y^T Y in row / column i % memory of two memory x memory arrays, G_i in slot i % 2 — an evaluation that is repeated writes
    its own slots again and nothing else.  At evaluation n behind a start or reset at `base` the window is the pairs
    max(base + 1, n - memory + 1) ... n, oldest first; a pair whose s.y is zero or not finite keeps its slot and is left out of
    every product (valid = False).  With R the upper triangle of S^T Y over the valid pairs, Dg its diagonal, H0 = 1 / alpha:
        u = S^T G,  v = H0 Y^T G,  t = R^-1 u,  top = R^-T ((Dg + H0 Y^T Y) t - v),  p = H0 G + S top - H0 Y t
    R^-1 is never solved for: pair n adds the column [-R^-1 c / d ; 1 / d] (c_i = s_i.y_n, d = s_n.y_n), the oldest pair leaves
    with its row and column.  Sums over the atoms: per workgroup of 256 rows in sorted order (_block_partials), the workgroups
    in index order (_index_order_sum), the three cell rows behind them; sums over pairs: oldest first.
    Rows: the N atoms in CALLER order (`order`: sorted -> caller), then — cell — the three cell rows.  held: bool [rows, 3]."""

    def __init__(self, N, order, memory, alpha, cell=False, held=None):
        self.N, self.NR, self.order, self.m, self.cell = N, N + (3 if cell else 0), np.asarray(order), int(memory), bool(cell)
        if not 1 <= self.m <= LBFGS_MAX_MEMORY:
            raise ValueError(f"memory: 1 ... {LBFGS_MAX_MEMORY}")
        self.H0 = 1.0 / float(alpha)
        self.held = held
        m = self.m
        self.S, self.Y, self.G = np.zeros((m, self.NR, 3)), np.zeros((m, self.NR, 3)), np.zeros((2, self.NR, 3))
        self.Rinv, self.YY, self.Dg, self.valid = np.zeros((m, m)), np.zeros((m, m)), np.zeros(m), np.zeros(m, bool)
        self.base = 0
        self._ev = None

    def reset(self, n):
        """Evaluation n is the first of a fresh history."""
        self.base = int(n)

    def _dot(self, A, b):
        """A [K, rows, 3] . b [rows, 3] -> [K] in the device's order."""
        N = self.N
        s = _index_order_sum(_block_partials(_rows3(A[:, :N], b[None, :N])[:, self.order]))
        if self.cell:
            r = _rows3(A[:, N:], b[None, N:])
            s = s + ((r[:, 0] + r[:, 1]) + r[:, 2])
        return s

    def evaluate(self, n, G):
        """Evaluation n with the generalised forces G [rows, 3] (held entries zero): stores G_n and y_n, forms the sums.
        Returns dict(cnt: pairs in the window, pairs: the valid ones, GG, gmax2)."""
        m, n = self.m, int(n)
        G = np.array(G, float)
        cnt = min(n - self.base, m)
        lo = n - cnt + 1
        self.G[n % 2] = G
        GG = float(self._dot(G[None], G)[0])
        g2 = _rows3(G, G)
        ev = dict(n=n, cnt=cnt, lo=lo, GG=GG, gmax2=float(g2.max()), G=G)
        if cnt:
            y = self.G[(n - 1) % 2] - G
            self.Y[n % m] = y
            sl = [i % m for i in range(lo, n + 1)]
            S, Y = self.S[sl], self.Y[sl]
            ev.update(c=self._dot(S, y), yy=self._dot(Y, y), u=self._dot(S, G), yg=self._dot(Y, G), sl=sl)
            d = float(ev["c"][-1])
            self.valid[n % m] = bool(np.isfinite(d) and d != 0.0)
        ev["pairs"] = int(sum(bool(self.valid[i % m]) for i in range(lo, n + 1)))
        self._ev = ev
        return dict(cnt=cnt, pairs=ev["pairs"], GG=GG, gmax2=ev["gmax2"])

    def direction(self):
        """p = H G [rows, 3] of the evaluation just evaluated, and p.G in closed form (H0 G.G + top.u - t.v)."""
        ev, m, H0 = self._ev, self.m, self.H0
        n, cnt, G = ev["n"], ev["cnt"], ev["G"]
        p = H0 * G
        pG = H0 * ev["GG"]
        if cnt:
            sl, c, u = ev["sl"], [float(x) for x in ev["c"]], [float(x) for x in ev["u"]]
            v = [H0 * float(x) for x in ev["yg"]]
            val = [bool(self.valid[s]) for s in sl]
            new, sn = cnt - 1, sl[cnt - 1]
            d = c[new]
            Rinv, YY, Dg = self.Rinv, self.YY, self.Dg
            for a in range(new):                       # the new column of R^-1
                col = 0.0
                if val[new] and val[a]:
                    acc = 0.0
                    for l in range(a, new):
                        if val[l]:
                            acc = acc + Rinv[sl[a], sl[l]] * c[l]
                    col = (-acc) / d
                Rinv[sl[a], sn] = col
            Rinv[sn, sn] = 1.0 / d if val[new] else 0.0
            for a in range(cnt):
                YY[sl[a], sn] = YY[sn, sl[a]] = float(ev["yy"][a])
            Dg[sn] = d
            t, w, top = [0.0] * cnt, [0.0] * cnt, [0.0] * cnt
            for a in range(cnt):
                if val[a]:
                    acc = 0.0
                    for l in range(a, cnt):
                        if val[l]:
                            acc = acc + Rinv[sl[a], sl[l]] * u[l]
                    t[a] = acc
            for a in range(cnt):
                if val[a]:
                    acc = 0.0
                    for j in range(cnt):
                        if val[j]:
                            mij = H0 * YY[sl[a], sl[j]]
                            if j == a:
                                mij = Dg[sl[a]] + mij
                            acc = acc + mij * t[j]
                    w[a] = acc - v[a]
            for a in range(cnt):
                if val[a]:
                    acc = 0.0
                    for i in range(a + 1):
                        if val[i]:
                            acc = acc + Rinv[sl[i], sl[a]] * w[i]
                    top[a] = acc
            for a in range(cnt):
                if val[a]:
                    pG = (pG + top[a] * u[a]) - t[a] * v[a]
                    p = (p + top[a] * self.S[sl[a]]) - (H0 * t[a]) * self.Y[sl[a]]
        if self.held is not None:
            p = np.where(self.held, 0.0, p)
        return p, float(pG)

    def moved(self, n, s):
        """The move out of evaluation n: s = X_(n+1) - X_n, the pair evaluation n + 1 completes."""
        self.S[(int(n) + 1) % self.m] = s


def lbfgs_relax(calc, numbers, pos, cell, pbc, steps, fmax, cell_relax=False, mask=None, species=None, reset_at=(), fixed=None, reset_if=None,
                **lbfgs):
    """L-BFGS without line search (ase/optimize/lbfgs.py, ASE 3.22, LGPL; Nocedal, Math. Comp. 35, 773 (1980)) on the
    generalised coordinates and forces of fire_relax — X = [r ; c D], G = [F D ; (W D^-T o M) / c] — in numpy around any
    calculator with the ASE surface, in the operations and the summation order of the device loop (sgpr_md_relax_lbfgs:
    md_lbfgs.inc): its host twin and the definition.  lbfgs: memory (pairs kept at most, 1 ... 128), maxstep, alpha (H0 =
    1 / alpha), damping — ASE's keywords and defaults.  Per evaluation n:
        max over rows |G_row|^2 < fmax^2:  converged, nothing moves
        behind a start or reset:  a pair s_n = X_n - X_(n-1) (the rounded difference of the stored coordinates, as ASE takes
            r - r0), y_n = G_(n-1) - G_n; at most `memory` pairs are kept, no curvature test — but a pair whose s.y is zero or
            not finite is left out (ASE would divide by it)
        p = H G through the compact form (LbfgsTwin), which is the two-loop recursion over the same pairs up to rounding
        step = damping * p, scaled by maxstep / longest when the longest row (atoms and cell rows) reaches maxstep (ASE's >=)
    reset_at: evaluation indices in front of which the history is emptied (optimizer.initialize()); reset_if: called behind
    the calculator's answer of every evaluation, true empties the history in front of that evaluation too (an active
    calculator that has just updated its model: the device loop's relax_reset behind a hand-over).  fixed: as in fire_relax — G = 0, the step is 0 and r keeps its bits, selected.
      Yields a dict per evaluated configuration: n, energy, positions, cell, D, gmax2, pG (p.G; 0 where nothing moves),
    scale (the factor applied to p; 0 where nothing moves), pairs (valid pairs in the window), converged.  The generator ends
    behind a converged configuration."""
    from .ase_shim import Atoms, constraints_from_mask
    unknown = set(lbfgs) - set(LBFGS_DEFAULTS)
    if unknown:
        raise TypeError(f"lbfgs_relax: unknown L-BFGS keywords {sorted(unknown)}")
    p = dict(LBFGS_DEFAULTS)
    p.update(lbfgs)
    maxstep, damping = float(p["maxstep"]), float(p["damping"])
    N = len(numbers)
    cf = float(N)
    h0 = [[float(v) for v in row] for row in np.asarray(cell, float).reshape(3, 3)]
    if mask is None:
        mask = [1.0] * 6
    mk6 = [1.0 if float(v) != 0.0 else 0.0 for v in np.asarray(mask, float).reshape(6)]
    M = [[mk6[0], mk6[5], mk6[4]], [mk6[5], mk6[1], mk6[3]], [mk6[4], mk6[3], mk6[2]]]
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    r = np.array(pos, float)
    x = r.copy()
    Xc = np.array([[cf * eye[a][b] for b in range(3)] for a in range(3)])     # the cell rows of X: c D
    D, h = eye, h0
    fmax2 = float(fmax) * float(fmax)
    fx = fixed_mask(fixed, N)
    cons = constraints_from_mask(fx)
    held = None if fx is None else (np.concatenate([fx, np.zeros((3, 3), bool)]) if cell_relax else fx)
    tw = LbfgsTwin(N, order, p["memory"], p["alpha"], cell=cell_relax, held=held)
    for n in range(steps + 1):
        if n in reset_at:
            tw.reset(n)
        at = Atoms(numbers, x, np.array(h), pbc, constraint=cons)
        at.calc = calc
        F, E = np.asarray(at.get_forces(apply_constraint=False), float), float(at.get_potential_energy())
        if reset_if is not None and reset_if():
            tw.reset(n)
        if fx is not None:
            F = np.where(fx, 0.0, F)
        if cell_relax:
            s6 = [float(t) for t in np.asarray(at.get_stress(), float)]
            vol = _cell_volume(h)
            w6 = [-(vol * t) for t in s6]
            W = [[w6[0], w6[5], w6[4]], [w6[5], w6[1], w6[3]], [w6[4], w6[3], w6[2]]]
            T = _m3_mul_t(W, _m3_inv(D))
            Gc = [[(T[a_][b] * M[a_][b]) / cf for b in range(3)] for a_ in range(3)]
            G = _row_mul(F, D)
            if fx is not None:
                G = np.where(fx, 0.0, G)
            G = np.concatenate([G, np.array(Gc)])
        else:
            G = F
        ev = tw.evaluate(n, G)
        out = dict(n=n, energy=E, positions=x, cell=np.array(h), D=np.array(D), gmax2=ev["gmax2"], pG=0.0, scale=0.0, pairs=ev["pairs"])
        if ev["gmax2"] < fmax2:
            out.update(converged=True)
            yield out
            return
        if n == steps:   # (the last evaluation: nothing moves behind it)
            out.update(converged=False)
            yield out
            return
        pdir, pG = tw.direction()
        longest = float(np.sqrt(_rows3(pdir, pdir).max()))
        sc = maxstep / longest if longest >= maxstep else 1.0
        out.update(pG=pG, scale=sc, converged=False)
        yield out
        dr = (pdir * sc) * damping
        rn = r + dr[:N]
        if fx is not None:   # (selected, not computed)
            rn = np.where(fx, r, rn)
        s = rn - r
        r = rn
        if cell_relax:
            Xn = Xc + dr[N:]
            s = np.concatenate([s, Xn - Xc])
            Xc = Xn
            D = [[float(Xc[a_][b]) / cf for b in range(3)] for a_ in range(3)]
            h = _m3_mul_t(h0, D)
            x = _row_mul(r, [[D[b][a_] for b in range(3)] for a_ in range(3)])
        else:
            x = r
        tw.moved(n, s)


# ---- the nudged elastic band under FIRE in the device's operations (neb_fire; md_neb.inc: md_neb_sums_kernel, md_neb_fire_kernel
# and md_neb_move_kernel)
NEB_MAX = 16   # interior images of a band (md_neb.inc)


def _neb_mic(d, h, hi, pbc):
    """Minimum-image form of displacements d [N, 3]: d - rint(d h^-1) h in the periodic directions (neb_mic, md_neb.inc)."""
    n = [np.rint((d[:, 0] * hi[0][k] + d[:, 1] * hi[1][k]) + d[:, 2] * hi[2][k]) if pbc[k] else np.zeros(len(d)) for k in range(3)]
    return np.stack([d[:, c] - ((n[0] * h[0][c] + n[1] * h[1][c]) + n[2] * h[2][c]) for c in range(3)], axis=1)


def _neb_cell(cell, pbc):
    h = [[float(v) for v in row] for row in np.asarray(cell, float).reshape(3, 3)]
    pbc = [bool(b) for b in np.broadcast_to(np.asarray(pbc, bool), (3,))]
    hi = [[0.0] * 3 for _ in range(3)]
    if any(pbc):
        if not _cell_volume(h) > 0.0:
            raise ValueError("neb: the cell is singular")
        hi = _m3_inv(h)
    return h, hi, pbc


def neb_check_band(images, cell, pbc):
    """The test sgpr_md_neb applies to the initial band: the rounding of _neb_mic recovers a displacement between neighbouring
    images only when it is well inside half a cell.  ValueError when a fractional component of a displacement, after rounding,
    is within 1e-9 of +-1/2 (rint may go either way from one evaluation to the next), or when the displacement after rounding
    is longer than half the smallest perpendicular width of the periodic directions (another image of the atom may be the
    nearer one).  The user keeps neighbouring images closer than that for the whole run: only the initial band is checked."""
    h, hi, pbc = _neb_cell(cell, pbc)
    if not any(pbc):
        return
    R = np.asarray(images, float)
    wmin = min(1.0 / np.sqrt((hi[0][k] * hi[0][k] + hi[1][k] * hi[1][k]) + hi[2][k] * hi[2][k]) for k in range(3) if pbc[k])
    for i in range(1, len(R)):
        o = _neb_mic(R[i] - R[i - 1], h, hi, pbc)
        for k in range(3):
            if pbc[k]:
                sfr = (o[:, 0] * hi[0][k] + o[:, 1] * hi[1][k]) + o[:, 2] * hi[2][k]
                if (np.abs(sfr) >= 0.5 - 1e-9).any():
                    c = int(np.argmax(np.abs(sfr)))
                    raise ValueError(f"neb: atom {c} moves half a cell (fractional {sfr[c]:.6f} along vector {k}) between images {i - 1} and {i}: "
                                     "the minimum-image rounding cannot recover it; add images")
        ln = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
        if (ln > 0.5 * wmin).any():
            c = int(np.argmax(ln))
            raise ValueError(f"neb: atom {c} moves {ln[c]:.4f} between images {i - 1} and {i}, more than half the smallest perpendicular "
                             f"width of the cell ({wmin:.4f}): the minimum-image rounding cannot recover it; add images")


def neb_fire(calc, numbers, images, cell, pbc, evals, fmax, k=0.1, climb=False, fixed=None, species=None, reset_at=(), update=None, **fire):
    """The nudged elastic band — ASE's default `aseneb` method (ase/neb.py, ASE 3.22, LGPL) — under FIRE (fire_relax's recurrence
    at constant cell) in numpy around any calculator with the three getters (forces and energy through the atoms,
    calc.get_covloss()), one call per interior image per evaluation: the host twin of the device loop (sgpr_md_neb:
    md_neb_sums_kernel, md_neb_fire_kernel, md_neb_move_kernel; md_neb.inc) in its operations and summation order, bit for bit —
    and, ASE not being a dependency, the definition.  images [K + 2, N, 3]: images 0 and K + 1 are the ends, never evaluated or
    moved; all share numbers, cell (constant) and pbc.  Per evaluation n, with F_i (zero on held components) and E_i of the
    interior images i = 1 ... K:
        t_i = mic(R_i - R_(i-1)), i = 1 ... K + 1          per atom d - rint(d h^-1) h in the periodic directions
        imax = the interior image of highest energy, the later one on a tie
        tau_i = t_(i+1) (i < imax),  t_i (i > imax),  t_i + t_(i+1) (i = imax)
        G_i = F_i - (F_i.tau_i / tau_i^2) tau_i - (((k t_i - k t_(i+1)).tau_i) / tau_i^2) tau_i
        climb, i = imax:  G_i = F_i - 2 (F_i.tau_i / tau_i^2) tau_i
    every dot a combination of the five sums F.t_i, F.t_(i+1), t_i.t_i, t_(i+1).t_(i+1), t_i.t_(i+1) of the image (each through
    _device_order_sum in the library's species-sorted order; `species`: the model's table), G_i = (F_i - ca_i t_i) - cb_i t_(i+1)
    with c = ft / tt + spr / tt (climbing: 2 ft / tt); held components of G are zero, their velocity is 0 and their coordinate
    keeps its bits.  FIRE runs over the concatenated K N rows: G.v, G.G, v.v per image in that order, the images added in the
    order 1 ... K; one dt, a, nsteps and maxstep scale; converged when max |G_row|^2 over all rows < fmax^2.
      reset_at: evaluation indices in front of which the optimizer is re-initialised.  update(out): called with every
    evaluation's dict before anything moves; a true return means the model behind `calc` has been dealt with (the covloss gate
    of the device loop and calculate() behind it): the same band is evaluated again — the repeat is not offered to update — behind
    optimizer.initialize() when the return is the string "reset".
      Yields a dict per evaluation: n, energies [K], covmax [K], imax and cimg (1 ... K: highest energy, largest covloss — the
    earlier image on a tie), gmax2, P (0 for a first evaluation), dt and a as used for the move out of this band (as they stand
    when it has converged), converged, band [K, N, 3] (a copy), forces [K, N, 3] (the model's), G [K, N, 3], velocities [K, N, 3] (FIRE's, in front of the move)."""
    from .ase_shim import Atoms, constraints_from_mask
    p = dict(FIRE_DEFAULTS)
    p.update(fire)
    R = np.array(images, float)
    K, N = len(R) - 2, len(numbers)
    if K < 1 or K > NEB_MAX:
        raise ValueError(f"neb: {K} interior images; a band has 1 to {NEB_MAX}")
    neb_check_band(R, cell, pbc)
    h, hi, pb = _neb_cell(cell, pbc)
    k = float(k)
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    fx = fixed_mask(fixed, N)
    cons = constraints_from_mask(fx)
    v = np.zeros((K, N, 3))
    dt, a, nsteps, fresh = float(p["dt"]), float(p["astart"]), 0, True
    fmax2 = float(fmax) * float(fmax)

    def dot(u, w):
        t = u * w
        return _device_order_sum(((t[:, 0] + t[:, 1]) + t[:, 2])[order])

    n, repeat = 0, False
    while n <= evals:
        if n in reset_at and not repeat:
            v = np.zeros((K, N, 3))
            dt, a, nsteps, fresh = float(p["dt"]), float(p["astart"]), 0, True
        F, E, cov = np.zeros((K, N, 3)), [0.0] * K, [0.0] * K
        for i in range(K):
            at = Atoms(numbers, R[i + 1].copy(), np.array(h), pbc, constraint=cons)
            at.calc = calc
            F[i] = np.asarray(at.get_forces(apply_constraint=False), float)
            E[i] = float(at.get_potential_energy())
            c = np.asarray(calc.get_covloss(), float)
            cov[i] = float(c.max()) if c.size else 0.0
        Fm = F if fx is None else np.where(fx[None], 0.0, F)
        t = [_neb_mic(R[i] - R[i - 1], h, hi, pb) for i in range(1, K + 2)]       # t[i - 1] = t_i
        imax = 0
        for i in range(1, K):
            if E[i] >= E[imax]:
                imax = i
        cimg = 0
        for i in range(1, K):
            if cov[i] > cov[cimg]:
                cimg = i
        G = np.zeros((K, N, 3))
        for i in range(K):
            ti, tn = t[i], t[i + 1]
            s = [dot(Fm[i], ti), dot(Fm[i], tn), dot(ti, ti), dot(tn, tn), dot(ti, tn)]
            if i < imax:
                ft, tt, spr = s[1], s[3], k * s[4] - k * s[3]
            elif i > imax:
                ft, tt, spr = s[0], s[2], k * s[2] - k * s[4]
            else:
                ft, tt, spr = s[0] + s[1], (s[2] + 2.0 * s[4]) + s[3], k * (s[2] + s[4]) - k * (s[4] + s[3])
            c = (2.0 * ft) / tt if (climb and i == imax) else ft / tt + spr / tt
            ca, cb = (0.0 if i < imax else c), (0.0 if i > imax else c)
            G[i] = (Fm[i] - ca * ti) - cb * tn
        if fx is not None:
            G = np.where(fx[None], 0.0, G)
        g2 = G * G
        g2 = (g2[..., 0] + g2[..., 1]) + g2[..., 2]
        gmax2 = max(0.0, float(g2.max()))
        Gv = GG = vv = 0.0
        for i in range(K):
            Gv = Gv + dot(G[i], v[i])
            GG = GG + dot(G[i], G[i])
            vv = vv + dot(v[i], v[i])
        P = 0.0 if fresh else Gv
        out = dict(n=n, energies=np.array(E), covmax=np.array(cov), imax=imax + 1, cimg=cimg + 1, gmax2=gmax2, P=P, band=R[1:-1].copy(),
                   forces=F, G=G, velocities=v.copy(), dt=dt, a=a, converged=False)
        if update is not None and not repeat:
            what = update(out)
            if what:
                if what == "reset":
                    v = np.zeros((K, N, 3))
                    dt, a, nsteps, fresh = float(p["dt"]), float(p["astart"]), 0, True
                repeat = True
                continue
        repeat = False
        if gmax2 < fmax2:
            out.update(converged=True)
            yield out
            return
        if fresh:
            alpha, beta = 0.0, dt
            fresh = False
            vv = 0.0
        elif P > 0.0:
            alpha = 1.0 - a
            gamma = (a * np.sqrt(vv)) / np.sqrt(GG)
            if nsteps > p["nmin"]:
                dt = min(dt * p["finc"], p["dtmax"])
                a = a * p["fa"]
            nsteps += 1
            beta = gamma + dt
        else:
            alpha, a, nsteps = 0.0, float(p["astart"]), 0
            dt = dt * p["fdec"]
            beta = dt
            vv = 0.0
        nv2 = ((alpha * alpha) * vv + (2.0 * (alpha * beta)) * P) + (beta * beta) * GG
        drn = dt * float(np.sqrt(nv2))
        cd = dt * (p["maxstep"] / drn) if drn > p["maxstep"] else dt
        out.update(dt=dt, a=a)
        yield out
        v = alpha * v + beta * G
        if fx is None:
            R[1:-1] = R[1:-1] + cd * v
        else:   # (selected, not computed)
            v = np.where(fx[None], 0.0, v)
            R[1:-1] = np.where(fx[None], R[1:-1], R[1:-1] + cd * v)
        n += 1


# ---- path-integral MD: a ring polymer under BAOAB with the PILE-L thermostat in the device's operations (pimd_baoab; md_pimd.inc:
# md_pimd_sums_kernel, md_pimd_gate_kernel and md_pimd_move_kernel)
PIMD_MAX = 32   # beads of a polymer


def pimd_tables(P, kT, dt, friction, pile_lambda):
    """The tables of a polymer run as sgpr_md_pimd computes them, once, on the host — scalar by scalar through the C library's
    sqrt, cos, sin and exp (the math module), in its operations: C [P, P], the orthonormal real DFT of the PILE paper's eq. 18
    (column 0: sqrt(1/P); 1 <= k < P/2: sqrt(2/P) cos(2 pi jk / P); k = P/2: sqrt(1/P) (-1)^j; k > P/2: sqrt(2/P) sin(2 pi jk / P),
    the argument reduced: jk mod P), w_k = 2 w_P sin(k pi / P) with w_P = P kT / hbar, the free ring polymer's propagator over
    dt / 2 — cs = cos(w_k dt/2), sn = sin(w_k dt/2) / w_k (k = 0: dt/2), wsn = w_k sin(w_k dt/2) — and the thermostat's
    c1_k = exp(-gamma_k dt), c2_k = sqrt(1 - c1_k^2) with gamma_0 = friction, gamma_k = 2 pile_lambda w_k."""
    import math
    dP, hdt = float(P), 0.5 * dt
    wP = (dP * kT) / HBAR
    C = np.zeros((P, P))
    for j in range(P):
        for k in range(P):
            arg = (2.0 * math.pi * float((j * k) % P)) / dP
            if k == 0:
                c = math.sqrt(1.0 / dP)
            elif 2 * k < P:
                c = math.sqrt(2.0 / dP) * math.cos(arg)
            elif 2 * k == P:
                c = -math.sqrt(1.0 / dP) if j & 1 else math.sqrt(1.0 / dP)
            else:
                c = math.sqrt(2.0 / dP) * math.sin(arg)
            C[j, k] = c
    w, cs, sn, wsn, c1, c2 = (np.zeros(P) for _ in range(6))
    for k in range(P):
        w[k] = (2.0 * wP) * math.sin((float(k) * math.pi) / dP) if k else 0.0
        s = math.sin(w[k] * hdt)
        cs[k] = math.cos(w[k] * hdt)
        sn[k] = s / w[k] if k else hdt
        wsn[k] = w[k] * s
        g = (2.0 * pile_lambda) * w[k] if k else friction
        c1[k] = math.exp(-(g * dt))
        c2[k] = math.sqrt(1.0 - c1[k] * c1[k])
    return dict(C=C, w=w, cs=cs, sn=sn, wsn=wsn, c1=c1, c2=c2, wP=wP)


def _pimd_modes(C, a, inverse=False):
    """a [P, N, 3] to normal modes, out_k = sum_j C[j][k] a_j (inverse: out_j = sum_k C[j][k] a_k), every sum sequentially in
    the order 0, 1, ..., P - 1: s = C a_0; s = s + C a_q."""
    M = C if inverse else C.T    # M[o][q]: the coefficient of input q in output o
    s = M[:, 0][:, None, None] * a[0][None]
    for q in range(1, len(a)):
        s = s + M[:, q][:, None, None] * a[q][None]
    return s


def _pimd_free(tb, hdt, x, v):
    """A(dt / 2): the exact free ring polymer in normal modes — mode 0 drifts, mode k >= 1 rotates."""
    cs, sn, wsn = (tb[q][:, None, None] for q in ("cs", "sn", "wsn"))
    xa, va = cs * x + sn * v, cs * v - wsn * x
    xa[0], va[0] = x[0] + hdt * v[0], v[0]
    return xa, va


def pimd_baoab(calc, numbers, beads, cell, pbc, steps, temperature=600.0, dt_fs=1.0, friction=1e-3, pile_lambda=1.0, vel=None, rng=None, seed=1,
               masses=None, species=None, noise=None, update=None):
    """Path-integral MD in numpy around any calculator with the ASE surface (forces and energy through the atoms; calc.get_covloss()
    where it has one), one call per bead per evaluation: a ring polymer of P beads (beads [P, N, 3], raw coordinates, no minimum
    image in the springs) at the physical temperature T, sampled at kT_P = P kB T with w_P = kT_P / hbar,
        H_P = sum_j sum_i [ m_i v_ij^2 / 2 + m_i w_P^2 / 2 |x_ij - x_i,j+1|^2 ] + sum_j V(x_j),
    integrated by BAOAB with the PILE-L thermostat (Ceriotti, Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104; Liu,
    Li, Liu, J. Chem. Phys. 145, 024103) — the host twin of the device loop (sgpr_md_pimd: md_pimd.inc) in its operations and
    summation order, bit for bit, and the definition.  By evaluation index n, behind the forces F_n of every bead: the closing half
    kick of step n - 1 (not at the start), the opening half kick v += (dt/2) F_n / m, to normal modes (pimd_tables' C), A(dt/2),
    O: v~_k <- c1_k v~_k + c2_k sqrt(kT_P / m) xi, A(dt/2), and back.  friction: the centroid's gamma_0; gamma_k = 2 pile_lambda w_k
    (friction = 0 with pile_lambda = 1/2: TRPMD, with 0: microcanonical RPMD).  At P = 1 (C = 1) this is langevin_nvt's loop,
    operation for operation, on the same random stream.
      vel [P, N, 3]: the beads' velocities (None: Maxwell-Boltzmann at P T from rng, the mean momentum of every bead removed);
    one rng.normal(size=(P, N, 3)) per step (mode k, atom, component) — or noise(n): the deviates that move evaluation n on;
    masses: [N] (None: the MASS table); species: the model's table (the order of the sums over atoms: species-sorted, stable).
    update(out): called with every evaluation's dict before anything moves; a true return means the model behind `calc` has
    been dealt with (the covloss gate of the device loop and calculate() behind it): the same configuration is evaluated again
    — the repeat is not offered to update.
      Yields a dict per evaluation n = 0 ... steps: n, energy (the mean of the beads'), energies [P], covmax [P], cbead (1 ... P:
    the largest covloss, the earlier bead on a tie), mv2 and mv2_pre (sum m v^2 over all beads after | before the closing half
    kick), cv (the centroid-virial kinetic energy 3 N kT / 2 - (1 / 2P) sum (x - xbar).F), spring (the spring energy), beads,
    forces, velocities_pre and velocities (closed) [P, N, 3] (copies)."""
    from .ase_shim import Atoms, kB
    rng = np.random.default_rng(seed) if rng is None else rng
    R = np.array(beads, float)
    P, N = R.shape[0], len(numbers)
    if R.shape != (P, N, 3) or P < 1 or P > PIMD_MAX:
        raise ValueError(f"pimd: beads is [P, N, 3] with 1 <= P <= {PIMD_MAX} for N = {N} atoms, not {R.shape}")
    mass = (np.array([MASS[int(z)] for z in numbers]) if masses is None else np.asarray(masses, float)).reshape(N, 1)
    kT = kB * temperature
    dP = float(P)
    kTP = dP * kT
    dt = dt_fs * FS
    hdt = 0.5 * dt
    tb = pimd_tables(P, kT, dt, friction, pile_lambda)
    C = tb["C"]
    wP2 = tb["wP"] * tb["wP"]
    sq = np.sqrt(kTP / mass)
    if vel is None:
        vel = rng.normal(size=(P, N, 3)) * sq
        for j in range(P):
            vel[j] -= (mass * vel[j]).sum(0) / mass.sum()
    v = np.array(vel, float).reshape(P, N, 3)
    table = sorted(set(int(z) for z in numbers)) if species is None else [int(z) for z in species]
    order = np.argsort([table.index(int(z)) if int(z) in table else len(table) for z in numbers], kind="stable")
    m1 = mass[:, 0]

    def dsum(vals):
        return _device_order_sum(vals[order])

    def rows(u, w):
        t = u * w
        return (t[:, 0] + t[:, 1]) + t[:, 2]

    n, repeat = 0, False
    while n <= steps:
        F, E, cov = np.zeros((P, N, 3)), [0.0] * P, [0.0] * P
        for j in range(P):
            at = Atoms(numbers, R[j].copy(), np.array(cell, float), pbc, velocities=v[j], masses=m1)
            at.calc = calc
            F[j] = np.asarray(at.get_forces(apply_constraint=False), float)
            E[j] = float(at.get_potential_energy())
            c = np.asarray(calc.get_covloss(), float) if hasattr(calc, "get_covloss") else np.zeros(0)
            cov[j] = float(c.max()) if c.size else 0.0
        kick = (hdt * F) / mass
        vc = v + kick if n > 0 else v       # closes step n - 1: the velocity an observer sees at evaluation n
        xbar = R[0]
        for j in range(1, P):
            xbar = xbar + R[j]
        xbar = xbar / dP
        Es, kc, kp, cv, sp = E[0], 0.0, 0.0, 0.0, 0.0
        cbead = 0
        for j in range(P):
            if j:
                Es = Es + E[j]
                if cov[j] > cov[cbead]:
                    cbead = j
            d, e = R[j] - xbar, R[j] - R[(j + 1) % P]
            # (the device combines the beads from the first one: x = s_0, x = x + s_j)
            parts = (dsum(m1 * rows(vc[j], vc[j])), dsum(m1 * rows(v[j], v[j])), dsum(rows(d, F[j])), dsum(m1 * rows(e, e)))
            kc, kp, cv, sp = parts if j == 0 else (kc + parts[0], kp + parts[1], cv + parts[2], sp + parts[3])
        out = dict(n=n, energy=Es / dP, energies=np.array(E), covmax=np.array(cov), cbead=cbead + 1, mv2=kc, mv2_pre=kp,
                   cv=(1.5 * float(N)) * kT - cv / (2.0 * dP), spring=(0.5 * wP2) * sp, beads=R.copy(), forces=F, velocities_pre=v.copy(),
                   velocities=np.array(vc))
        if update is not None and not repeat:
            if update(out):
                repeat = True
                continue
        repeat = False
        yield out
        if n == steps:
            return
        v2 = vc + kick                                                   # B
        xt, vt = _pimd_modes(C, R), _pimd_modes(C, v2)
        xt, vt = _pimd_free(tb, hdt, xt, vt)                             # A
        xi = rng.normal(size=(P, N, 3)) if noise is None else np.asarray(noise(n), float).reshape(P, N, 3)
        vt = tb["c1"][:, None, None] * vt + (tb["c2"][:, None, None] * sq[None]) * xi   # O
        xt, vt = _pimd_free(tb, hdt, xt, vt)                             # A
        R, v = _pimd_modes(C, xt, inverse=True), _pimd_modes(C, vt, inverse=True)
        n += 1


MSD_CHUNK = 256   # sorted atoms of one species per workgroup of md_msd_part_kernel (md_msd.inc)


def _block_order_sums(p):
    """_block_order_sum along the last axis of p[..., 256], every row at once: the same additions in the same order."""
    v = np.asarray(p, float).reshape(p.shape[:-1] + (4, 64))
    i = np.arange(64)
    v = v + v[..., i ^ 1]
    v = v + v[..., i ^ 2]
    v = v + v[..., (i & ~7) | (7 - (i & 7))]
    v = v + v[..., (i & ~15) | (15 - (i & 15))]
    w = (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


class MsdBlocks:
    """Mean-square displacements by blocked multiple origins — the host twin of the accumulator inside the device loop
    (SGPRModel.md_msd, md_msd.inc) and its definition: the same operations in the same order, so the two tables agree bit
    for bit.  What theforce/analysis/analysis.py:109-176 (`correlator`: the tracer msd mean_i |dr_i|^2 and the collective
    smd |sum_i dr_i|^2 / n of a species) works out of a stored trajectory, taken as the run goes.
      add(x) is fed the configurations 0, 1, 2, ... of a run ([N, 3], caller atom order, never wrapped).  Configuration n with
    n % every == 0 is sample s = n / every.  Level l < levels has the lag 2^l samples and keeps ONE origin O_l; at sample s
    every level with s mod 2^l == 0 measures, if s >= 2^l, d_i = x_i - O_l,i and then sets O_l <- x:
        c   = sum_all m_i d_i / sum_all m_i  (com; else 0)
        msd = ((A - 2 c.B) + n_z |c|^2) / n_z,  A = sum_z |d_i|^2,  B = sum_z d_i      (mean |d_i - c|^2)
        smd = |B - n_z c|^2 / n_z
    per species z of `species` (the model's table; one absent from the frame keeps zeros); the row (l, z) gains msd, msd^2, smd,
    smd^2 and count[l] gains 1.  The windows of a level do not overlap: its samples are independent blocks.
      Order: atoms sorted by species (stable), a species cut into chunks of MSD_CHUNK atoms; per chunk the seven sums A, B, sum m d
    in the workgroup's order (_block_order_sum, one atom per thread, the per-atom term (d0 d0 + d1 d1) + d2 d2); the chunks of a
    species ascending; sum m d over the species in table order; the total mass atom by atom in sorted order."""

    def __init__(self, every, levels, com, masses, numbers, species):
        if every < 1 or not 1 <= levels <= 32:
            raise ValueError("MsdBlocks: every >= 1, 1 <= levels <= 32")
        self.every, self.levels, self.com = int(every), int(levels), bool(com)
        numbers = np.asarray(numbers)
        self.species = [int(z) for z in species]
        zi = np.array([self.species.index(int(z)) for z in numbers])
        self.perm = np.argsort(zi, kind="stable")
        self.nz = np.array([int(np.sum(zi == z)) for z in range(len(self.species))])
        self.mass = np.asarray(masses, float)[self.perm]
        self.mtot = 0.0
        for v in self.mass:
            self.mtot = self.mtot + float(v)
        self.chunks, first = [], 0   # (species, first atom, atoms)
        for z, nz in enumerate(self.nz):
            self.chunks += [(z, first + o, min(MSD_CHUNK, nz - o)) for o in range(0, nz, MSD_CHUNK)]
            first += nz
        self.origin = [None] * self.levels
        self.count = np.zeros(self.levels, dtype=np.int64)
        self.sums = np.zeros((self.levels, len(self.species), 4))
        self.n = 0   # configurations seen

    def _measure(self, l, x):
        d = x - self.origin[l]
        terms = np.concatenate([((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None], d, self.mass[:, None] * d], axis=1)
        pad = np.zeros((len(self.chunks), 7, MSD_CHUNK))
        for c, (_, a, k) in enumerate(self.chunks):
            pad[c, :, :k] = terms[a:a + k].T
        part = _block_order_sums(pad)   # [chunks, 7]
        S = len(self.species)
        sums = np.zeros((S, 7))
        for c, (z, _, _) in enumerate(self.chunks):
            sums[z] = sums[z] + part[c]
        cm = np.zeros(3)
        if self.com:
            for z in range(S):
                cm = cm + sums[z, 4:7]
            cm = cm / self.mtot
        for z in range(S):
            if self.nz[z] == 0:
                continue
            fn, A, B = float(self.nz[z]), sums[z, 0], sums[z, 1:4]
            cB = (cm[0] * B[0] + cm[1] * B[1]) + cm[2] * B[2]
            cc = (cm[0] * cm[0] + cm[1] * cm[1]) + cm[2] * cm[2]
            msd = ((A - 2.0 * cB) + fn * cc) / fn
            e = B - fn * cm
            smd = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / fn
            self.sums[l, z] = self.sums[l, z] + np.array([msd, msd * msd, smd, smd * smd])
        self.count[l] += 1

    def add(self, positions):
        """The next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        s = n // self.every
        x = np.asarray(positions, float).reshape(-1, 3)[self.perm]
        for l in range(self.levels):
            if s % (1 << l):
                break
            if s >= (1 << l):
                self._measure(l, x)
            self.origin[l] = x.copy()

    def table(self):
        """What SGPRModel.md_msd_table returns."""
        return dict(lags=self.every * 2 ** np.arange(self.levels, dtype=np.int64), count=self.count.copy(), msd=self.sums[:, :, 0].copy(),
                    msd_sq=self.sums[:, :, 1].copy(), smd=self.sums[:, :, 2].copy(), smd_sq=self.sums[:, :, 3].copy(),
                    species=np.array(self.species), n=self.nz.copy(), samples=-(-self.n // self.every), next_due=-(-self.n // self.every) * self.every)


VACF_CHUNK = 256   # sorted atoms of one species per workgroup of md_vacf_store_kernel and md_vacf_corr_kernel (md_vacf.inc)


def observer_velocities(v_pre, F, mass, hdt, pending, fixed=None):
    """The velocities an observer of the trajectory sees at a configuration — what sgpr_md_velocities returns, operation for
    operation: v_pre + hdt * F / m where the closing half kick is due (pending: every configuration of a Langevin / velocity
    Verlet run but the first), v_pre as it is otherwise (pending = 0: configuration 0, and Nose-Hoover, whose v_pre is the
    centred velocity already); a held component (fixed [N, 3] bool) exactly 0.  [N, 3], caller atom order."""
    v = np.array(v_pre, float).reshape(-1, 3)
    if pending:
        v = v + float(hdt) * np.asarray(F, float).reshape(-1, 3) / np.asarray(mass, float)[:, None]
    if fixed is not None:
        v[np.asarray(fixed, bool).reshape(-1, 3)] = 0.0
    return v


class VacfRing:
    """Velocity autocorrelations over a ring of stored samples — the host twin of the accumulator inside the device loop
    (SGPRModel.md_vacf, md_vacf.inc) and its definition: the same operations in the same order, so the two tables agree bit for
    bit.  The reference has no velocity autocorrelation; the definition is ours.
      add(v) is fed the observer's velocities (observer_velocities) of the configurations 0, 1, 2, ... of a run ([N, 3], caller
    atom order).  Configuration n with n % every == 0 is sample s = n / every.  For every sample s, lag k < lags and origin
    o = s - k with o >= 0 and o % origin_every == 0, per species z of `species` (the model's table, n_z atoms in the frame; one
    absent from the frame keeps zeros), J_z(s) = sum_z v_i(s) and c_s = sum_all m_i v_i(s) / sum_all m_i (com; else 0):
        A            = sum_z ((v_i0(s) v_i0(o) + v_i1(s) v_i1(o)) + v_i2(s) v_i2(o))
        tr[k, z]    += ((A - (c_s.J_z(o) + c_o.J_z(s))) + n_z (c_s.c_o)) / n_z     (mean over z of (v_i(s) - c_s).(v_i(o) - c_o))
        col[k, a, b] += e_a(s).e_b(o),  e_z = J_z - n_z c
        count[k]    += 1
      A sample is taken in two parts, as the device must take it (a configuration behind a covloss halt is evaluated again, with
    other forces): add(v) STORES sample s in slot s % (lags + 1) of a ring — v and the chunk parts of J and sum m v — and
    CORRELATES sample s - 1, which is final: its J and c go into their own rings, its due lags are accumulated.  Sample 0 only
    stores; the last sample fed stays pending.
      Order: atoms sorted by species (stable), a species cut into chunks of VACF_CHUNK atoms; per chunk the block sums in the
    workgroup's order (_block_order_sums, one atom per thread); the chunks of a species ascending; sum m v over the species in
    table order; the total mass atom by atom in sorted order; dot products (a0 b0 + a1 b1) + a2 b2."""

    def __init__(self, every, lags, origin_every, com, masses, numbers, species):
        if every < 1 or lags < 1 or origin_every < 1:
            raise ValueError("VacfRing: every >= 1, lags >= 1, origin_every >= 1")
        self.every, self.lags, self.origin_every, self.com = int(every), int(lags), int(origin_every), bool(com)
        numbers = np.asarray(numbers)
        self.species = [int(z) for z in species]
        zi = np.array([self.species.index(int(z)) for z in numbers])
        self.perm = np.argsort(zi, kind="stable")
        self.nz = np.array([int(np.sum(zi == z)) for z in range(len(self.species))])
        self.mass = np.asarray(masses, float)[self.perm]
        self.mtot = 0.0
        for v in self.mass:
            self.mtot = self.mtot + float(v)
        self.chunks, first = [], 0   # (species, first atom, atoms)
        for z, nz in enumerate(self.nz):
            self.chunks += [(z, first + o, min(VACF_CHUNK, nz - o)) for o in range(0, nz, VACF_CHUNK)]
            first += nz
        S, self.slots = len(self.species), self.lags + 1
        self.ring = [None] * self.slots                    # v [N, 3] sorted
        self.vpart = [None] * self.slots                   # [chunks, 6]
        self.J = np.zeros((self.slots, S, 3))
        self.c = np.zeros((self.slots, 3))
        self.tr = np.zeros((self.lags, S))
        self.col = np.zeros((self.lags, S, S))
        self.count = np.zeros(self.lags, dtype=np.int64)
        self.samples = 0   # correlated
        self.n = 0         # configurations seen

    def _chunk_sums(self, terms):
        """terms [N, q] per sorted atom -> [chunks, q] in the workgroup's order."""
        pad = np.zeros((len(self.chunks), terms.shape[1], VACF_CHUNK))
        for c, (_, a, k) in enumerate(self.chunks):
            pad[c, :, :k] = terms[a:a + k].T
        return _block_order_sums(pad)

    def _species_sums(self, part):
        sums = np.zeros((len(self.species), part.shape[1]))
        for c, (z, _, _) in enumerate(self.chunks):
            sums[z] = sums[z] + part[c]
        return sums

    @staticmethod
    def _dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def _store(self, s, v):
        q = s % self.slots
        self.ring[q] = v
        self.vpart[q] = self._chunk_sums(np.concatenate([v, self.mass[:, None] * v], axis=1))

    def _correlate(self, p):
        S, qp = len(self.species), p % self.slots
        sums = self._species_sums(self.vpart[qp])
        cp = np.zeros(3)
        if self.com:
            for z in range(S):
                cp = cp + sums[z, 3:6]
            cp = cp / self.mtot
        self.J[qp], self.c[qp] = sums[:, :3], cp
        vp, Jp = self.ring[qp], self.J[qp]
        fn = self.nz.astype(float)
        ep = Jp - fn[:, None] * cp[None]
        for k in range(self.lags):
            o = p - k
            if o < 0:
                break
            if o % self.origin_every:
                continue
            qo = o % self.slots
            vo, Jo, co = self.ring[qo], self.J[qo], self.c[qo]
            A = self._species_sums(self._chunk_sums(((vp[:, 0] * vo[:, 0] + vp[:, 1] * vo[:, 1]) + vp[:, 2] * vo[:, 2])[:, None]))[:, 0]
            eo = Jo - fn[:, None] * co[None]
            cc = self._dot(cp, co)
            for a in range(S):
                for b in range(S):
                    self.col[k, a, b] = self.col[k, a, b] + self._dot(ep[a], eo[b])
                if self.nz[a] > 0:
                    self.tr[k, a] = self.tr[k, a] + ((A[a] - (self._dot(cp, Jo[a]) + self._dot(co, Jp[a]))) + fn[a] * cc) / fn[a]
            self.count[k] += 1
        self.samples += 1

    def add(self, velocities):
        """The observer's velocities of the next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        s = n // self.every
        self._store(s, np.array(velocities, float).reshape(-1, 3)[self.perm])
        if s > 0:
            self._correlate(s - 1)

    def table(self):
        """What SGPRModel.md_vacf_table returns."""
        due = -(-self.n // self.every)
        return dict(tracer=self.tr.copy(), collective=self.col.copy(), count=self.count.copy(),
                    lags=self.every * np.arange(self.lags, dtype=np.int64), species=np.array(self.species), n=self.nz.copy(),
                    samples=self.samples, pending=1 if due > 0 else 0, next_due=due * self.every)


SQ_MAXQ, SQ_MAXLAGS, SQ_MAXH = 8192, 8192, 32   # wave vectors, lags and |index| of a table (md_sq.inc)


def sq_vectors(hkl, cell):
    """q [nq, 3] = 2 pi hkl inv(cell)^T: the vectors of the reciprocal lattice that the integer triples name (q . r = 2 pi
    hkl . s for r = s cell)."""
    return 2.0 * np.pi * np.asarray(hkl, float).reshape(-1, 3) @ np.linalg.inv(np.asarray(cell, float).reshape(3, 3)).T


def sq_bounds(hmax, smax, nz, count):
    """The a-priori bounds the device accumulator (md_sq.inc) and SqRing are held to against each other and against any other
    evaluation in double precision: B [S] with |d rho_z(q)| <= B_z = 128 hmax (1 + smax) n_z 2^-52 (hmax: the largest |index|,
    smax: the largest |scaled coordinate| fed; a phase error of 2 pi (|h| + |k| + |l|) roundings of a three-term scaled
    coordinate, a few roundings per power, that much on both sides) and F [lags, S, S] with
    |d f[k, j, a, b]| <= count[k] (n_a B_b + n_b B_a + count[k] n_a n_b 2^-52)."""
    n = np.asarray(nz, float)
    c = np.asarray(count, float)[:, None, None]
    B = 128.0 * float(hmax) * (1.0 + float(smax)) * n * 2.0 ** -52
    return B, c * (n[:, None] * B[None, :] + n[None, :] * B[:, None] + c * n[:, None] * n[None, :] * 2.0 ** -52)


class SqRing:
    """Partial structure factors and coherent intermediate scattering functions over a ring of stored densities — the host twin of
    the accumulator inside the device loop (SGPRModel.md_sq, md_sq.inc) and its definition.  The reference has nothing in
    reciprocal space; the definition is ours.
      hkl: int [nq, 3], vectors of the reciprocal lattice of `cell`: q_j = 2 pi hkl_j inv(cell)^T, so q_j . r = 2 pi hkl_j . s
    with s = r inv(cell) — wrapped and unwrapped positions give the same phases.  One vector of each +- pair (the real part is the
    average over the pair); duplicates are not checked for.
      add(x) is fed the configurations 0, 1, 2, ... of a run ([N, 3], caller atom order, wrapped or not).  Configuration n with
    n % every == 0 is sample s = n / every.  Per atom f = s - rint(s) and e_a = exp(2 pi i f_a) per axis, the powers 0 ... hmax
    of e_a by repeated multiplication (a negative index: the conjugate), and per species z of `species` (the model's table; one
    absent from the frame keeps zeros)
        rho_z(q_j; s) = sum_{i in z} e_0^h e_1^k e_2^l
    For every lag k < lags and origin o = s - k with o >= 0 and o % origin_every == 0
        f[k, j, a, b] += Re(rho_a(q_j; s) conj rho_b(q_j; o)),  count[k] += 1      (the full block: a != b is not symmetric at k > 0)
    and per sample mean[j, a] += rho_a(q_j; s), samples += 1.  rho(s) is kept in slot s % lags of a ring.  Lag 0 is the static S_ab.
      The device's sincospi is not numpy's sin and cos: the two tables agree within sq_bounds, not bit for bit; count, samples and
    next_due are equal."""

    def __init__(self, every, hkl, lags, origin_every, numbers, species, cell, pbc):
        if every < 1 or lags < 1 or origin_every < 1:
            raise ValueError("SqRing: every >= 1, lags >= 1, origin_every >= 1")
        self.every, self.lags, self.origin_every = int(every), int(lags), int(origin_every)
        given = np.asarray(hkl)
        if given.ndim != 2 or given.shape[1] != 3 or not np.array_equal(given, np.rint(given)):
            raise ValueError("SqRing: hkl is an integer array [nq, 3]")
        self.hkl = given.astype(np.int64)
        pbc = np.broadcast_to(np.asarray(pbc, bool), (3,))
        if not 1 <= len(self.hkl) <= SQ_MAXQ or self.lags > SQ_MAXLAGS:
            raise ValueError(f"SqRing: 1 <= nq <= {SQ_MAXQ}, lags <= {SQ_MAXLAGS}")
        if np.any(np.all(self.hkl == 0, axis=1)) or np.abs(self.hkl).max() > SQ_MAXH or np.any(self.hkl[:, ~pbc] != 0):
            raise ValueError(f"SqRing: no zero row, every |index| <= {SQ_MAXH}, 0 along a direction that is not periodic")
        self.cell = np.asarray(cell, float).reshape(3, 3).copy()
        self.inv = rdf_geometry(self.cell, pbc, 1.0)[0]   # (sgpr_md_sq's inverse: frac_c = sum_k x_k inv[k, c])
        self.hmax = int(np.abs(self.hkl).max())
        numbers = np.asarray(numbers)
        self.species = [int(z) for z in species]
        self.idx = [np.flatnonzero(numbers == z) for z in self.species]
        self.nz = np.array([len(i) for i in self.idx])
        S, nq = len(self.species), len(self.hkl)
        self.ring = np.zeros((self.lags, nq, S), dtype=complex)
        self.f = np.zeros((self.lags, nq, S, S))
        self.mean = np.zeros((nq, S), dtype=complex)
        self.count = np.zeros(self.lags, dtype=np.int64)
        self.samples = 0
        self.n = 0         # configurations seen
        self.smax = 0.0    # the largest |scaled coordinate| fed: what the bound takes

    def density(self, positions):
        """rho [nq, S] of one configuration."""
        x = np.asarray(positions, float).reshape(-1, 3)
        inv = self.inv
        s = np.stack([(x[:, 0] * inv[0, c] + x[:, 1] * inv[1, c]) + x[:, 2] * inv[2, c] for c in range(3)], axis=1)
        if len(s):
            self.smax = max(self.smax, float(np.abs(s).max()))
        f = s - np.rint(s)
        e = np.cos(2.0 * np.pi * f) + 1j * np.sin(2.0 * np.pi * f)
        pw = np.ones((self.hmax + 1,) + e.shape, dtype=complex)   # [power, atom, axis]
        for p in range(1, self.hmax + 1):
            pw[p] = pw[p - 1] * e
        rho = np.zeros((len(self.hkl), len(self.species)), dtype=complex)
        fac = []
        for ax in range(3):
            t = pw[np.abs(self.hkl[:, ax]), :, ax]   # [nq, atom]
            fac.append(np.where((self.hkl[:, ax] < 0)[:, None], np.conj(t), t))
        prod = (fac[0] * fac[1]) * fac[2]
        for z, i in enumerate(self.idx):
            if len(i):
                rho[:, z] = prod[:, i].sum(axis=1)
        return rho

    def add(self, positions):
        """The next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        s = n // self.every
        rho = self.density(positions)
        self.ring[s % self.lags] = rho
        self.mean += rho
        for k in range(self.lags):
            o = s - k
            if o < 0:
                break
            if o % self.origin_every:
                continue
            org = self.ring[o % self.lags]
            self.f[k] += (rho[:, :, None] * np.conj(org)[:, None, :]).real
            self.count[k] += 1
        self.samples += 1

    def table(self):
        """What SGPRModel.md_sq_table returns."""
        return dict(f=self.f.copy(), mean=self.mean.copy(), count=self.count.copy(), lags=self.every * np.arange(self.lags, dtype=np.int64),
                    hkl=self.hkl.copy(), q=sq_vectors(self.hkl, self.cell), species=np.array(self.species), n=self.nz.copy(),
                    origin_every=self.origin_every, samples=self.samples, next_due=-(-self.n // self.every) * self.every)


RDF_MAXR = 2      # images |s_k| <= 2 around a pair's nearest one: at most 125 shifts (md_rdf.inc)
RDF_MAXBINS = 2048


def rdf_geometry(cell, pbc, rmax):
    """What sgpr_md_rdf works out of the run's cell at the attach, operation for operation: (inv [3, 3] with frac_c = sum_k
    x_k inv[k, c], by the cofactor formula of nl_make_grid; volume |det|; heights [3] = V / |cross|; R [3] = floor(rmax /
    height_k + 1/2), 0 along an open direction — every image of a pair that can come within rmax lies within R of its nearest)."""
    h = [[float(v) for v in row] for row in np.asarray(cell, float).reshape(3, 3)]
    p, q, r = h
    dt = p[0] * (q[1] * r[2] - q[2] * r[1]) - p[1] * (q[0] * r[2] - q[2] * r[0]) + p[2] * (q[0] * r[1] - q[1] * r[0])
    if not abs(dt) > 1e-12:
        raise ValueError("rdf_geometry: the cell has no volume; densities need one")
    bc = [q[1] * r[2] - q[2] * r[1], q[2] * r[0] - q[0] * r[2], q[0] * r[1] - q[1] * r[0]]
    ca = [r[1] * p[2] - r[2] * p[1], r[2] * p[0] - r[0] * p[2], r[0] * p[1] - r[1] * p[0]]
    ab = [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
    inv = np.array([[bc[k] / dt, ca[k] / dt, ab[k] / dt] for k in range(3)])
    V = abs(dt)
    heights = np.array([V / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) for c in (bc, ca, ab)])
    R = np.array([int(np.floor(float(rmax) / heights[k] + 0.5)) if pbc[k] else 0 for k in range(3)])
    return inv, V, heights, R


class RdfCounts:
    """Pair-distance histograms per species pair — the host twin of the accumulator inside the device loop (SGPRModel.md_rdf,
    md_rdf.inc) and its definition; the counts are integers, so the two tables are equal.  What theforce/analysis/rdf.py's
    `rdf` takes from every atom's neighbour list at cutoff rmax, from the configurations as the run goes.
      add(x) is fed the configurations 0, 1, 2, ... of a run ([N, 3], caller atom order, wrapped or not); those with n % every
    == 0 are samples.  For a sample, species slots a, b of `species` (the model's table) and k < bins, hist[a, b, k] gains the
    number of triples (i of a, j of b, s in Z^3) with (j, s) != (i, 0) — periodic self-images count — and
        d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),  r = sqrt((d0 d0 + d1 d1) + d2 d2),  rmin <= r < rmax,
        k = (int)(((r - rmin) / (rmax - rmin)) bins)   (torch.histc's rule; a quotient that rounds up to `bins`: the last bin)
    with s = 0 along an open direction.  Enumeration: a pair goes to its nearest image by n_k = rint((dx0 inv[0, k] + dx1
    inv[1, k]) + dx2 inv[2, k]) (rdf_geometry's inverse), then s = t - n over the block |t_k| <= R_k.  d depends on (i, j, s)
    alone: brute force over all pairs here, tiles on the device, the same integers.  hist[b, a] = hist[a, b] exactly (i <-> j
    negates every intermediate), so a <= b is swept and the table filled out."""

    def __init__(self, every, rmax, bins, rmin, numbers, species, cell, pbc):
        if every < 1 or not 1 <= bins <= RDF_MAXBINS or not 0.0 <= rmin < rmax:
            raise ValueError(f"RdfCounts: every >= 1, 1 <= bins <= {RDF_MAXBINS}, 0 <= rmin < rmax")
        self.every, self.bins, self.rmin, self.rmax = int(every), int(bins), float(rmin), float(rmax)
        self.h = np.asarray(cell, float).reshape(3, 3).copy()
        self.pbc = np.broadcast_to(np.asarray(pbc, bool), (3,)).copy()
        self.inv, self.volume, self.heights, self.R = rdf_geometry(self.h, self.pbc, self.rmax)
        for k in range(3):
            if self.R[k] > RDF_MAXR:
                raise NotImplementedError(f"RdfCounts: rmax = {self.rmax:g} against the cell height {self.heights[k]:g} along direction {k} needs "
                                          f"images {self.R[k]} cells away; at most {RDF_MAXR} (125 shifts)")
        numbers = np.asarray(numbers)
        self.species = [int(z) for z in species]
        self.idx = [np.flatnonzero(numbers == z) for z in self.species]
        self.nz = np.array([len(i) for i in self.idx])
        self.hist = np.zeros((len(self.species), len(self.species), self.bins), dtype=np.uint64)
        self.n = 0   # configurations seen

    def _pairs(self, xi, xj, same):
        """The counts [bins] of the i-atoms xi against the j-atoms xj (same: they are one list, (j, 0) == (i, 0) stays out)."""
        h, inv, out = self.h, self.inv, np.zeros(self.bins, dtype=np.int64)
        width, fbins = self.rmax - self.rmin, float(self.bins)
        for o in range(0, len(xi), 256):
            dx = xj[None, :, :] - xi[o:o + 256, None, :]
            dx0, dx1, dx2 = dx[..., 0], dx[..., 1], dx[..., 2]
            n = [np.rint((dx0 * inv[0, k] + dx1 * inv[1, k]) + dx2 * inv[2, k]) if self.pbc[k] else np.zeros_like(dx0) for k in range(3)]
            for t0 in range(-self.R[0], self.R[0] + 1):
                for t1 in range(-self.R[1], self.R[1] + 1):
                    for t2 in range(-self.R[2], self.R[2] + 1):
                        s0, s1, s2 = float(t0) - n[0], float(t1) - n[1], float(t2) - n[2]
                        d0 = dx0 + ((s0 * h[0, 0] + s1 * h[1, 0]) + s2 * h[2, 0])
                        d1 = dx1 + ((s0 * h[0, 1] + s1 * h[1, 1]) + s2 * h[2, 1])
                        d2 = dx2 + ((s0 * h[0, 2] + s1 * h[1, 2]) + s2 * h[2, 2])
                        r = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
                        ok = (r >= self.rmin) & (r < self.rmax)
                        if same and t0 == 0 and t1 == 0 and t2 == 0:
                            rows = np.arange(dx.shape[0])
                            ok[rows, o + rows] = False
                        k = np.minimum((((r[ok] - self.rmin) / width) * fbins).astype(np.int64), self.bins - 1)
                        out += np.bincount(k, minlength=self.bins)
        return out

    def add(self, positions):
        """The next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        x = np.asarray(positions, float).reshape(-1, 3)
        for a in range(len(self.species)):
            for b in range(a, len(self.species)):
                if self.nz[a] and self.nz[b]:
                    c = self._pairs(x[self.idx[a]], x[self.idx[b]], a == b).astype(np.uint64)
                    self.hist[a, b] += c
                    if b != a:
                        self.hist[b, a] += c

    def table(self):
        """What SGPRModel.md_rdf_table returns."""
        samples = -(-self.n // self.every)
        return dict(hist=self.hist.copy(), species=np.array(self.species), n=self.nz.copy(), samples=samples, next_due=samples * self.every,
                    every=self.every, bins=self.bins, rmin=self.rmin, rmax=self.rmax, volume=self.volume)


ADF_MAXCOORD = 64    # coordination numbers 0 ... 62, and 63 and above (md_adf.inc)
ADF_MAXBINS = 1024


def adf_edges(bins):
    """The edges of the angle bins as the comparisons take them: ct [bins] = cos(e pi / bins) (entry 0 is never compared).  Made
    here once, with numpy; SGPRModel.md_adf uploads these doubles and AdfCounts compares with the same ones."""
    return np.cos(np.arange(int(bins), dtype=float) * np.pi / float(bins))


def adf_cutoffs(cutoffs, species):
    """The table cut [S, S] over the slots of `species` from a scalar (all pairs) or a dict {(Z1, Z2): r} (either order; pairs
    that are absent never bond: 0)."""
    S = len(species)
    if isinstance(cutoffs, dict):
        slot = {int(z): k for k, z in enumerate(species)}
        cut = np.zeros((S, S))
        for (z1, z2), r in cutoffs.items():
            if int(z1) not in slot or int(z2) not in slot:
                raise ValueError(f"adf_cutoffs: the pair ({z1}, {z2}) names a species outside the model's table {list(species)}")
            a, b = slot[int(z1)], slot[int(z2)]
            if (int(z2), int(z1)) in cutoffs and float(cutoffs[(int(z2), int(z1))]) != float(r):
                raise ValueError(f"adf_cutoffs: ({z1}, {z2}) and ({z2}, {z1}) differ")
            cut[a, b] = cut[b, a] = float(r)
        return cut
    cut = np.array(cutoffs, dtype=float)
    return np.full((S, S), float(cut)) if cut.ndim == 0 else cut.reshape(S, S).copy()


class AdfCounts:
    """Bond-angle and coordination distributions per species triple — the host twin of the accumulator inside the device loop
    (SGPRModel.md_adf, md_adf.inc) and its definition (the reference has no angular analysis); all entries are integer counts,
    so the two sets of tables are equal.
      add(x) is fed the configurations 0, 1, 2, ... of a run ([N, 3], caller atom order, wrapped or not); those with n % every
    == 0 are samples.  cut [S, S] is the symmetric table of bond cutoffs over the slots of `species` (the model's table; 0: the
    pair never bonds).  For a sample and a centre i of species a, its neighbours are all (j of species b, s in Z^3) with (j, s)
    != (i, 0) — periodic self-images and several images of one atom are distinct neighbours — and
        d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),  r = sqrt((d0 d0 + d1 d1) + d2 d2),  r < cut[a, b]
    with s = 0 along an open direction, enumerated as RdfCounts does: nearest image by rint, then the block |t_k| <= R_k for the
    largest cutoff.  For every unordered pair {t, t'} of distinct neighbours, species b <= c after ordering,
        q = (d_t0 d_t'0 + d_t1 d_t'1) + d_t2 d_t'2,  p = r_t r_t',  k = #{e in 1 ... bins - 1 : q <= ct[e] p},  angles[a, b, c, k] += 1
    with ct = adf_edges(bins): no arccos, no division (bin k holds the angles in [k pi / bins, (k + 1) pi / bins): an angle on
    an edge belongs to the bin above it).  And for every species b, n_ib the neighbours of i of species b:
    coord[a, b, min(n_ib, ADF_MAXCOORD - 1)] += 1.  table() fills angles[a, c, b] = angles[a, b, c]."""

    def __init__(self, every, bins, cut, numbers, species, cell, pbc, ct=None):
        if every < 1 or not 1 <= bins <= ADF_MAXBINS:
            raise ValueError(f"AdfCounts: every >= 1, 1 <= bins <= {ADF_MAXBINS}")
        self.every, self.bins = int(every), int(bins)
        self.species = [int(z) for z in species]
        S = len(self.species)
        self.cut = adf_cutoffs(cut, self.species)
        if not (np.all(self.cut >= 0.0) and np.all(np.isfinite(self.cut)) and np.array_equal(self.cut, self.cut.T)):
            raise ValueError("AdfCounts: the cutoff table must be symmetric and >= 0")
        if not self.cut.max() > 0.0:
            raise ValueError("AdfCounts: every cutoff is 0: no pair bonds")
        self.ct = adf_edges(self.bins) if ct is None else np.asarray(ct, float).copy()
        self.h = np.asarray(cell, float).reshape(3, 3).copy()
        self.pbc = np.broadcast_to(np.asarray(pbc, bool), (3,)).copy()
        if self.pbc.any():
            # (an open direction of a cell without volume: any vector that gives one serves, it is never a shift)
            self.inv, _, self.heights, self.R = rdf_geometry(self.h, self.pbc, float(self.cut.max()))
        else:
            self.inv, self.R = np.zeros((3, 3)), np.zeros(3, dtype=int)
        for k in range(3):
            if self.R[k] > 127:
                raise NotImplementedError(f"AdfCounts: a cutoff of {self.cut.max():g} needs images {self.R[k]} cells away along direction {k}")
        self.block = np.array([[float(t0), float(t1), float(t2)] for t0 in range(-self.R[0], self.R[0] + 1)
                               for t1 in range(-self.R[1], self.R[1] + 1) for t2 in range(-self.R[2], self.R[2] + 1)])
        self.block0 = int(np.flatnonzero(np.all(self.block == 0.0, axis=1))[0])
        numbers = np.asarray(numbers)
        self.slot = np.full(len(numbers), -1)
        for k, z in enumerate(self.species):
            self.slot[numbers == z] = k
        if (self.slot < 0).any():
            raise ValueError("AdfCounts: an atom's species is not in the table")
        self.nz = np.array([int(np.sum(self.slot == k)) for k in range(S)])
        self.angles = np.zeros((S, S, S, self.bins), dtype=np.uint64)   # b <= c filled
        self.coord = np.zeros((S, S, ADF_MAXCOORD), dtype=np.uint64)
        self.n = 0   # configurations seen

    def neighbours(self, x, i):
        """(d [T, 3], r [T], b [T]) of centre i in the configuration x: the definition's neighbours, in the order (image, atom)."""
        h, inv, a = self.h, self.inv, self.slot[i]
        dx = x - x[i]
        dx0, dx1, dx2 = dx[:, 0], dx[:, 1], dx[:, 2]
        n = [np.rint((dx0 * inv[0, k] + dx1 * inv[1, k]) + dx2 * inv[2, k]) if self.pbc[k] else np.zeros_like(dx0) for k in range(3)]
        cutj = self.cut[a][self.slot]
        # the block of images, all at once: t [M, 1] against the atoms [N]
        t = self.block
        s0, s1, s2 = t[:, 0:1] - n[0][None, :], t[:, 1:2] - n[1][None, :], t[:, 2:3] - n[2][None, :]
        d0 = dx0[None, :] + ((s0 * h[0, 0] + s1 * h[1, 0]) + s2 * h[2, 0])
        d1 = dx1[None, :] + ((s0 * h[0, 1] + s1 * h[1, 1]) + s2 * h[2, 1])
        d2 = dx2[None, :] + ((s0 * h[0, 2] + s1 * h[1, 2]) + s2 * h[2, 2])
        r = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
        ok = r < cutj[None, :]
        ok[self.block0, i] = False   # (i, 0) is the centre itself
        return np.stack([d0[ok], d1[ok], d2[ok]], axis=1), r[ok], np.broadcast_to(self.slot[None, :], ok.shape)[ok]

    def add(self, positions):
        """The next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        x = np.asarray(positions, float).reshape(-1, 3)
        S, bins, edges = len(self.species), self.bins, self.ct[1:]
        for i in range(len(x)):
            a = self.slot[i]
            d, r, b = self.neighbours(x, i)
            nib = np.bincount(b, minlength=S)
            for s in range(S):
                self.coord[a, s, min(int(nib[s]), ADF_MAXCOORD - 1)] += np.uint64(1)
            if len(r) < 2:
                continue
            t, u = np.triu_indices(len(r), 1)
            q = (d[t, 0] * d[u, 0] + d[t, 1] * d[u, 1]) + d[t, 2] * d[u, 2]
            p = r[t] * r[u]
            k = np.zeros(len(q), dtype=np.int64)
            for o in range(0, len(q), 4096):   # (the linear count, a block of pairs at a time)
                k[o:o + 4096] = np.sum(q[o:o + 4096, None] <= edges[None, :] * p[o:o + 4096, None], axis=1)
            lo, hi = np.minimum(b[t], b[u]), np.maximum(b[t], b[u])
            flat = np.bincount((lo * S + hi) * bins + k, minlength=S * S * bins).astype(np.uint64)
            self.angles[a] += flat.reshape(S, S, bins)

    def table(self):
        """What SGPRModel.md_adf_table returns."""
        samples = -(-self.n // self.every)
        angles = self.angles.copy()
        for b in range(len(self.species)):
            for c in range(b):
                angles[:, b, c] = angles[:, c, b]
        return dict(angles=angles, coord=self.coord.copy(), species=np.array(self.species), n=self.nz.copy(), samples=samples,
                    next_due=samples * self.every, every=self.every, bins=self.bins, cut=self.cut.copy())


VH_MAXRBINS = 2048   # radial bins of the self part (md_vanhove.inc)
VH_MAXABINS = 64     # polar and azimuthal bins: the edge tables sit in LDS
VH_MAXBYTES = 1 << 30   # the self table levels S rbins tbins pbins 8 B


def vanhove_edges(tbins, pbins):
    """The angular edges of the van Hove self part as the comparisons take them: ct [tbins] = cos(k pi / tbins), cu, su [pbins] =
    cos, sin of f_k = -pi + 2 pi k / pbins (entry 0 of each is never compared).  Made here once, with numpy; SGPRModel.md_vanhove
    uploads these doubles and VanHoveCounts compares with the same ones."""
    kt, kp = np.arange(int(tbins), dtype=float), np.arange(int(pbins), dtype=float)
    f = -np.pi + 2.0 * np.pi * kp / float(pbins)
    return np.cos(kt * np.pi / float(tbins)), np.cos(f), np.sin(f)


def vanhove_self_bins(d, rmax, rbins, tbins, pbins, ct, cu, su):
    """The bin rule of the self part for displacements d [n, 3]: (inside [n] bool, kr, kt, kp [n]) — r = sqrt((d0 d0 + d1 d1) +
    d2 d2) as the reference's cart_coord_to_sph forms it; r >= rmax is outside; kr = min((int)((r / rmax) rbins), rbins - 1); kt
    counts the polar edges k = 1 ... tbins - 1 with d2 <= ct[k] r (theta >= k pi / tbins); kp counts the azimuthal edges
    k = 1 ... pbins - 1 that atan2(d1, d0) has passed, decided by the sign of d1 and of cu[k] d1 - su[k] d0; r == 0 is bin
    (0, 0, pbins / 2), where the reference's atan2(0, 0) = 0 lands.  Only + - x / sqrt and comparisons: no acos, no atan2."""
    d = np.asarray(d, float).reshape(-1, 3)
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    q = d0 * d0 + d1 * d1
    r = np.sqrt(q + d2 * d2)
    inside = r < rmax
    kr = np.minimum(((r / rmax) * float(rbins)).astype(np.int64), rbins - 1)
    kt = np.zeros(len(d), dtype=np.int64)
    for k in range(1, tbins):
        kt += d2 <= ct[k] * r
    kp = np.zeros(len(d), dtype=np.int64)
    for k in range(1, pbins):
        cross = cu[k] * d1 - su[k] * d0 >= 0.0
        if 2 * k < pbins:
            kp += (d1 >= 0.0) | cross
        elif 2 * k == pbins:
            kp += d1 >= 0.0
        else:
            kp += (d1 >= 0.0) & cross
    held = r == 0.0
    kr[held], kt[held], kp[held] = 0, 0, pbins // 2
    return inside, kr, kt, kp


class VanHoveCounts:
    """Van Hove correlation functions as tables of integers — the host twin of the accumulator inside the device loop
    (SGPRModel.md_vanhove, md_vanhove.inc) and its definition; every entry is a count, so the two are equal.  The self part is
    what theforce/analysis/analysis.py:178-210 (`hist_rtp_displacements`: np.histogramdd of the displacements over (r, theta,
    phi) at one lag) takes from a stored trajectory; the reference has no distinct part.
      add(x) is fed the configurations 0, 1, 2, ... of a run ([N, 3], caller atom order, never wrapped).  Samples and levels are
    MsdBlocks': configuration n with n % every == 0 is sample s = n / every; level l < levels has the lag 2^l samples and ONE
    origin O_l; at sample s every level with s mod 2^l == 0 is due, measures if s >= 2^l (count[l] += 1) and then sets O_l <- x.
      Self: per atom i of species slot z, d = x_i - O_l,i goes through vanhove_self_bins; self[l, z, kr, kt, kp] or over[l, z]
    gains 1, so self[l, z].sum() + over[l, z] == n_z count[l].  Displacements are raw: no centre of mass is taken out.
      Distinct (dbins > 0): distinct[l, a, b, k] gains the number of triples (i of a, j of b, s in Z^3) with (j, s) != (i, 0) and
        d = (x_j - O_l,i) + ((s0 h0 + s1 h1) + s2 h2),  r = sqrt((d0 d0 + d1 d1) + d2 d2) < dmax,  k = (int)((r / dmax) dbins)
    — RdfCounts' enumeration with rmin = 0: the pair goes to its nearest image by n = rint(dx inv), s = t - n over the block
    |t_k| <= R_k, and for j == i the image left out is s == 0, that is t == n (an atom that has moved more than half a cell has
    n != 0).  Origin and present are not interchangeable: the full S x S is kept.  A frozen trajectory gives RdfCounts' table
    per window."""

    def __init__(self, every, levels, rmax, rbins, tbins, pbins, dmax, dbins, numbers, species, cell, pbc):
        if every < 1 or not 1 <= levels <= 32:
            raise ValueError("VanHoveCounts: every >= 1, 1 <= levels <= 32")
        if not (1 <= rbins <= VH_MAXRBINS and 1 <= tbins <= VH_MAXABINS and 1 <= pbins <= VH_MAXABINS and 0.0 < rmax < 1e300):
            raise ValueError(f"VanHoveCounts: rmax > 0, 1 <= rbins <= {VH_MAXRBINS}, 1 <= tbins, pbins <= {VH_MAXABINS}")
        if not 0 <= dbins <= RDF_MAXBINS or (dbins and not 0.0 < float(dmax) < 1e300):
            raise ValueError(f"VanHoveCounts: 0 <= dbins <= {RDF_MAXBINS}, dmax > 0 with dbins > 0")
        self.every, self.levels, self.rmax = int(every), int(levels), float(rmax)
        self.rbins, self.tbins, self.pbins = int(rbins), int(tbins), int(pbins)
        self.dbins, self.dmax = int(dbins), float(dmax) if dbins else 0.0
        self.species = [int(z) for z in species]
        S = len(self.species)
        if self.levels * S * self.rbins * self.tbins * self.pbins * 8 > VH_MAXBYTES:
            raise NotImplementedError(f"VanHoveCounts: a self table of {self.levels} x {S} x {self.rbins} x {self.tbins} x {self.pbins} counts; at most 1 GiB")
        self.ct, self.cu, self.su = vanhove_edges(self.tbins, self.pbins)
        self.h = np.asarray(cell, float).reshape(3, 3).copy()
        self.pbc = np.broadcast_to(np.asarray(pbc, bool), (3,)).copy()
        self.volume = 0.0
        if self.dbins:
            self.inv, self.volume, self.heights, self.R = rdf_geometry(self.h, self.pbc, self.dmax)
            for k in range(3):
                if self.R[k] > RDF_MAXR:
                    raise NotImplementedError(f"VanHoveCounts: dmax = {self.dmax:g} against the cell height {self.heights[k]:g} along direction {k} "
                                              f"needs images {self.R[k]} cells away; at most {RDF_MAXR} (125 shifts)")
        else:
            try:
                self.volume = rdf_geometry(self.h, self.pbc, 0.0)[1]
            except ValueError:   # (a cell without volume: the self part needs none, the density is then 0)
                pass
        numbers = np.asarray(numbers)
        self.idx = [np.flatnonzero(numbers == z) for z in self.species]
        self.nz = np.array([len(i) for i in self.idx])
        self.origin = [None] * self.levels
        self.count = np.zeros(self.levels, dtype=np.int64)
        self.hs = np.zeros((self.levels, S, self.rbins, self.tbins, self.pbins), dtype=np.uint64)
        self.over = np.zeros((self.levels, S), dtype=np.uint64)
        self.hd = np.zeros((self.levels, S, S, self.dbins), dtype=np.uint64)
        self.n = 0   # configurations seen

    def _self(self, l, x):
        shape = (self.rbins, self.tbins, self.pbins)
        for z, I in enumerate(self.idx):
            if len(I) == 0:
                continue
            inside, kr, kt, kp = vanhove_self_bins(x[I] - self.origin[l][I], self.rmax, self.rbins, self.tbins, self.pbins, self.ct, self.cu, self.su)
            flat = np.ravel_multi_index((kr[inside], kt[inside], kp[inside]), shape)
            self.hs[l, z] += np.bincount(flat, minlength=self.rbins * self.tbins * self.pbins).reshape(shape).astype(np.uint64)
            self.over[l, z] += np.uint64(np.sum(~inside))

    def _pairs(self, xi, xj, same):
        """The counts [dbins] of the origins xi against the present positions xj (same: one list of atoms, (i, 0) stays out)."""
        h, inv, out = self.h, self.inv, np.zeros(self.dbins, dtype=np.int64)
        rmin, width, fbins = 0.0, self.dmax - 0.0, float(self.dbins)
        for o in range(0, len(xi), 256):
            dx = xj[None, :, :] - xi[o:o + 256, None, :]
            dx0, dx1, dx2 = dx[..., 0], dx[..., 1], dx[..., 2]
            n = [np.rint((dx0 * inv[0, k] + dx1 * inv[1, k]) + dx2 * inv[2, k]) if self.pbc[k] else np.zeros_like(dx0) for k in range(3)]
            rows = np.arange(dx.shape[0])
            for t0 in range(-self.R[0], self.R[0] + 1):
                for t1 in range(-self.R[1], self.R[1] + 1):
                    for t2 in range(-self.R[2], self.R[2] + 1):
                        s0, s1, s2 = float(t0) - n[0], float(t1) - n[1], float(t2) - n[2]
                        d0 = dx0 + ((s0 * h[0, 0] + s1 * h[1, 0]) + s2 * h[2, 0])
                        d1 = dx1 + ((s0 * h[0, 1] + s1 * h[1, 1]) + s2 * h[2, 1])
                        d2 = dx2 + ((s0 * h[0, 2] + s1 * h[1, 2]) + s2 * h[2, 2])
                        r = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
                        ok = (r >= rmin) & (r < self.dmax)
                        if same:   # (the image of i itself with s == 0: t == n)
                            own = (s0[rows, o + rows] == 0.0) & (s1[rows, o + rows] == 0.0) & (s2[rows, o + rows] == 0.0)
                            ok[rows[own], o + rows[own]] = False
                        k = np.minimum((((r[ok] - rmin) / width) * fbins).astype(np.int64), self.dbins - 1)
                        out += np.bincount(k, minlength=self.dbins)
        return out

    def _distinct(self, l, x):
        for a, Ia in enumerate(self.idx):
            for b, Ib in enumerate(self.idx):
                if len(Ia) and len(Ib):
                    self.hd[l, a, b] += self._pairs(self.origin[l][Ia], x[Ib], a == b).astype(np.uint64)

    def add(self, positions):
        """The next configuration of the run."""
        n = self.n
        self.n += 1
        if n % self.every:
            return
        s = n // self.every
        x = np.array(positions, float).reshape(-1, 3)
        for l in range(self.levels):
            if s % (1 << l):
                break
            if s >= (1 << l):
                self._self(l, x)
                if self.dbins:
                    self._distinct(l, x)
                self.count[l] += 1
            self.origin[l] = x.copy()

    def table(self):
        """What SGPRModel.md_vanhove_table returns."""
        samples = -(-self.n // self.every)
        tab = dict(over=self.over.copy(), distinct=self.hd.copy(), count=self.count.copy(),
                   lags=self.every * 2 ** np.arange(self.levels, dtype=np.int64), species=np.array(self.species), n=self.nz.copy(),
                   samples=samples, next_due=samples * self.every, every=self.every, levels=self.levels, rmax=self.rmax, rbins=self.rbins,
                   tbins=self.tbins, pbins=self.pbins, dmax=self.dmax, dbins=self.dbins, volume=self.volume)
        tab["self"] = self.hs.copy()
        return tab


def philox4x32_10(counter, key):
    """Philox4x32 with ten rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, section
    3.3 and the constants of its table): counter[..., 4] and key[..., 2] 32-bit words -> uint32[..., 4].  One round takes
    (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) with the 32 x 32 -> 64 bit
    products of M0 = D2511F53 and M1 = CD9E8D57; between two rounds the key moves on by the Weyl constants (9E3779B9: the
    golden ratio, BB67AE85: sqrt(3) - 1).  The statement of the stream the device loop draws from (md_deviate, api.hip), in
    numpy alone: nothing of the library is called."""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    c = np.asarray(counter, dtype=np.uint64) & m32
    k = np.asarray(key, dtype=np.uint64) & m32
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2   # (32 x 32 bits: no overflow of the 64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms_of_words(words):
    """(u1, u2) of four 32-bit words [..., 4], the conversion of md_deviate: the 53 leading bits of the 64-bit numbers
    c0 2^32 + c1 and c2 2^32 + c3,  u1 = ((c0 2^32 + c1 >> 11) + 1) 2^-53 in (0, 1]  and  u2 = (c2 2^32 + c3 >> 11) 2^-53
    in [0, 1): every value is a double, exactly."""
    w = np.asarray(words, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    a = (w[..., 0] << np.uint64(32)) | w[..., 1]
    b = (w[..., 2] << np.uint64(32)) | w[..., 3]
    scale = 2.0 ** -53
    return ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * scale, (b >> np.uint64(11)).astype(np.float64) * scale


def box_muller(u1, u2):
    """sqrt(-2 ln u1) cos(6.283185307179586 u2): the cosine branch of Box-Muller with the angle factor md_deviate uses, that
    double literal (the double nearest 2 pi), operation by operation in float64."""
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * np.asarray(u2, dtype=np.float64))


def md_deviate_uniforms(seed, t, atom, comp):
    """The two uniforms behind deviate (t, atom, comp) of the stream `seed` (sgpr_md_seed): Philox4x32-10 on the counter
    (t low word, t high word, atom, comp) with the key (seed low word, seed high word) — t a 64-bit two's-complement
    word (a negative t is its bit pattern), seed an unsigned one, atom and comp 32-bit words — then uniforms_of_words.
    The arguments broadcast against each other."""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    sd = np.asarray(seed, dtype=np.uint64)
    tt = np.asarray(t, dtype=np.int64).astype(np.uint64)
    at = np.asarray(atom, dtype=np.int64).astype(np.uint64) & m32
    cp = np.asarray(comp, dtype=np.int64).astype(np.uint64) & m32
    sd, tt, at, cp = np.broadcast_arrays(sd, tt, at, cp)
    counter = np.stack([tt & m32, tt >> s32, at, cp], axis=-1)
    key = np.stack([sd & m32, sd >> s32], axis=-1)
    return uniforms_of_words(philox4x32_10(counter, key))


def md_deviate(seed, t, atom, comp):
    """The standard normal deviate (t, atom, comp) of the stream `seed` as the device loop draws it (md_deviate in api.hip;
    SGPRModel.md_deviates returns out[r, a, c] = md_deviate(seed, t_first + r, a, c), a in caller order): the host twin of
    the stream, float64.  Equal to the device's up to the roundings of log, sqrt and cos — the integer part is exact."""
    return box_muller(*md_deviate_uniforms(seed, t, atom, comp))


def langevin_nvt_device(model, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, friction=1e-3, seed=1, vel=None,
                        ediff=0.0, chunk=256, on_halt=None, device_rng=False, fixed=None):
    """langevin_nvt with the state in device memory (SGPRModel.md_begin / md_run): same scheme, same random stream
    (one rng.normal(size=(N, 3)) per step, drawn here and uploaded a chunk at a time), so positions and velocities equal
    the host loop's bit for bit.  Yields (step, energy, temperature, largest covloss) per evaluation.  With ediff > 0 an
    evaluation whose largest covloss reaches it stops the run ON THE DEVICE; on_halt(model, state) — the model update of
    calculator/active.py:477-484 — is called with that configuration and its results, and the evaluation is repeated
    with whatever model on_halt left behind (an on_halt that leaves the covloss above ediff must raise ediff itself:
    it receives and may return the threshold).  fixed: held components (fixed_mask; SGPRModel.md_begin(fixed=)), the rules of
    langevin_nvt(fixed=); the temperature is over the remaining degrees of freedom."""
    from .ase_shim import kB
    rng = np.random.default_rng(seed)
    N = len(numbers)
    fx = fixed_mask(fixed, N)
    dof = 3 * N if fx is None else 3 * N - int(fx.sum())
    mass = np.array([MASS[int(z)] for z in numbers])
    kT = kB * temperature
    if vel is None:
        vel = rng.normal(size=(N, 3)) * np.sqrt(kT / mass[:, None])
        vel -= (mass[:, None] * vel).sum(0) / mass.sum()
    # device_rng: the deviates are drawn on the device (counter-based on `seed`; SGPRModel.md_deviates returns them for a
    # host twin) instead of from numpy here: nothing is generated or uploaded on the step's path
    model.md_begin(numbers, pos, cell, pbc, mass, vel, dt=dt_fs * FS, friction=friction, kT=kT,
                   seed=(int(seed) or 1) if device_rng else 0, **({} if fx is None else dict(fixed=fx)))
    done = 0                      # evaluations accepted so far (evaluation k = the configuration after k steps)
    rows = np.empty((0, N, 3))    # deviates drawn and not yet consumed: rows[0] moves the current configuration on
    skip_gate = False
    while done <= steps:
        n = 1 if skip_gate else min(chunk, steps + 1 - done)
        final = done + n == steps + 1
        need = 0 if device_rng else (n - 1 if final else n)
        if len(rows) < need:  # (numpy fills an (r, N, 3) request like r requests of (N, 3): the host loop's stream)
            rows = np.concatenate([rows, rng.normal(size=(need - len(rows), N, 3))])
        noise = None if device_rng else (rows[:n] if len(rows) >= n else np.concatenate([rows, np.zeros((n - len(rows), N, 3))]))
        sc, code = model.md_run(n, noise, ediff=0.0 if skip_gate else ediff, final=final)
        accepted = len(sc) - 1 if code == 1 else len(sc)
        if accepted:
            skip_gate = False   # (code 2 with nothing accepted: a capacity was outgrown, the same call again re-sizes it)
        for r in sc[:accepted]:
            yield done, float(r[0]), float(r[12] / (dof * kB)), float(r[11])
            done += 1
        rows = rows[accepted:]
        if code == 1:
            if on_halt is None:
                raise RuntimeError("the covloss gate fired and no on_halt handler is installed")
            on_halt(model, model.md_state(results=True))
            skip_gate = True   # the repeated evaluation stands whatever its covloss (active.py:477-484 updates once per step)
    # (the state stays readable: SGPRModel.md_state; md_begin starts the next run)


def fit_to_teacher(model, numbers, pos, cell, pbc, noise=0.05, device=0):
    """Weights of `model` fitted to the PairTeacher's energy and forces on one frame (its inducing set as it is): a
    model whose forces hold the atoms together, for MD loops that have to run for hundreds of steps."""
    teacher = PairTeacher(sorted(set(int(z) for z in numbers)), device=device)
    at = type("A", (), dict(numbers=np.asarray(numbers), positions=np.asarray(pos, float), cell=np.asarray(cell, float), pbc=pbc))()
    teacher.calculate(at)
    mu = model.fit([dict(numbers=numbers, positions=pos, cell=cell, pbc=pbc, energy=teacher.results["energy"],
                         forces=teacher.results["forces"])], noise=noise)
    teacher.close()
    return mu


def inducing_from_frame(model, numbers, pos, cell, pbc, m, seed, noise=0.05):
    """m LCEs drawn species-proportionally from a frame (+ noise), using the MODEL's own device
    neighbour list (the product path; no oracle involved)."""
    rng = np.random.default_rng(seed)
    N = len(numbers)
    model.predict(numbers, pos, cell, pbc, beta=False)  # builds the neighbour list on the device
    ptr, j, off = model.neighbors(N)
    numbers = np.asarray(numbers)
    picks = []
    zs, cnt = np.unique(numbers, return_counts=True)
    quota = np.floor(cnt / N * m).astype(int)
    quota[np.argmax(cnt)] += m - quota.sum()
    for z, q in zip(zs, quota):
        picks.extend(rng.choice(np.nonzero(numbers == z)[0], size=q, replace=False).tolist())
    X = []
    rc = model.cutoff
    for a in picks:
        s = slice(int(ptr[a]), int(ptr[a + 1]))
        r = pos[j[s]] - pos[a] + off[s].astype(float) @ cell
        r = r + noise * rng.normal(size=r.shape)
        keep = np.linalg.norm(r, axis=1) < rc - 1e-3
        X.append(Local(int(numbers[a]), numbers[j[s]][keep], r[keep]))
    return X


def config5_preseeded(shape=(32, 32, 16), m_seed=1000, max_inducing=1024, n_exceed=8, seed=0, device=0, temperature=600.0,
                      friction=0.1, n_equil=250, **calc_kw):
    """BASELINE config 5 with the model ALREADY near its size limit, in a STATIONARY state: the ordered 4-species oxide
    (16384 atoms for the default shape) is first equilibrated at `temperature` by `n_equil` steps of Langevin MD under
    the teacher alone; an SGPR model is pre-seeded with `m_seed` inducing LCEs drawn species-proportionally from two
    frames of that trajectory and fitted to a third; a fourth, held out, sets the sampling threshold: ediff = the
    `n_exceed`-th largest covloss of that frame — so that on-the-fly MD continued from there offers a handful of
    environments per step (not none, not all: the default 2 kcal/mol is calibrated for DFT energies), reaches
    `max_inducing` within a few update steps, and from then on every update ends in downsize(lii=True)
    (calculator/active.py:963-969 -> regression/gppotential.py:829-832).
    Returns (calc, teacher, (numbers, positions, cell, pbc), velocities)."""
    from .calculator import ActiveCalculator
    from .model import SGPRModel
    from .posterior import Frame, PosteriorPotential
    numbers, pos, cell, pbc = oxide_ordered(shape, seed=seed, sigma=0.05)
    species = sorted(set(int(z) for z in numbers))
    teacher = PairTeacher(species, device=device)
    marks = sorted({max(1, int(n_equil * f)) for f in (0.6, 0.75, 0.9)} | {n_equil})
    snaps = {}
    vel = None
    for step, E, T, wall, p, v in langevin_nvt(teacher, numbers, pos, cell, pbc, n_equil, temperature, 1.0, friction, seed=seed + 5):
        if step in marks:
            snaps[step] = (p.copy(), teacher.results["energy"], teacher.results["forces"].copy(), teacher.results["stress"].copy())
        pos, vel = p, v
    model = SGPRModel(3, 3, 4, 6.0, species=species, device=device)
    X = []
    for k, st in enumerate(marks[:2]):
        X += inducing_from_frame(model, numbers, snaps[st][0], cell, pbc, m_seed // 2 + (k == 0) * (m_seed % 2), seed=seed + 21 + k, noise=0.0)
    p3, e3, f3, s3 = snaps[marks[2]]
    post = PosteriorPotential(model)
    post.set_data([Frame(numbers, p3, cell, pbc, e3, f3, s3)], X)
    post.make_munu(algo=3, noise_f=calc_kw.get("noise_f", 0.043))
    beta = np.sort(np.asarray(model.predict(numbers, snaps[marks[3]][0], cell, pbc)["beta"]))
    ediff = float(beta[-max(1, int(n_exceed))])
    kw = dict(logfile=None, tape=None, pckl=None, ediff=ediff, fdiff=3 * ediff, ediff_tot=2 * ediff, max_inducing=max_inducing)
    kw.update(calc_kw)
    calc = ActiveCalculator(covariance=post, calculator=teacher, **kw)
    return calc, teacher, (numbers, pos, cell, pbc), vel
