"""Host references for the three GEMMs of a step (K_nm, the energy, the covloss), independent of the device's tile tables.

The inputs are the device's own descriptors (sgpr_get_descriptors / sgpr_get_inducing_descriptors), so descriptor error
stays out of these checks and the bounds can be tight.  Everything is computed in np.longdouble (large blocks: float64, see _prod), only inside species blocks
(K is block-diagonal: k(x, x') = 0 for two central species), with an a-priori bound of the device's rounding error:

  K_iq   = [Z_i == Z_q] (p_i . p_q)^eta, the lone-atom rule of similarity.py:94-103 (csrc/gemm_tile.inc, the EPI_KERNEL
           epilogue): lone_weight for two lone atoms of one species, 0 for one lone atom against a non-lone one.
           |dK| <= eta |v|^(eta-1) gamma_D sum|p q| + gamma_eta |K|
  E      = sum_iq K_iq mu_q + sum_i mean_w[Z_i]          |dE| <= sum |mu| |dK| + gamma_nm sum |K mu| + gamma_n sum |mean_w|
  c_i    = sum_a (sum_q choli[a, q] K_iq)^2, over ALL rows a of choli
           |dc| <= sum_a (2 |y_a| + dy_a) dy_a + gamma_m c,  dy_a = sum_q |choli_aq| (gamma_m |K_iq| + |dK_iq|)

The device reports beta = sqrt(1 - c) sqrt(vscale); with vscale = 1, c_dev = 1 - beta^2 carries about 4 eps of its own.

Also restated here: the tile-count arithmetic of csrc/api.hip (count_tiles, decide_tile_heights, the half-tile rule and the
chaining window of build_tiles), so that the GPU tests can place frames on both sides of every automatic switch.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble
KT = 32          # k-slice of every step GEMM (build_tiles: kb / ke rounded out to it)
TN = 64          # columns per tile


LD_WORK = 2e7   # multiply-adds of one species block beyond which the product runs in float64 (BLAS), its own rounding
                # (the same gamma_n sum|a b| as the device's) added to the bound


def _prod(A, B):
    """(A @ B, bound of the host's rounding): long double for small blocks, float64 for large ones."""
    if A.shape[0] * A.shape[1] * B.shape[1] <= LD_WORK:
        return A.astype(LD) @ B.astype(LD), 0.0
    A64, B64 = A.astype(float), B.astype(float)
    return (A64 @ B64).astype(LD), gamma(A.shape[1] + 2) * (np.abs(A64) @ np.abs(B64))


def gamma(n):
    n = float(n) * EPS
    return n / (1.0 - n)


def _dpow(av, dv, eta):
    """Bound of |x^eta - v^eta| for |x - v| <= dv, x and v >= 0, av = |v|.  eta >= 1: the derivative eta x^(eta-1) grows with
    x, so its value at av + dv times dv.  eta < 1: the derivative falls with x, so its value at av - dv where that is
    positive, and never more than dv^eta (|x^eta - v^eta| <= |x - v|^eta for a concave power).  dv = 0 (a pair of
    descriptors with disjoint blocks: every product of the dot is an exact zero) gives 0 at every exponent."""
    if eta >= 1.0:
        return eta * (av + dv) ** (eta - 1.0) * dv
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(av > dv, eta * np.maximum(av - dv, 1e-300) ** (eta - 1.0) * dv, np.inf)
    return np.minimum(lo, dv ** eta)


# ---------------------------------------------------------------------------------------------- references
def knm(P, Q, zi, zq, lone_i, lone_q, eta, lone_weight=1.0):
    """P [n, ...] and Q [m, ...] descriptors (flattened to rows), zi [n] / zq [m] species slots (-1: a ghost, no kernel),
    lone_* True where the atom has no neighbour.  Returns (K [n, m] longdouble, bound [n, m])."""
    P = np.asarray(P, float).reshape(len(zi), -1)
    Q = np.asarray(Q, float).reshape(len(zq), -1)
    zi, zq = np.asarray(zi), np.asarray(zq)
    lone_i, lone_q = np.asarray(lone_i, bool), np.asarray(lone_q, bool)
    n, m = len(zi), len(zq)
    K = np.zeros((n, m), LD)
    B = np.zeros((n, m))
    g = gamma(P.shape[1] + 2)
    for s in np.unique(zq):
        rows, cols = np.flatnonzero(zi == s), np.flatnonzero(zq == s)
        if s < 0 or len(rows) == 0 or len(cols) == 0:
            continue
        v, host = _prod(P[rows], Q[cols].T)
        a = np.abs(P[rows]) @ np.abs(Q[cols]).T
        dv = g * a + host
        k = v ** LD(eta)
        bk = _dpow(np.abs(v).astype(float), dv, eta) + gamma(int(np.ceil(eta)) + 2) * np.abs(k).astype(float)
        li, lq = lone_i[rows][:, None], lone_q[cols][None, :]
        k = np.where(li & lq, LD(lone_weight), np.where(li | lq, LD(0), k))
        bk = np.where(li | lq, 0.0, bk)
        K[np.ix_(rows, cols)] = k
        B[np.ix_(rows, cols)] = bk
    return K, B


def energy(K, bK, mu, zi, mean_w):
    """(E, bound) of sum K mu + sum mean_w[Z_i] (ghosts, zi < 0, carry no mean)."""
    mu = np.asarray(mu, float)
    zi = np.asarray(zi)
    mean = np.array([mean_w[s] if s >= 0 else 0.0 for s in zi], float)
    t = K * mu.astype(LD)[None, :]
    E = t.sum() + mean.astype(LD).sum()
    n, m = K.shape
    b = (bK * np.abs(mu)[None, :]).sum() + gamma(n * m + n + 2) * (float(np.abs(t).sum()) + np.abs(mean).sum())
    return E, b


def covloss(K, bK, choli, zi, zq):
    """(c [n] longdouble, bound [n]) of c_i = sum_a (sum_q choli[a, q] K_iq)^2 over every row a of choli."""
    choli = np.asarray(choli, float)
    zi, zq = np.asarray(zi), np.asarray(zq)
    n, m = K.shape
    c = np.zeros(n, LD)
    b = np.zeros(n)
    g = gamma(m + 4)
    for s in np.unique(zq):
        rows, cols = np.flatnonzero(zi == s), np.flatnonzero(zq == s)
        if s < 0 or len(rows) == 0 or len(cols) == 0:
            continue
        Cs = choli[:, cols]                                   # every row a (rows that are zero here add nothing), this species' columns
        Cs = Cs[np.any(Cs != 0, axis=1)]
        Ks = K[np.ix_(rows, cols)]
        y, host = _prod(Ks, Cs.T)                             # [rows, a]
        dy = g * (np.abs(Ks).astype(float) @ np.abs(Cs).T) + bK[np.ix_(rows, cols)] @ np.abs(Cs).T + host
        cs = (y * y).sum(axis=1)
        c[rows] = cs
        b[rows] = ((2 * np.abs(y).astype(float) + dy) * dy).sum(axis=1) + g * cs.astype(float)
    return c, b


def c_from_beta(beta, vscale=1.0):
    """The device's covloss c back from beta = sqrt(1 - c) sqrt(vscale) (exact to about 4 eps where c < 1)."""
    return 1.0 - (np.asarray(beta, float) / np.sqrt(vscale)) ** 2


C_READ = 4 * EPS   # what c_from_beta adds to the device's own rounding


# ---------------------------------------------------------------------------------------------- checks
def check_knm(Kdev, K, bK, zi, zq, rows=None, what=""):
    """Cross-species (and ghost) entries exactly zero; the rest within the bound."""
    Kdev = np.asarray(Kdev, float)
    zi, zq = np.asarray(zi), np.asarray(zq)
    rows = np.arange(len(zi)) if rows is None else np.asarray(rows)
    same = (zi[rows][:, None] == zq[None, :]) & (zi[rows][:, None] >= 0)
    off = Kdev[rows][~same]
    assert not np.any(off != 0.0), (what, "cross-species K entries", int(np.count_nonzero(off)))
    err = np.abs(Kdev[rows].astype(LD) - K[rows]).astype(float)
    bad = err > bK[rows]
    assert not bad.any(), (what, "K_nm", int(bad.sum()), float((err / np.maximum(bK[rows], 1e-300)).max()))
    return float(err.max()) if err.size else 0.0


def check_energy(Edev, E, bE, what=""):
    err = abs(LD(Edev) - E)
    assert err <= bE, (what, "energy", float(err), bE)
    return float(err)


def check_c(cdev, c, bc, rows=None, what=""):
    cdev = np.asarray(cdev, float)
    rows = np.arange(len(c)) if rows is None else np.asarray(rows)
    err = np.abs(cdev[rows].astype(LD) - c[rows]).astype(float)
    lim = bc[rows] + C_READ
    bad = err > lim
    assert not bad.any(), (what, "covloss", int(bad.sum()), float(err.max()), float(lim[np.argmax(err - lim)]))
    return float(err.max()) if err.size else 0.0


def scale_for_c(c, cmax=0.9):
    """alpha such that the covloss of alpha * choli peaks at cmax (c scales with alpha^2)."""
    top = float(np.max(c)) if len(c) else 0.0
    return 1.0 if top <= 0 else float(np.sqrt(cmax / top))


# ---------------------------------------------------------------------------------------------- tile counts
def offsets(slots, S, rank=0, world=1):
    """(aoff [S + 1], cnt) of a rank's rows: atoms stably sorted by species slot (slot < 0: a ghost, sorted last), rank r
    taking sorted atoms r, r + world, ...  (sgpr_bind_system).  Ghost rows lie beyond aoff[S]: species_of() counts them
    with the last species."""
    s = np.asarray(slots)
    s = np.where(s < 0, S, s)
    srt = np.sort(s, kind="stable")
    mine = srt[rank::world]
    aoff = np.zeros(S + 1, int)
    for k in range(S):
        aoff[k + 1] = aoff[k] + int(np.count_nonzero(mine == k))
    return aoff, len(mine)


def qoffsets(zq, S):
    q = np.zeros(S + 1, int)
    for k in range(S):
        q[k + 1] = q[k] + int(np.count_nonzero(np.asarray(zq) == k))
    return q


def _species_of(off, S, idx):
    s = 0
    while s + 1 < S and off[s + 1] <= idx:
        s += 1
    return s


def tiles(aoff, qoff, cnt, m, Dpad, kind, bm, choli_lower=True):
    """(rt, ct, kb, ke) of every working tile of product `kind` (0 K_nm, 1 W, 2 covloss), as build_tiles lists them."""
    S = len(qoff) - 1
    ncols = Dpad if kind == 1 else m
    out = []
    for rt in range(-(-cnt // bm)):
        r0, r1 = rt * bm, min(cnt, rt * bm + bm) - 1
        sa, sb = _species_of(aoff, S, r0), _species_of(aoff, S, r1)
        qlo, qhi = qoff[sa], qoff[sb + 1]
        for ct in range(-(-ncols // TN)):
            c0, c1 = ct * TN, min(ncols, ct * TN + TN)
            if kind == 0:
                if c0 >= qhi or c1 <= qlo:
                    continue
                kb, ke = 0, Dpad
            elif kind == 1:
                kb, ke = qlo, qhi
            else:
                if c0 >= qhi or c1 <= qlo:
                    continue
                kb, ke = qlo, (min(qhi, c1) if choli_lower else qhi)
            kb, ke = kb // KT * KT, -(-ke // KT) * KT
            if ke > kb:
                out.append((rt, ct, kb, ke))
    return out


def count_tiles(aoff, qoff, cnt, m, Dpad, kind, bm):
    return len(tiles(aoff, qoff, cnt, m, Dpad, kind, bm))


def tile_heights(aoff, qoff, cnt, m, Dpad, ncu, half=True):
    """(K_nm rows, W + covloss rows) per tile that decide_tile_heights and build_tiles pick automatically."""
    n32k = count_tiles(aoff, qoff, cnt, m, Dpad, 0, 32)
    n32w = count_tiles(aoff, qoff, cnt, m, Dpad, 1, 32) + count_tiles(aoff, qoff, cnt, m, Dpad, 2, 32)
    bk = 64 if n32k >= 3 * ncu else 16 if (half and 5 * n32k <= 2 * ncu) else 32
    bw = 64 if 2 * n32w >= 11 * ncu else 16 if (half and 5 * n32w <= 3 * ncu) else 32
    return bk, bw


def xcd_shares(aoff, qoff, cnt, m, Dpad, bm, choli_lower=True):
    """Entries of the grouped W + covloss table each XCD gets (position % 8 == row tile % 8)."""
    sh = [0] * 8
    for kind in (1, 2):
        for t in tiles(aoff, qoff, cnt, m, Dpad, kind, bm, choli_lower):
            sh[t[0] % 8] += 1
    return sh


def chained(aoff, qoff, cnt, m, Dpad, ncu, bw, chain=True):
    """Tiles build_tiles chains behind another one: per XCD, those beyond four per CU while at most one more per CU."""
    if not chain or bw == 64:
        return 0
    cx = ncu // 8
    return sum(s - 4 * cx for s in xcd_shares(aoff, qoff, cnt, m, Dpad, bw) if 4 * cx < s <= 5 * cx)
