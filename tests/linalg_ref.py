"""Host references for the solve-side kernels (Cholesky, triangular inverse, least squares), independent of the device.

The regression's least squares (regression/gppotential.py:1204-1339) is
    mu = argmin || [K; sigma L^T] mu - [Y; 0] ||,   L L^T = K_mm + ridge I,
so every check here is written against A = [K; sigma L^T], b = [Y; 0].  Its normal equations only need L L^T, so the
backward-error check takes K_mm + ridge I itself and never forms a factor: the residual is the same for every L.

Also restated here: the dispatch arithmetic of the flat-panel band QR (csrc/bandqr.inc: launch_band_qr), so that the GPU
tests can aim at each of its branches by shape.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# csrc/bandqr.inc / csrc/tsqr.hip constants the shapes are aimed at
BQ_MAXR = 64 * 17          # rows of the largest panel the flat-panel band form holds
BQ_SLOTS = (2, 4, 6, 9, 13, 17)   # band_qr_step_kernel<NS> instantiations
QR_MAX_COLS = 8192
TNB = 32                   # panel width of both QR forms
QR_APPEND_MAX = 32         # csrc/data.inc: one-column panels a kept first-stage factor takes before it is refactored
ER_MAX = 16                # csrc/data.inc: frames the one-workgroup energy-row kernel takes


# ---------------------------------------------------------------------------------------------- band QR dispatch
def band_panel_rows(m, rows=None, band=2, band_off=0):
    """Active rows (row_end - k0) of every 32-column panel of a banded rows x m problem, as launch_band_qr computes them.
    The regression's second stage is rows = 2m, band = 2."""
    rows = 2 * m if rows is None else rows
    out = []
    for k0 in range(0, m, TNB):
        nb = min(TNB, m - k0)
        out.append(min(rows, band * (k0 + nb) + band_off) - k0)
    return out


def band_form_takes(m):
    """True when the 2m x m second stage runs on the flat-panel kernel (every panel within BQ_MAXR rows)."""
    return max(band_panel_rows(m)) <= BQ_MAXR


def band_slot_bucket(m):
    """The band_qr_step_kernel<NS> instantiation the largest panel of the 2m x m second stage launches."""
    ns = -(-max(band_panel_rows(m)) // 64)
    return next(b for b in BQ_SLOTS if ns <= b)


def band_bucket_edges():
    """For every slot bucket, the largest m whose second stage still fits it, and the next m (which does not)."""
    out = {}
    m = 1
    while band_form_takes(m):
        b = band_slot_bucket(m)
        if band_form_takes(m + 1) and band_slot_bucket(m + 1) == b:
            m += 1
            continue
        out[b] = m
        m += 1
    return out


# ---------------------------------------------------------------------------------------------- resident data path
def data_keeps_factor(m, rows):
    """True when the resident solve takes the kept first-stage factor (data.inc: qr_keep_update), the only route that
    appends the energy rows to a force-only factor; the other one factors the whole matrix from scratch."""
    return rows >= m + QR_APPEND_MAX + 64 and m + QR_APPEND_MAX + 8 <= 2048


def energy_rows_form(m, frames):
    """The form data.inc: energy_rows_append takes on the kept route: (SLOTS, NE) of energy_rows_update_kernel, or
    "blocked" (the banded factorisation).  Its m + 1 > 2048 condition cannot hold there (the kept route needs m <= 2008)."""
    if frames > ER_MAX or m + 1 > 2048:
        return "blocked"
    return (1 if m + 1 <= 1024 else 2, 2 if frames <= 2 else 4 if frames <= 4 else 16)


# ---------------------------------------------------------------------------------------------- Cholesky
def integer_spd(n, seed=0):
    """(A, L0): A = L0 L0^T with L0 lower triangular, integer, diagonal in [8, 16], off-diagonal entries in [-3, 3] on
    about eight places per row.  Every entry of A is an integer below 2^53, so A is exact in fp64, and L0 is the exact
    Cholesky factor; cond(A) stays below ~20 at every n (dense rows of this size would grow it exponentially)."""
    rng = np.random.default_rng(seed)
    p = min(0.5, 8.0 / max(n, 1))
    L0 = np.tril(rng.integers(-3, 4, size=(n, n)) * (rng.random((n, n)) < p), -1).astype(np.int64)
    L0[np.diag_indices(n)] = rng.integers(8, 17, size=n)
    A = L0 @ L0.T   # int64: exact
    assert np.abs(A).max() < 2 ** 53
    return A.astype(np.float64), L0.astype(np.float64)


def cholesky_ld(A):
    """Lower Cholesky factor of a symmetric positive definite matrix in long double (right-looking, column by column)."""
    A = np.array(A, dtype=LD)
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"cholesky_ld: pivot {j} is {d}")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tril_inverse_ld(L):
    """L^-1 of a lower triangular matrix by forward substitution in long double (row by row: X L = I)."""
    L = np.asarray(L, dtype=LD)
    n = len(L)
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        # row i of L X = I: L[i, :i] X[:i] + L[i, i] X[i] = e_i
        r = -(L[i, :i] @ X[:i]) if i else np.zeros(n, dtype=LD)
        r[i] += 1
        X[i] = r / L[i, i]
    return X


# ---------------------------------------------------------------------------------------------- least squares
def _chunks(n, size=2048):
    for a in range(0, n, size):
        yield slice(a, min(n, a + size))


def lstsq_eta(K, Y, mu, sigma=0.0, G=None):
    """Normwise backward error of mu for min ||A mu - b||, A = [K; sigma L^T], b = [Y; 0], L L^T = G, through the normal
    equations residual:
        eta = ||A^T (b - A mu)|| / (||A||_F (||A||_F ||mu|| + ||b||)),
        A^T (b - A mu) = K^T (Y - K mu) - sigma^2 G mu,   ||A||_F^2 = ||K||_F^2 + sigma^2 trace(G).
    Accumulated in long double from the fp64 inputs, in row chunks (O(rows m + m^2), no m x m copy of K)."""
    K = np.asarray(K)
    m = K.shape[1]
    mu_l = np.asarray(mu, dtype=np.float64).astype(LD)
    g = np.zeros(m, dtype=LD)
    fro2 = LD(0)
    for s in _chunks(len(K)):
        Kc = K[s].astype(LD)
        r = np.asarray(Y[s], dtype=np.float64).astype(LD) - Kc @ mu_l
        g += Kc.T @ r
        fro2 += np.sum(Kc * Kc)
    if G is not None and sigma != 0.0:
        G = np.asarray(G)
        s2 = LD(sigma) * LD(sigma)
        for s in _chunks(m):
            Gc = G[s].astype(LD)
            g[s] -= s2 * (Gc @ mu_l)
            fro2 += s2 * np.trace(Gc[:, s])
    afro = np.sqrt(fro2)
    bnorm = np.sqrt(np.sum(np.asarray(Y, dtype=np.float64).astype(LD) ** 2))
    den = afro * (afro * np.sqrt(np.sum(mu_l * mu_l)) + bnorm)
    return float(np.sqrt(np.sum(g * g)) / den)


def stacked_system(K, Y, G, sigma):
    """The explicit A = [K; sigma L^T], b = [Y; 0] with L = chol(G) (any factor: the solution does not depend on it)."""
    L = np.linalg.cholesky(G)
    A = np.vstack([K, sigma * L.T])
    b = np.concatenate([Y, np.zeros(len(G))])
    return A, b


def lstsq_forward(A, b):
    """(x, tol, kappa) for the fp64 least-squares solution of A x = b: LAPACK's Householder QR (an independent
    implementation), and the first-order bound of the forward error of a backward-stable solver relative to ||x||,
        eps (kappa + kappa^2 ||r|| / (||A|| ||x||)),   kappa = cond_2(A) = cond_2(R),
    times 8 sqrt(m) for the constants of two Householder factorisations in a row (stage 1, stage 2) against this one."""
    from scipy.linalg import solve_triangular
    Q, R = np.linalg.qr(A)
    x = solve_triangular(R, Q.T @ b)
    s = np.linalg.svd(R, compute_uv=False)
    kappa = s[0] / s[-1]
    r = b - A @ x
    tol = 8 * np.sqrt(A.shape[1]) * EPS * (kappa + kappa ** 2 * np.linalg.norm(r) / (s[0] * np.linalg.norm(x)))
    return x, tol, kappa
