"""The solve side (regression/gppotential.py:1204-1339, regression/algebra.py:29-47) at the sizes where its kernels change
code: Cholesky panels, the per-species triangular inverse, the TSQR tree of the first stage, the flat-panel band QR of the
second stage and its hand-over to the tree form, the batched re-solve, the energy rows of the resident data path, and the
m = 8192 column limit.  Every result is checked against a host reference (tests/linalg_ref.py), never only against
another device path:

  Cholesky   exact integer factors: ridge 0, upper triangle exactly 0, L within n eps cond(A) of L0;
  choli      zero off the species blocks and above the diagonal; each block against a long-double inverse;
  weights    the normwise backward error eta of the normal equations of [K; sigma L^T] mu = [Y; 0] (<= 1e-13), and for
             m <= 2304 the forward error against LAPACK's Householder QR within eps (kappa + kappa^2 ||r|| / (||A|| ||x||)).

Environment switches are read once per process, so the non-default forms run in a child process each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linalg_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SPECIES = [3, 15, 16]
ETA_MAX = 1e-13
_POOLS = {}


def model():
    from autoforce_amd import SGPRModel
    return SGPRModel(3, 3, 4, 6.0, species=SPECIES)


def pool(n_side, seed=1):
    """All but eight atoms of a lips(n_side) frame as LCEs, drawn by workloads.inducing_from_frame (whose species quotas
    round down: eight spare atoms keep the remainder within the largest species), grouped by species in the order of
    SPECIES: the caller order of an inducing set drawn from it is the device's species-sorted order."""
    key = (n_side, seed)
    if key not in _POOLS:
        from autoforce_amd.workloads import inducing_from_frame, lips
        numbers, pos, cell, pbc = lips(n_side, seed=seed)
        mdl = model()
        X = inducing_from_frame(mdl, numbers, pos, cell, pbc, len(numbers) - 8, seed=seed)
        mdl.close()
        _POOLS[key] = {z: [x for x in X if x.number == z] for z in SPECIES}
    return _POOLS[key]


def inducing(m, n_side=None, counts=None):
    """m LCEs (species-proportional, species-sorted), or exactly `counts` = {Z: n} of them."""
    if counts is None:
        n_side = n_side or int(np.ceil((m + 1) ** (1 / 3))) + 1
        P = pool(n_side)
        N = sum(len(v) for v in P.values())
        counts = {z: len(P[z]) * m // N for z in SPECIES}
        counts[SPECIES[-1]] += m - sum(counts.values())
    else:
        P = pool(n_side or 10)
    X = []
    for z in SPECIES:
        assert counts.get(z, 0) <= len(P[z])
        X += P[z][:counts.get(z, 0)]
    return X


def dense_problem(m, rows, seed=0):
    rng = np.random.default_rng(1000 * m + rows + seed)
    return rng.normal(size=(rows, m)), rng.normal(size=rows)


def check_weights(K, Y, M, ridge, sigma, mu, forward=True, what=""):
    """eta <= 1e-13 always; the forward error against LAPACK's QR solution where the host can afford it."""
    m = len(M)
    G = M + ridge * np.eye(m)
    eta = ref.lstsq_eta(K, Y, mu, sigma, G)
    assert eta <= ETA_MAX, (what, eta)
    if forward and m <= 2304:
        A, b = ref.stacked_system(K, Y, G, sigma)
        x, tol, kappa = ref.lstsq_forward(A, b)
        err = np.linalg.norm(mu - x) / np.linalg.norm(x)
        assert err <= tol, (what, err, tol, kappa)
    return eta


def sigma_of(M, noise):
    return noise * 0.99 * np.mean(np.diag(M))   # gppotential.py:1219-1222, :1245-1247


# ---------------------------------------------------------------------------------------------- jitcholesky
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 257, 1000])
def test_jitcholesky_exact_integer_factor(n):
    """potrf_panel_kernel over 64-column panels (the last one partial, none below the last) and the EPI_SUBLOWER
    update: A = L0 L0^T is exact in fp64 and cond(A) < 50, so L must reproduce L0 to n eps cond(A) of its largest
    entry, with no ridge and an upper triangle of exact zeros."""
    A, L0 = ref.integer_spd(n, seed=n)
    mdl = model()
    L, ridge = mdl.jitcholesky(A)
    mdl.close()
    assert ridge == 0.0
    assert np.all(np.triu(L, 1) == 0.0)
    cond = np.linalg.cond(A)
    err = np.abs(L - L0).max()
    assert err <= n * ref.EPS * cond * np.abs(L0).max(), (err, cond)


@pytest.mark.parametrize("n", [64, 65, 129])
def test_jitcholesky_semidefinite_rung(n):
    """A rank-n/2 Gram matrix: the jitter ladder must stop at the oracle's rung (as test_hip_parity at n = 150), with the
    factor of the shifted matrix."""
    from oracle import oracle as orc
    rng = np.random.default_rng(n)
    V = rng.normal(size=(n, n // 2))
    G = V @ V.T
    _, r0 = orc.jitcholesky(G)
    mdl = model()
    L, r1 = mdl.jitcholesky(G)
    mdl.close()
    assert r0 > 0.0 and r1 == r0, (r1, r0)
    assert np.all(np.triu(L, 1) == 0.0)
    np.testing.assert_allclose(L @ L.T, G + r1 * np.eye(n), rtol=0, atol=1e-10 * np.abs(G).max())


# ---------------------------------------------------------------------------------------------- species blocks
BLOCKS = [(1,), (31,), (32,), (33,), (63,), (64,), (65,), (129,), (63, 64, 65)]


@pytest.mark.parametrize("sizes", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_species_blocks_of_the_inverse_factor(sizes):
    """tril_inverse_kernel (one workgroup per 64-column block) per species block of K_mm.  choli must be exactly zero
    off the blocks and above the diagonal.  Each block is compared with the long-double inverse of the long-double
    Cholesky factor of the same block; the device inverts its own fp64 factor, whose forward error is up to
    n eps cond(block) relative, and inverting moves that by cond(L) = cond(block)^(1/2) again: the tolerance is
    n eps cond(block)^(3/2) of the largest entry (cond of these blocks: 1 to ~1e4)."""
    counts = dict(zip(SPECIES, sizes)) if len(sizes) > 1 else {SPECIES[0]: sizes[0]}
    X = inducing(sum(sizes), counts=counts)
    mdl = model()
    mdl.set_inducing(X)
    m = mdl.m
    K, Y = dense_problem(m, 3 * m + 7)
    mu = mdl.solve(K, Y)
    M, ridge, sigma = mdl.M, mdl.ridge, mdl.sigma
    choli = mdl.choli
    mdl.close()
    assert sigma == pytest.approx(sigma_of(M, 0.01), rel=1e-12)
    assert np.all(np.triu(choli, 1) == 0.0)
    off = 0
    for n in [c for c in (counts.get(z, 0) for z in SPECIES) if c]:
        blk = slice(off, off + n)
        assert np.all(choli[blk, :off] == 0.0) and np.all(choli[blk, off + n:] == 0.0)
        G = M[blk, blk] + ridge * np.eye(n)
        want = ref.tril_inverse_ld(ref.cholesky_ld(G)).astype(np.float64)
        cond = np.linalg.cond(G)
        err = np.abs(choli[blk, blk] - want).max()
        assert err <= 4 * n * ref.EPS * cond ** 1.5 * np.abs(want).max(), (n, err, cond)
        off += n
    check_weights(K, Y, M, ridge, sigma, mu)


# ---------------------------------------------------------------------------------------------- dense solve shapes
BUCKETS = ref.band_bucket_edges()   # {slots: largest m of that slot count}
SHAPES = (
    [(40, 20), (40, 40), (40, 41)]                                         # rows < m (zero rows), rows = m, rows = m + 1
    + [(33, r) for r in (255, 256, 257, 2048, 2049, 16385)]                # TSQR tree depth 1 / 2 / 3 / 4
    + [(m, r) for m in (32, 33) for r in (8191, 8192)]                     # look-ahead: rows >= 8192 and m > 32
    + [(95, 300), (97, 300), (127, 400), (129, 400)]                       # m = 31, 1 (mod 32): partial last panels
    + [(m + d, m + d + 64) for b, m in sorted(BUCKETS.items()) if b < 17 for d in (0, 1)]   # band slot buckets
    + [(BUCKETS[17] - 1, BUCKETS[17] + 63)]
)


@pytest.mark.parametrize("m,rows", SHAPES, ids=lambda v: str(v))
def test_solve_shapes_against_the_reference(m, rows):
    """First stage (TSQR of [K | Y], rows padded to max(rows, m + 1)) and second stage (band QR of [R1; sigma L^T]) at
    the boundaries of their tree depth, panel count, look-ahead switch and band slot count."""
    X = inducing(m)
    mdl = model()
    mdl.set_inducing(X)
    assert mdl.m == m
    K, Y = dense_problem(m, rows)
    mu = mdl.solve(K, Y)
    M, ridge, sigma = mdl.M, mdl.ridge, mdl.sigma
    mdl.close()
    assert sigma == pytest.approx(sigma_of(M, 0.01), rel=1e-12)
    check_weights(K, Y, M, ridge, sigma, mu, what=f"m={m} rows={rows} slots={ref.band_slot_bucket(m)}")


# ---------------------------------------------------------------------------------------------- child processes
_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import test_hip_solve_edges as t
np.savez(sys.argv[4], **t.run_case(sys.argv[3]))
"""


def run_case(name):
    """One named problem (the same inputs in every process): its weights and what the reference needs."""
    kind, m, rows = name.split(":")
    m, rows = int(m), int(rows)
    mdl = model()
    try:
        if kind == "dense":
            mdl.set_inducing(inducing(m))
            K, Y = dense_problem(m, rows)
            mu = mdl.solve(K, Y)
        else:   # "data": rows = the frame count (data_problem)
            K, Y = data_problem(mdl, m, rows)
            mu = mdl.data_solve(Y, with_energies=True)
            info = mdl.solve_info()
        out = dict(mu=mu, M=mdl.M, ridge=mdl.ridge, sigma=mdl.sigma)
        if kind == "data":
            out.update(K=K, Y=Y, info=np.array(info))
        return out
    finally:
        mdl.close()


def child(name, **env):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        e = dict(os.environ, PYTHONPATH=ROOT, **env)
        r = subprocess.run([sys.executable, "-c", _CHILD, HERE, ROOT, name, path], env=e, capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


def check_case(name, out):
    kind, m, rows = name.split(":")
    if kind == "dense":
        K, Y = dense_problem(int(m), int(rows))
    else:
        K, Y = out["K"], out["Y"]
        assert str(out["info"]).startswith(KEPT), (name, str(out["info"]))
    check_weights(K, Y, out["M"], float(out["ridge"]), float(out["sigma"]), out["mu"], what=name)


@pytest.mark.parametrize("m", [BUCKETS[17], BUCKETS[17] + 1])
def test_band_form_hands_over_to_the_tree_form(m):
    """launch_band_qr takes the 2m x m second stage while every panel fits BQ_MAXR = 1088 rows: m <= 1072.  Beyond, the
    tree form runs by default — found by its bits: the default result equals the SGPR_BANDQR=0 child's exactly at
    m = 1073 and differs at m = 1072.  Both results are checked against the reference."""
    name = f"dense:{m}:{m + 64}"
    here = run_case(name)
    tree = child(name, SGPR_BANDQR="0")
    check_case(name, here)
    check_case(name, tree)
    same = np.array_equal(here["mu"], tree["mu"])
    assert same == (not ref.band_form_takes(m)), (m, same)


@pytest.mark.parametrize("switch,name", [
    ("SGPR_BANDQR=0", "dense:500:700"),            # the tree form where the band form would run
    ("SGPR_TSQR_LEAF=1", "dense:97:2049"),         # the row-group leaf of the first stage, tree depth 3
    ("SGPR_QR_LOOKAHEAD=0", "dense:65:8192"),      # one stream where the look-ahead would run
    ("SGPR_ENERGY_ROWS_QR=1", "data:1024:3"),      # the blocked factorisation of the energy rows (kept route: asserted)
])
def test_non_default_forms(switch, name):
    k, v = switch.split("=")
    check_case(name, child(name, **{k: v}))


# ---------------------------------------------------------------------------------------------- re-solves
@pytest.mark.parametrize("count", [1, 64, 65])
@pytest.mark.parametrize("m", [500, 1100])
def test_resolve_batches(m, count):
    """sgpr_resolve_batch (one problem per grid row; band form at m = 500, tree form at m = 1100) and resolve_many's
    split at 64: every noise against the reference on its own — eta for all of them, the forward error for the first,
    the last and the ones at the split (a host lstsq per noise would take minutes at m = 1100)."""
    mdl = model()
    mdl.set_inducing(inducing(m))
    K, Y = dense_problem(m, m + 200)
    mdl.solve(K, Y)
    M, ridge = mdl.M, mdl.ridge
    noises = np.geomspace(1e-3, 0.3, count)
    many = mdl.resolve_many(noises)
    one = mdl.resolve(float(noises[-1]))
    mdl.close()
    assert many.shape == (count, m)
    full = {0, count - 1, 63, 64} & set(range(count))
    for i, nz in enumerate(noises):
        check_weights(K, Y, M, ridge, sigma_of(M, nz), many[i], forward=i in full, what=f"noise {nz}")
    check_weights(K, Y, M, ridge, sigma_of(M, noises[-1]), one, what="resolve")


# ---------------------------------------------------------------------------------------------- resident data path
def frame_side(m, frames):
    """The smallest lips(n) frame whose rows (energy, 3N forces, 6 virials) put `frames` of them on the kept route."""
    return next(n for n in range(4, 12) if ref.data_keeps_factor(m, frames * (7 + 3 * n ** 3)))


def data_problem(mdl, m, frames):
    from autoforce_amd.workloads import lips
    mdl.set_inducing(inducing(m, n_side=13))
    n = frame_side(m, frames)
    for f in range(frames):
        mdl.data_push(*lips(n, seed=100 + f))
    K = mdl.data_get()
    assert K.shape == (frames * (7 + 3 * n ** 3), m)
    Y = np.random.default_rng(m + frames).normal(size=len(K))
    return K, Y


KEPT = "stage1=full factorisation;"   # the kept first stage, factored for the first time: the energy rows are appended


@pytest.mark.parametrize("m,frames", [(1023, 2), (1023, 16), (1024, 3), (1024, 16), (1024, 17), (2008, 2), (2008, 5)])
def test_data_solve_energy_rows(m, frames):
    """energy_rows_append on the kept first stage (rows >= m + 96, m <= 2008: asserted from the route): the kernel
    energy_rows_update_kernel<SLOTS, NE> with SLOTS 1 / 2 on either side of m + 1 = 1024 and at the route's upper end
    m = 2008, NE 2 / 4 / 16 by frame count, and the blocked factorisation beyond 16 frames.  (Its other condition,
    m + 1 > 2048, cannot be met on this route.)  The reference is built from data_get()'s matrix."""
    mdl = model()
    K, Y = data_problem(mdl, m, frames)
    mu = mdl.data_solve(Y, with_energies=True)
    info = mdl.solve_info()
    M, ridge, sigma = mdl.M, mdl.ridge, mdl.sigma
    mdl.close()
    assert info.startswith(KEPT), (info, ref.energy_rows_form(m, frames))
    check_weights(K, Y, M, ridge, sigma, mu, what=f"m={m} frames={frames} form={ref.energy_rows_form(m, frames)}")


# ---------------------------------------------------------------------------------------------- the column limit
def test_solve_at_the_column_limit():
    """m = QR_MAX_COLS = 8192 (include/sgpr_hip.h): the back substitution's right-hand side fills its 64 KB of LDS.
    Backward error only (a host QR of 8192 columns is out of reach); 2000 rows: the first stage pads to m + 1."""
    m = ref.QR_MAX_COLS
    mdl = model()
    mdl.set_inducing(inducing(m, n_side=21))
    assert mdl.m == m
    K, Y = dense_problem(m, 2000)
    mu = mdl.solve(K, Y)
    M, ridge, sigma = mdl.M, mdl.ridge, mdl.sigma
    mdl.close()
    check_weights(K, Y, M, ridge, sigma, mu, forward=False, what="m=8192")


def test_one_column_beyond_the_limit_is_refused():
    """m = 8193: SGPR_E_UNSUPPORTED, no device error — the same handle then solves at m = 64."""
    from autoforce_amd import SgprError
    from autoforce_amd._lib import E_UNSUPPORTED
    X = inducing(ref.QR_MAX_COLS + 1, n_side=21)
    mdl = model()
    mdl.set_inducing(X)
    K, Y = dense_problem(len(X), 64)
    with pytest.raises(SgprError) as e:
        mdl.solve(K, Y)
    assert e.value.code == E_UNSUPPORTED
    X64 = inducing(64)
    mdl.set_inducing(X64)
    K, Y = dense_problem(64, 200)
    mu = mdl.solve(K, Y)
    check_weights(K, Y, mdl.M, mdl.ridge, mdl.sigma, mu)
    mdl.close()
