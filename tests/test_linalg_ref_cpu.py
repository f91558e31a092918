"""The host references of test_hip_solve_edges.py, checked on CPU: exact where they claim to be exact, and sharp enough
that the least-squares check fails on errors far below the tolerances of the device tests."""
import numpy as np
import pytest

import linalg_ref as ref


@pytest.mark.parametrize("n", [1, 2, 3, 64, 129, 1000])
def test_integer_spd_is_exact_and_well_conditioned(n):
    A, L0 = ref.integer_spd(n, seed=n)
    Li = L0.astype(np.int64)
    assert np.array_equal(A, (Li @ Li.T).astype(np.float64))
    assert np.array_equal(A, A.T)
    assert np.all(np.triu(L0, 1) == 0) and L0.diagonal().min() >= 8
    assert np.linalg.cond(A) < 50
    np.testing.assert_allclose(np.linalg.cholesky(A), L0, rtol=0, atol=n * ref.EPS * 50 * 16)


def test_long_double_cholesky_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    rng = np.random.default_rng(1)
    V = rng.normal(size=(24, 24))
    A = V @ V.T + 0.1 * np.eye(24)
    mpmath.mp.dps = 40
    Lm = mpmath.cholesky(mpmath.matrix(A.tolist()))
    Lm = np.array([[float(Lm[i, j]) for j in range(24)] for i in range(24)])
    L = ref.cholesky_ld(A)
    np.testing.assert_allclose(L.astype(np.float64), Lm, rtol=1e-14, atol=1e-15)
    assert np.all(np.triu(L, 1) == 0)


def test_long_double_triangular_inverse():
    A, L0 = ref.integer_spd(200, seed=4)
    X = ref.tril_inverse_ld(L0)
    assert np.all(np.triu(X, 1) == 0)
    E = X @ L0.astype(np.longdouble) - np.eye(200, dtype=np.longdouble)
    assert float(np.abs(E).max()) < 1e-17
    np.testing.assert_allclose(X.astype(np.float64), np.linalg.inv(L0), rtol=0, atol=1e-14)


def _problem(rows=100, m=40, seed=0):
    rng = np.random.default_rng(seed)
    K, Y = rng.normal(size=(rows, m)), rng.normal(size=rows)
    V = rng.normal(size=(m, m))
    G = V @ V.T / m + 1e-3 * np.eye(m)
    return K, Y, G, 0.05


def test_eta_of_the_exact_solution_is_rounding():
    K, Y, G, sigma = _problem()
    A, b = ref.stacked_system(K, Y, G, sigma)
    x, tol, kappa = ref.lstsq_forward(A, b)
    assert ref.lstsq_eta(K, Y, x, sigma, G) < 1e-15
    # the normal-equation form equals the explicit stacked one
    assert ref.lstsq_eta(A, b, x) == pytest.approx(ref.lstsq_eta(K, Y, x, sigma, G), rel=1e-6, abs=1e-18)
    assert tol < 1e-11 and kappa > 1


def test_eta_catches_one_perturbed_weight():
    """One entry of an exact solution moved by 1e-9 relative: eta rises four orders above the 1e-13 the device tests
    allow."""
    K, Y, G, sigma = _problem()
    A, b = ref.stacked_system(K, Y, G, sigma)
    x, *_ = np.linalg.lstsq(A, b, rcond=None)
    for j in (0, 17, 39):
        y = x.copy()
        y[j] *= 1 + 1e-9
        assert ref.lstsq_eta(K, Y, y, sigma, G) > 1e-13, j


def test_eta_catches_one_perturbed_column_of_R():
    """A QR solve whose R has one column wrong by 1e-9 relative (a single bad element of a panel's update)."""
    K, Y, G, sigma = _problem()
    A, b = ref.stacked_system(K, Y, G, sigma)
    Q, R = np.linalg.qr(A)
    assert ref.lstsq_eta(K, Y, np.linalg.solve(R, Q.T @ b), sigma, G) < 1e-15
    for j in (0, 20, 39):
        Rp = R.copy()
        Rp[:j + 1, j] *= 1 + 1e-9
        assert ref.lstsq_eta(K, Y, np.linalg.solve(Rp, Q.T @ b), sigma, G) > 1e-13, j


def test_forward_bound_separates_solver_rounding_from_a_real_error():
    """An independent backward-stable solver (SVD-based lstsq) lands within the bound of the QR solution; a weight moved
    by 1e-9 relative does not."""
    K, Y, G, sigma = _problem()
    A, b = ref.stacked_system(K, Y, G, sigma)
    x, tol, _ = ref.lstsq_forward(A, b)
    assert tol < 1e-11
    y, *_ = np.linalg.lstsq(A, b, rcond=None)
    assert np.linalg.norm(y - x) <= tol * np.linalg.norm(x)
    for j in (int(np.argmax(np.abs(x))), 0, 39):
        z = x.copy()
        z[j] *= 1 + 1e-9
        assert np.linalg.norm(z - x) > tol * np.linalg.norm(x), j


def test_data_route_restatement():
    """The kept first stage needs rows >= m + 96 and m <= 2008; on it the energy-row kernel takes up to 16 frames."""
    assert ref.data_keeps_factor(1023, 1119) and not ref.data_keeps_factor(1023, 1118)
    assert ref.data_keeps_factor(2008, 10000) and not ref.data_keeps_factor(2009, 10000)
    assert ref.energy_rows_form(1023, 2) == (1, 2) and ref.energy_rows_form(1024, 3) == (2, 4)
    assert ref.energy_rows_form(1024, 16) == (2, 16) and ref.energy_rows_form(1024, 17) == "blocked"
    assert all(ref.energy_rows_form(m, 5) != "blocked" for m in range(1, 2009))


def test_band_dispatch_restatement():
    """The 2m x m second stage: panel k0 spans k0 + 64 rows, the last one 2m - k0; the flat-panel form takes every
    panel up to 1088 rows."""
    assert ref.band_panel_rows(64) == [64, 96]
    assert ref.band_panel_rows(33) == [64, 34]
    assert max(ref.band_panel_rows(1072)) == 1088 and ref.band_form_takes(1072)
    assert max(ref.band_panel_rows(1073)) == 1090 and not ref.band_form_takes(1073)
    edges = ref.band_bucket_edges()
    assert sorted(edges) == list(ref.BQ_SLOTS)
    for b, m in edges.items():
        assert ref.band_slot_bucket(m) == b and max(ref.band_panel_rows(m)) <= 64 * b
        if b != 17:
            assert ref.band_slot_bucket(m + 1) > b
    assert edges[17] == 1072
