"""CPU tests of workloads.neb_fire, the host twin — and, ASE not being a dependency, the definition — of the nudged elastic band
inside the device loop (sgpr_md_neb, md_neb.inc): ASE's default `aseneb` method under FIRE.  The calculators are small analytic
ones defined here: a periodic sum of cosines with a cosine pair term (energy, forces and a made-up covloss), and a two-
dimensional double well with a curved valley whose saddle energy is known.  The twin is checked against a dense numpy
restatement of the formulas with np.vdot on whole arrays — the two differ in summation order only, and the allowed difference is
built from the magnitudes of the summed terms —; then the invariants of the projection, the held components, the tie rule of
imax, the minimum-image refusal, and a band that converges onto the saddle."""
import numpy as np
import pytest

from autoforce_amd.workloads import neb_check_band, neb_fire

EPS = np.finfo(float).eps
L = 6.0
CELL = np.diag([L, L, L])
PBC = [True, True, True]


class _Cosines:
    """E = sum_i sum_c A_c (1 - cos(w x_ic)) + B sum_(i, i+1) sum_c (1 - cos(w (x_ic - x_(i+1)c))), w = 2 pi / L: periodic
    and smooth; the covloss is made up, 0.05 + 0.04 sin(w x_i0 + i)."""
    implemented_properties = ["energy", "forces"]
    A, B, W = np.array([0.30, 0.45, 0.20]), 0.15, 2.0 * np.pi / L

    def __init__(self):
        self.calls = 0

    def get_property(self, name, atoms=None):
        x, w = atoms.positions, self.W
        d = x[:-1] - x[1:]
        E = float((self.A * (1.0 - np.cos(w * x))).sum() + self.B * (1.0 - np.cos(w * d)).sum())
        F = -(self.A * w * np.sin(w * x))
        g = self.B * w * np.sin(w * d)
        F[:-1] -= g
        F[1:] += g
        self._beta = 0.05 + 0.04 * np.sin(w * x[:, 0] + np.arange(len(x)))
        self.calls += 1
        return dict(energy=E, forces=F)[name]

    def get_covloss(self):
        return self._beta


class _Listed:
    """A small constant force; the energies come from a list, one per evaluated image, cycling."""
    implemented_properties = ["energy", "forces"]

    def __init__(self, energies):
        self.energies, self.calls = list(energies), -1

    def get_property(self, name, atoms=None):
        if name == "forces":
            self.calls += 1
            return np.full(atoms.positions.shape, 1e-3)
        return self.energies[self.calls % len(self.energies)]

    def get_covloss(self):
        return np.zeros(1)


def _band(N=7, K=4, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, L, size=(N, 3))
    b = a + rng.uniform(-0.8, 0.8, size=(N, 3))
    return np.array([a + (i / (K + 1.0)) * (b - a) + (0.05 * rng.normal(size=(N, 3)) if 0 < i < K + 1 else 0.0) for i in range(K + 2)])


def _mic(d):
    """d - rint(d h^-1) h for the diagonal cell of these tests, elementwise (no sum of more than one non-zero term)."""
    return d - np.rint(d / L) * L


def _dense(o, images_now, k, climb, fx):
    """The projection of one evaluation, restated with np.vdot on whole arrays.  Returns G and, per image, the bound on
    |G_twin - G_dense| per component that follows from the magnitudes of the summed terms."""
    F = o["forces"] if fx is None else np.where(fx[None], 0.0, o["forces"])
    E = o["energies"]
    K, n = len(F), F[0].size
    t = [_mic(images_now[i] - images_now[i - 1]) for i in range(1, K + 2)]
    imax = max(range(K), key=lambda i: (E[i], i))
    G, tol = np.zeros_like(F), np.zeros(K)
    for i in range(K):
        ti, tn = t[i], t[i + 1]
        tau = tn if i < imax else (ti if i > imax else ti + tn)
        ft, tt = np.vdot(F[i], tau), np.vdot(tau, tau)
        spr = np.vdot(k * ti - k * tn, tau)
        if climb and i == imax:
            G[i] = F[i] - 2.0 * ft / tt * tau
            spr = 0.0
        else:
            G[i] = F[i] - ft / tt * tau - spr / tt * tau
        # the sums the twin and np.vdot order differently, by the magnitudes of their terms (the twin expands the dots with
        # tau = t_i + t_(i+1) into the five sums of the image: the expanded terms bound both forms)
        parts = [tn] if i < imax else ([ti] if i > imax else [ti, tn])
        a_ft = sum(np.abs(F[i] * q).sum() for q in parts)
        a_tt = sum(np.abs(q1 * q2).sum() for q1 in parts for q2 in parts)
        a_spr = 0.0 if (climb and i == imax) else k * sum((np.abs(ti * q).sum() + np.abs(tn * q).sum()) for q in parts)
        e_ft, e_tt, e_spr = n * EPS * a_ft, n * EPS * a_tt, n * EPS * a_spr
        c = (2.0 * abs(ft) if (climb and i == imax) else abs(ft) + abs(spr)) / tt
        dc = (2.0 if (climb and i == imax) else 1.0) * (e_ft + e_spr) / tt + c * e_tt / tt + 8.0 * EPS * (a_ft + a_spr) / tt
        tol[i] = 4.0 * (dc * np.abs(tau).max() + 8.0 * EPS * (np.abs(F[i]).max() + c * np.abs(tau).max()))
    if fx is not None:
        G = np.where(fx[None], 0.0, G)
    return G, tol, imax, t


@pytest.mark.parametrize("climb", [False, True], ids=["plain", "climb"])
@pytest.mark.parametrize("held", [False, True], ids=["free", "held"])
def test_the_twin_is_the_dense_restatement_up_to_summation_order(climb, held):
    images = _band()
    N, K, k = images.shape[1], len(images) - 2, 0.1
    fx = (np.random.default_rng(4).random((N, 3)) < 0.25) if held else None
    numbers = np.array([3, 15, 16, 3, 16, 3, 15])
    rows = list(neb_fire(_Cosines(), numbers, images, CELL, PBC, 25, 1e-9, k=k, climb=climb, fixed=fx))
    assert len(rows) == 26
    n = 3 * N
    for o in rows:
        now = np.concatenate([images[:1], o["band"], images[-1:]])
        G, tol, imax, _ = _dense(o, now, k, climb, fx)
        assert o["imax"] == imax + 1
        for i in range(K):
            d = np.abs(o["G"][i] - G[i]).max()
            assert d <= tol[i], (o["n"], i, d, tol[i])
        assert tol.max() < 1e-12                                     # (the bound itself is tight: nothing hides behind it)
        g2 = (G * G).sum(axis=2)
        assert abs(o["gmax2"] - g2.max()) <= 8.0 * EPS * g2.max() + 4.0 * np.sqrt(g2.max()) * tol.max()
        v = o["velocities"]
        Pd = np.vdot(G, v)
        bound = 4.0 * (K * n * EPS * np.abs(G * v).sum() + tol.max() * np.abs(v).sum())
        assert abs(o["P"] - (0.0 if o["n"] == 0 else Pd)) <= bound, (o["n"], o["P"], Pd, bound)
        assert (o["covmax"] == [0.05 + 0.04 * np.sin(_Cosines.W * b[:, 0] + np.arange(N)).max() for b in o["band"]]).all()
        assert o["cimg"] == 1 + int(np.argmax(o["covmax"]))
    # FIRE's recurrence: positive power raises the time step after nmin steps, negative power halves it
    dts = [o["dt"] for o in rows]
    assert max(dts) > 0.1 and all(rows[j + 1]["dt"] <= 1.1 * rows[j]["dt"] * (1 + 4 * EPS) for j in range(25))
    for a, b in zip(rows[:-1], rows[1:]):   # the move: v' = alpha v + beta G, x' = x + cd v', |cd v'| <= maxstep
        step = b["band"] - a["band"]
        assert np.sqrt((step ** 2).sum()) <= 0.2 * (1 + 1e-12)
        free = np.ones((N, 3), bool) if fx is None else ~fx
        assert np.array_equal(step[:, ~free], np.zeros_like(step[:, ~free]))
        if a["P"] <= 0.0:                                            # v was dropped: the step out of `a` is along its G alone
            cos = np.vdot(step, a["G"]) / np.sqrt(np.vdot(step, step) * np.vdot(a["G"], a["G"]))
            assert cos > 1.0 - 1e-12


def test_projection_invariants():
    """Ordinary images: G.tau is the spring term alone (the model's force along the tangent is gone).  The climbing image: the
    tangential force is reversed, the perpendicular part untouched, and no spring acts."""
    images = _band(seed=3)
    N, K, k = images.shape[1], len(images) - 2, 0.1
    numbers = np.arange(N) % 3
    n = 3 * N
    for climb in (False, True):
        for o in neb_fire(_Cosines(), numbers, images, CELL, PBC, 6, 1e-9, k=k, climb=climb):
            now = np.concatenate([images[:1], o["band"], images[-1:]])
            _, tol, imax, t = _dense(o, now, k, climb, None)
            for i in range(K):
                ti, tn, F, G = t[i], t[i + 1], o["forces"][i], o["G"][i]
                tau = tn if i < imax else (ti if i > imax else ti + tn)
                slack = 4.0 * (n * EPS * (np.abs(G * tau).sum() + np.abs(F * tau).sum() + k * (np.abs(ti * tau).sum() + np.abs(tn * tau).sum()))
                               + tol[i] * np.abs(tau).sum())
                if climb and i == imax:
                    assert abs(np.vdot(G, tau) + np.vdot(F, tau)) <= slack
                    perp = lambda u: u - np.vdot(u, tau) / np.vdot(tau, tau) * tau
                    assert np.abs(perp(G) - perp(F)).max() <= slack
                else:
                    assert abs(np.vdot(G, tau) + np.vdot(k * ti - k * tn, tau)) <= slack


def test_held_components_never_move_and_carry_no_velocity():
    images = _band(seed=5)
    N = images.shape[1]
    fx = np.zeros((N, 3), bool)
    fx[1] = True                 # a whole atom
    fx[4, 0] = fx[5, 2] = True   # single components
    rows = list(neb_fire(_Cosines(), np.arange(N) % 3, images, CELL, PBC, 20, 1e-9, fixed=fx))
    for o in rows:
        assert np.array_equal(o["band"][:, fx], images[1:-1][:, fx])
        assert not o["velocities"][:, fx].any() and not o["G"][:, fx].any()
    assert np.abs(rows[-1]["band"][:, ~fx] - images[1:-1][:, ~fx]).min() > 0.0
    one = list(neb_fire(_Cosines(), np.arange(N) % 3, images, CELL, PBC, 3, 1e-9, fixed=fx.all(axis=1)))   # the [N] form: atom 1
    assert np.array_equal(one[-1]["band"][:, 1], images[1:-1, 1]) and np.abs(one[-1]["band"][:, 4] - images[1:-1, 4]).min() > 0.0


def test_imax_is_the_later_image_on_a_tie():
    images = _band(K=3, seed=6)
    N = images.shape[1]
    for energies, want in (([1.0, 2.0, 2.0], 3), ([2.0, 2.0, 1.0], 2), ([3.0, 1.0, 2.0], 1), ([1.0, 1.0, 1.0], 3)):
        o = next(neb_fire(_Listed(energies), np.zeros(N, int), images, CELL, PBC, 0, 1e-9))
        assert o["imax"] == want, (energies, o["imax"])


def test_the_rounding_on_a_triclinic_cell_is_numpy_s():
    """A cell with all nine components: the twin's minimum-image form against d - rint(d inv(h)) h with numpy's inverse and
    matrix products (a transposed inverse would give other integers), whole cell vectors taken out again, and the refusal's
    perpendicular widths against volume / |a x b|."""
    from autoforce_amd.workloads import _neb_cell, _neb_mic
    cell = np.array([[6.0, 0.4, -0.7], [1.5, 5.2, 0.9], [-1.1, 2.0, 4.8]])
    rng = np.random.default_rng(8)
    small = rng.uniform(-1.0, 1.0, size=(40, 3))
    shifts = rng.integers(-3, 4, size=(40, 3)).astype(float)
    d = small + shifts @ cell
    for pbc in ([True, True, True], [True, False, True]):
        h, hi, pb = _neb_cell(cell, pbc)
        assert np.abs(np.array(hi) - np.linalg.inv(cell)).max() <= 16 * EPS * np.abs(np.linalg.inv(cell)).max()
        got = _neb_mic(d, h, hi, pb)
        want = d - np.where(pbc, np.rint(d @ np.linalg.inv(cell)), 0.0) @ cell
        scale = np.abs(d).max() + 3.0 * np.abs(cell).sum()
        assert np.abs(got - want).max() <= 16 * EPS * scale
        if all(pbc):                                                 # the shifts are gone, the small part is what is left
            assert np.abs(got - _neb_mic(small, h, hi, pb)).max() <= 64 * EPS * scale
    vol = abs(np.linalg.det(cell))
    widths = [vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)]
    wmin = min(widths)
    base = rng.uniform(0.0, 1.0, size=(3, 3)) @ cell
    n = np.cross(cell[(int(np.argmin(widths)) + 1) % 3], cell[(int(np.argmin(widths)) + 2) % 3])
    n = n / np.linalg.norm(n)
    for length, ok in ((0.45 * wmin, True), (0.55 * wmin, False)):   # along the normal of the narrowest pair of faces
        band = np.array([base, base + length * n, base + length * n])
        frac = (length * n) @ np.linalg.inv(cell)
        if ok:
            assert np.abs(frac).max() < 0.5
            neb_check_band(band, cell, [True] * 3)
        else:
            with pytest.raises(ValueError, match="cannot recover"):
                neb_check_band(band, cell, [True] * 3)


def test_a_band_the_rounding_cannot_recover_is_refused():
    images = _band(seed=7)
    N = images.shape[1]
    neb_check_band(images, CELL, PBC)
    wrapped = images.copy()
    wrapped[2, 3] += CELL[0] - 2.0 * CELL[2]                         # whole cell vectors: the rounding takes them out
    neb_check_band(wrapped, CELL, PBC)
    rows = [next(neb_fire(_Cosines(), np.zeros(N, int), im, CELL, PBC, 0, 1e-9)) for im in (images, wrapped)]
    assert np.abs(rows[0]["G"] - rows[1]["G"]).max() < 1e-12
    half = images.copy()
    half[3, 2] = half[2, 2] + 0.5 * CELL[1]                          # half a cell: rint may go either way
    long = images.copy()
    long[3, 2] = long[2, 2] + 0.4 * (CELL[0] + CELL[1] + CELL[2])    # every fraction below 1/2, longer than half the cell's width
    for bad in (half, long):
        with pytest.raises(ValueError, match="cannot recover"):
            neb_check_band(bad, CELL, PBC)
        with pytest.raises(ValueError, match="cannot recover"):
            next(neb_fire(_Cosines(), np.zeros(N, int), bad, CELL, PBC, 0, 1e-9))
    neb_check_band(long, CELL, [False, False, False])                # no periodic direction: nothing is rounded
    with pytest.raises(ValueError, match="interior images"):
        next(neb_fire(_Cosines(), np.zeros(N, int), images[:2], CELL, PBC, 0, 1e-9))
    with pytest.raises(ValueError, match="interior images"):
        next(neb_fire(_Cosines(), np.zeros(N, int), np.repeat(images[:1], 19, axis=0), CELL, PBC, 0, 1e-9))


class _DoubleWell:
    """Atom 0 in V = (B/2)(1 - cos(2 w x)) + C (1 - cos(w u)) + C (1 - cos(w z)), u = y - s sin^2(w x), w = 2 pi / L: minima at
    x = 0 and x = L/2 (y = z = 0), a curved valley y = s sin^2(w x) between them whose highest point, x = L/4, y = s, is the
    saddle with V = B exactly.  Atom 1 is a spectator in A (1 - cos(w r)) per component, minimum at the origin."""
    implemented_properties = ["energy", "forces"]
    B, C, S, A, W = 0.4, 0.6, 0.5, 0.3, 2.0 * np.pi / L

    def get_property(self, name, atoms=None):
        (x, y, z), r1, w = atoms.positions[0], atoms.positions[1], self.W
        u = y - self.S * np.sin(w * x) ** 2
        E = 0.5 * self.B * (1.0 - np.cos(2.0 * w * x)) + self.C * (1.0 - np.cos(w * u)) + self.C * (1.0 - np.cos(w * z))
        E += (self.A * (1.0 - np.cos(w * r1))).sum()
        dVdu = self.C * w * np.sin(w * u)
        F = np.zeros((2, 3))
        F[0, 0] = -(self.B * w * np.sin(2.0 * w * x) - dVdu * self.S * w * np.sin(2.0 * w * x))
        F[0, 1] = -dVdu
        F[0, 2] = -self.C * w * np.sin(w * z)
        F[1] = -self.A * w * np.sin(w * r1)
        return dict(energy=float(E), forces=F)[name]

    def get_covloss(self):
        return np.zeros(2)


def test_the_climbing_image_converges_onto_the_saddle():
    """K = 3 on the double well, the interior images off the valley and off its symmetry.  At convergence every row of G is
    shorter than fmax; the climbing image's G is its force with the tangential part reversed — the same length —, so the
    force on the climbing image obeys |F|^2 <= N fmax^2 (N = 2 rows).  Around the saddle F = -H d and E - E_s = d.H.d / 2
    to second order, hence |E - E_s| <= |F|^2 / (2 lambda) <= N fmax^2 / (2 lambda) with lambda the smallest |eigenvalue| of the
    Hessian there: H = diag(-2 B w^2, C w^2, C w^2) for atom 0 (the valley's tangent is along x at the saddle, grad u = (0, 1))
    and A w^2 for the spectator's components.  The third-order remainder is O(|d|^3 V''') with |d| <= sqrt(N) fmax / lambda ~
    1e-2: a factor of two on the bound covers it."""
    pot = _DoubleWell
    fmax, w = 1e-3, pot.W
    lam = min(2.0 * pot.B * w * w, pot.C * w * w, pot.A * w * w)
    ends = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[L / 2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])   # (the spectator at its minimum)
    rng = np.random.default_rng(2)
    images = np.array([ends[0] + (i / 4.0) * (ends[1] - ends[0]) for i in range(5)])
    images[1:-1] += 0.05 * rng.normal(size=(3, 2, 3))
    rows = list(neb_fire(pot(), np.array([3, 16]), images, CELL, PBC, 3000, fmax, k=0.1, climb=True))
    last = rows[-1]
    print("evaluations", len(rows), "E", last["energies"], "gmax", np.sqrt(last["gmax2"]))
    assert last["converged"] and len(rows) < 3000
    assert last["gmax2"] < fmax * fmax and all(o["gmax2"] >= fmax * fmax for o in rows[:-1])
    top = last["imax"] - 1
    tol = 2.0 * (2 * fmax * fmax / (2.0 * lam))
    assert abs(last["energies"][top] - pot.B) <= tol, (last["energies"][top] - pot.B, tol)
    assert abs(last["band"][top, 0, 0] - L / 4.0) < 0.05 and abs(last["band"][top, 0, 1] - pot.S) < 0.05   # ... and it IS the saddle
    assert last["energies"][top] > max(np.delete(last["energies"], top)) + 0.05
