"""The kernel exponent at every site and tile form of the library that applies it.  k(i, q) = [Z_i == Z_q] (p_i . p_q)^eta is
raised to eta in three copies of the step GEMM's epilogue (csrc/gemm_tile.inc: the four-wave / 64-row / fused body, the
eight-wave and half-tile body, the r64 / r64x3 body; each with a dedicated eta = 4, a multiply loop for the other integers up
to 64 and pow() for the rest), by the rule of csrc/gemm.hip that picks between them (twice), in the normalisation
correction of the sixteen-column training rows (rows16.inc: p^.W = eta k), in k(loc, X) (solve.inc: pow() always) and in the
border products of add_inducing.  Everywhere else the suite runs eta = 4; here every site runs the exponents of
exponent_common.ETAS (4 stays where it is), against the references test_exponent_refs_cpu.py holds against each other:

  (a) a step in every tile form of test_hip_step_edges.FORMS, on the five-species and on the sixteen-species edge frame;
  (b) orthogonal pairs (p_i . p_q = 0 exactly) in K_mm and K_nm, also below exponent 1;
  (c) the training rows in both forms, and their column subsets;
  (d) the inducing-set edits against a rebuild, and k(loc, X) against the row of K_mm;
  (e) a sharded step (the scatter form of the reverse pass);
  (f) the device MD loop against the host loop around predict().

Found here: below exponent 1 the pow() branch of the epilogue gave k = pow(0, eta - 1) * 0 = inf * 0 = NaN for an orthogonal
pair (K_mm, K_nm, the energy and every covloss of the row with it), where the references and k(loc, X) give 0.

Tolerances are those of the tests this file borrows from: the derived bounds of step_ref for K_nm, E and c, 1e-8 of the
largest component for forces and virial against the oracle, test_hip_rows' for the rows, bit equality for edits and the
device loop.  None moved."""
import numpy as np
import pytest

import step_ref as ref
import test_hip_step_edges as T
from exponent_common import ORTHO_PAIRS, ORTHO_SPECIES, RC, oracle_inducing, orthogonal_lces, sparse_frame

pytestmark = pytest.mark.gpu

STEP_ETAS = (1.0, 3.0, 64.0, 65.0, 2.5, 0.5)          # every form, on s5 and s16
MORE_ETAS = (2.0, 5.0, 1.5)                            # s5, one form per epilogue copy and the fused launch
MORE_FORMS = ("auto", "bm64_kd32_w8", "bm16_kd16_w8", "r64_wgs3", "fused")
STEP_CASES = ([(form, eta, ("s5", "s16")) for form in T.FORMS for eta in STEP_ETAS] +
              [(form, eta, ("s5",)) for form in MORE_FORMS for eta in MORE_ETAS])


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    """Tests that ran before may have left the oracle at os.cpu_count() threads, which on a machine that grants a process a
    fraction of its CPUs makes every call of it slow (kernel_rows of the 160-atom frame: seconds instead of 0.1 s).  The
    frames here are small: eight threads at the most while this file runs, then what was there."""
    from oracle import oracle as orc
    n = orc.num_threads()
    orc.set_num_threads(min(n, 8))
    yield
    orc.set_num_threads(n)


def edge_case(name, eta, seed=0):
    sp, ac, qc, g = T.EDGES[name]
    return T.model(sp, qc, seed=seed, ghosts=g > 0, eta=eta), T.frame(sp, ac, seed + 5, ghosts=g)


def weights(mdl, seed=3):
    """T.weights.  Below exponent 1 (and for some sets at other non-integer ones) v^eta is no positive definite kernel and
    a block of K_mm has negative eigenvalues: there its Cholesky factor is taken after a shift by twice the lowest one
    (choli is any block-lower matrix to the step; the references take it as it is)."""
    try:
        return T.weights(mdl, seed=seed)
    except np.linalg.LinAlgError:
        pass
    rng = np.random.default_rng(seed)
    m = mdl.m
    zq = T.slots_of(mdl.species, [x.number for x in mdl.X])
    M = mdl.M
    assert np.all(np.isfinite(M))
    C = np.zeros((m, m))
    for s in np.unique(zq):
        q = np.flatnonzero(zq == s)
        B = M[np.ix_(q, q)]
        shift = max(1e-6 * np.mean(np.diag(B)), -2.0 * np.linalg.eigvalsh(B).min())
        C[np.ix_(q, q)] = np.linalg.inv(np.linalg.cholesky(B + shift * np.eye(len(q))))
    mu = rng.normal(size=m)
    return mu, {z: 0.01 * (k + 1) for k, z in enumerate(mdl.species)}, C


def assert_form(form, mdl, fr, what):
    """The "step=" prefix, as test_edge_frames_in_every_tile_form asserts it."""
    want = T.FORMS[form][2]
    got = T.step_form(mdl)
    exp = want if want is not None else T.expected_auto(mdl, fr, chain=form not in ("chain_off", "balance_off"))
    if form == "cov_in_rev" and len(mdl.species) > 8:
        exp = T.expected_auto(mdl, fr, half=False)
    assert got.startswith(exp), (what, got, exp)


# ---------------------------------------------------------------------------------------------- (a) every tile form
@pytest.mark.parametrize("form,eta,names", STEP_CASES, ids=[f"{f}-{e:g}-{'+'.join(n)}" for f, e, n in STEP_CASES])
def test_step_in_every_tile_form(form, eta, names, monkeypatch):
    opts, _ = T.set_form(monkeypatch, form)
    for name in names:
        mdl, fr = edge_case(name, eta)
        T.apply_opts(mdl, opts)
        mu, mean, C = weights(mdl)
        out = T.check(mdl, fr, mu, mean, C, what=(form, eta, name), eta=eta)
        assert np.all(np.isfinite(out["cov"])) and np.isfinite(out["energy"]) and np.all(np.isfinite(out["forces"]))
        assert_form(form, mdl, fr, (form, eta, name))
        mdl.close()


# ---------------------------------------------------------------------------------------------- (b) orthogonal pairs
def ortho_model(eta):
    from autoforce_amd import SGPRModel
    mdl = SGPRModel(3, 3, eta, RC, species=ORTHO_SPECIES)
    mdl.set_inducing(orthogonal_lces() + T.inducing(ORTHO_SPECIES, [6, 5, 5], 2))
    return mdl


@pytest.fixture(scope="module")
def ortho_zeros():
    """Where the oracle's K_mm and K_nm are exactly zero inside a species block: the same entries at every exponent (they are
    the zero dot products), shown here at 1."""
    from oracle import oracle as orc
    X = orthogonal_lces() + T.inducing(ORTHO_SPECIES, [6, 5, 5], 2)
    ind_z, Pm, nnm = oracle_inducing(X, ORTHO_SPECIES)
    numbers, pos, cell, pbc = sparse_frame()
    nl = orc.neighbors(pos, cell, pbc, RC)
    assert np.diff(nl[0]).min() >= 2
    o = orc.frame(3, 3, RC, 1.0, np.array(ORTHO_SPECIES, np.int32), numbers, pos, cell, nl, ind_z, nnm, Pm, np.ones(len(X)),
                  want_p=False)
    zM = (orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, 1.0) == 0) & (ind_z[:, None] == ind_z[None, :])
    zK = (o["cov"] == 0) & (numbers[:, None] == ind_z[None, :])
    for a, b in ORTHO_PAIRS:
        assert zM[a, b] and zM[b, a]
    assert zM.sum() == 2 * len(ORTHO_PAIRS)
    # the atoms of species 3 in the trimers (centres with two ends of one species, ends of a trimer without 6 or without 7)
    # against the orthogonal LCEs that hold none of their neighbours' species; none against an ordinary LCE
    assert zK.sum() >= 7 and np.all(zK[:, :4].any(axis=0)) and not zK[:, 4:].any() and zK.any(axis=1).sum() >= 3
    return zM, zK


@pytest.mark.parametrize("eta", [0.5, 1.0, 1.5, 2.5])
def test_orthogonal_pairs(eta, ortho_zeros):
    """Exact zeros of the dot product in K_mm and K_nm: k = 0 at every exponent, K_mm, K_nm, E and c finite and equal to the
    references, k(loc, X) of an orthogonal LCE equal to its row of K_mm.  Forces and virial against the oracle from exponent 1
    on; below 1 the derivative of an orthogonal pair is unbounded and the oracle's forces on the atoms of such a pair are not
    finite (inf * 0): there the forces are compared on the atoms where the oracle's are finite."""
    from oracle import oracle as orc
    zM, zK = ortho_zeros
    mdl = ortho_model(eta)
    X = mdl.X
    fr = sparse_frame()
    numbers, pos, cell, pbc = fr
    zq = T.slots_of(mdl.species, [x.number for x in X])
    M = mdl.M
    assert np.all(np.isfinite(M)), (eta, int(np.count_nonzero(~np.isfinite(M))))
    assert np.all(M[zM] == 0.0)
    Q = mdl.inducing_descriptors().reshape(mdl.m, -1)
    none = np.zeros(mdl.m, bool)
    Km, bKm = ref.knm(Q, Q, zq, zq, none, none, eta)
    assert np.all(np.isfinite(bKm))
    ref.check_knm(M, Km, bKm, zq, zq, what=("K_mm", eta))
    for q in range(4):
        k, kxx = mdl.kernel_local(X[q])
        np.testing.assert_allclose(k, M[q], rtol=1e-12, atol=1e-14)
        assert np.all(k[zM[q]] == 0.0) and abs(kxx - M[q, q]) < 1e-12
    mu, mean, C = weights(mdl)
    out = T.check(mdl, fr, mu, mean, C, what=("ortho", eta), oracle=eta >= 1.0, eta=eta)
    assert np.all(np.isfinite(out["cov"])) and np.isfinite(out["energy"]) and np.all(np.isfinite(out["beta"]))
    assert np.all(out["cov"][zK] == 0.0)
    if eta < 1.0:
        ind_z, Pm, nnm = oracle_inducing(X, mdl.species)
        nl = orc.neighbors(pos, cell, pbc, RC)
        o = orc.frame(3, 3, RC, eta, np.array(mdl.species, np.int32), numbers, pos, cell, nl, ind_z, nnm, Pm, mu, want_p=False)
        fin = np.all(np.isfinite(o["forces"]), axis=1)
        assert fin.any() and not fin.all()
        fmax = np.abs(o["forces"][fin]).max()
        assert np.abs(out["forces"][fin] - o["forces"][fin]).max() <= 1e-8 * fmax
    mdl.close()


# ---------------------------------------------------------------------------------------------- (c) training rows
ROWS_SPECIES = [3, 15, 16]


@pytest.fixture(scope="module")
def rows_frame():
    from test_hip_paths import random_frame
    numbers, pos, cell = random_frame(np.random.default_rng(31), 160, 13.0, ROWS_SPECIES)
    return numbers, pos, cell, [True] * 3


@pytest.mark.parametrize("eta", [1.0, 3.0, 2.5, 0.5, 65.0])
def test_training_rows_in_both_forms(eta, rows_frame, monkeypatch):
    """kernel_rows of a 160-atom three-species frame against 40 inducing LCEs, the sixteen-columns-per-pass form (its
    normalisation correction takes p^.W = eta k) and the one-column-per-wave form, against the oracle at test_hip_rows'
    tolerances; kernel_columns bit-equal to the columns of kernel_rows in each form."""
    from oracle import oracle as orc
    from test_hip_paths import build
    from test_hip_rows import _rows_route
    numbers, pos, cell, pbc = rows_frame
    want = None
    for form in ("1", "0"):
        monkeypatch.setenv("SGPR_ROWS16", form)
        mdl, nl = build(3, 3, eta, RC, ROWS_SPECIES, numbers, pos, cell, pbc, 40, seed=5)
        if want is None:
            ind_z, Pm, nnm = oracle_inducing(mdl.X, ROWS_SPECIES)
            want = orc.kernel_rows(3, 3, RC, eta, np.array(ROWS_SPECIES, np.int32), numbers, pos, cell, nl, ind_z, nnm, Pm)
            assert all(np.all(np.isfinite(w)) for w in want)
        Ke, Kf, Kv = mdl.kernel_rows(numbers, pos, cell, pbc)
        assert _rows_route(mdl) == ("sixteen columns per workgroup pass" if form == "1" else "one column per wave")
        np.testing.assert_allclose(Ke, want[0], rtol=1e-10, atol=1e-13)
        assert np.abs(Kf - want[1]).max() <= 1e-9 * np.abs(want[1]).max(), (eta, form)
        assert np.abs(Kv - want[2]).max() <= 1e-9 * np.abs(want[2]).max(), (eta, form)
        cols = mdl.kernel_columns(numbers, pos, cell, pbc, 7, 20)
        np.testing.assert_array_equal(cols[0], Ke[7:27])
        np.testing.assert_array_equal(cols[1], Kf[:, 7:27])
        np.testing.assert_array_equal(cols[2], Kv[:, 7:27])
        mdl.close()


# ---------------------------------------------------------------------------------------------- (d) edits
def fixture_model(g, eta):
    from autoforce_amd import Local, SGPRModel
    mdl = SGPRModel(int(g["lmax"]), int(g["nmax"]), eta, float(g["rc"]), species=g["species"].tolist())
    ptr = g["ind_ptr"]
    mdl.set_inducing([Local(int(z), g["ind_nbr_z"][ptr[q]:ptr[q + 1]], g["ind_nbr_r"][ptr[q]:ptr[q + 1]])
                      for q, z in enumerate(g["ind_z"])])
    return mdl


@pytest.mark.parametrize("eta", [1.0, 2.5, 65.0])
def test_edit_entry_points_equal_rebuild(eta):
    """The sequence of test_hip_active.test_edit_entry_points_equal_rebuild on g5_mixed64 with the fixture's exponent
    overridden: the border products of add_inducing take the same epilogue as the full K_mm product."""
    from test_hip_parity import load
    g = load("g5_mixed64")
    full = fixture_model(g, eta)
    X = list(full.X)
    M = full.M
    assert np.all(np.isfinite(M))
    rows = full.kernel_rows(g["numbers"], g["positions"], g["cell"], g["pbc"])
    m = len(X)
    inc = full.scratch()
    for x in X[:3]:
        inc.add_inducing(x)
    inc.set_inducing(X[:5])
    for x in X[5:]:
        inc.add_inducing(x)
    np.testing.assert_array_equal(inc.M, M)
    for a, b in zip(inc.kernel_rows(g["numbers"], g["positions"], g["cell"], g["pbc"]), rows):
        np.testing.assert_array_equal(a, b)
    cols = inc.kernel_columns(g["numbers"], g["positions"], g["cell"], g["pbc"], 2, 3)
    np.testing.assert_array_equal(cols[0], rows[0][2:5])
    np.testing.assert_array_equal(cols[1], rows[1][:, 2:5])
    np.testing.assert_array_equal(cols[2], rows[2][:, 2:5])
    k, kxx = inc.kernel_local(X[4])
    np.testing.assert_allclose(k, M[4], rtol=1e-12, atol=1e-14)
    assert abs(kxx - M[4, 4]) < 1e-12
    inc.remove_inducing(-1)
    np.testing.assert_array_equal(inc.M, M[:-1, :-1])
    inc.remove_inducing(0)
    np.testing.assert_array_equal(inc.M, M[1:-1, 1:-1])
    keep = [m - 3, 0, 2]
    inc.select_inducing(keep)
    sel = [k + 1 for k in keep]
    np.testing.assert_array_equal(inc.M, M[np.ix_(sel, sel)])
    assert [x is X[i] for x, i in zip(inc.X, sel)] == [True] * 3
    # and against the oracle: a K_mm that is wrong in the same way in both models would pass everything above
    ind_z, Pm, nnm = oracle_inducing(X, g["species"].tolist(), rc=float(g["rc"]), lmax=int(g["lmax"]), nmax=int(g["nmax"]))
    from oracle import oracle as orc
    np.testing.assert_allclose(M, orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, eta), rtol=1e-10, atol=1e-13)
    inc.close()
    full.close()


# ---------------------------------------------------------------------------------------------- (e) a sharded step
@pytest.mark.parametrize("eta", [3.0, 2.5])
def test_sharded_shares(eta, world=3):
    """test_hip_step_edges.test_sharded_shares at three ranks (the scatter form of the reverse pass): the whole frame through
    check, then every share of K_nm and c against the references and the summed shares against the whole."""
    mdl, fr = edge_case("s5", eta)
    numbers, pos, cell, pbc = fr
    N = len(numbers)
    mu, mean, C = weights(mdl)
    full = T.check(mdl, fr, mu, mean, C, what=("world 1", eta), eta=eta)
    P = mdl.descriptors(N).reshape(N, -1)
    Q = mdl.inducing_descriptors().reshape(mdl.m, -1)
    zi = T.slots_of(mdl.species, numbers)
    zq = T.slots_of(mdl.species, [x.number for x in mdl.X])
    lone_i = np.diff(mdl.neighbors(N)[0]) == 0
    lone_q = np.array([not np.isin(x._b, mdl.species).any() for x in mdl.X])
    K, bK = ref.knm(P, Q, zi, zq, lone_i, lone_q, eta)
    Ca = ref.scale_for_c(ref.covloss(K, bK, C, zi, zq)[0]) * C
    c, bc = ref.covloss(K, bK, Ca, zi, zq)
    T.install(mdl, mu, mean, Ca)
    perm = np.argsort(np.where(zi < 0, len(mdl.species), zi), kind="stable")
    E = 0.0
    F = np.zeros((N, 3))
    beta = np.zeros(N)
    for r in range(world):
        out = mdl.predict(numbers, pos, cell, pbc, rank=r, world=world, cov=True)
        mine = perm[r::world]
        ref.check_knm(out["cov"], K, bK, zi, zq, rows=mine, what=("rank", r))
        others = np.setdiff1d(np.arange(N), mine)
        assert np.all(out["cov"][others] == 0) and np.all(out["beta"][others] == 0)
        has_q = mine[np.isin(zi[mine], zq)]
        ref.check_c(ref.c_from_beta(out["beta"]), c, bc, rows=has_q, what=("rank", r))
        got = T.step_form(mdl)
        assert got.startswith(T.expected_auto(mdl, fr, world=world, rank=r)), (r, got)
        E += out["energy"]
        F += out["forces"]
        beta += out["beta"]
    Er, bE = ref.energy(K, bK, mu, zi, [mean[z] for z in mdl.species])
    ref.check_energy(E, Er, bE + 1e-15 * world * abs(float(Er)), what="sum of shares")
    assert np.abs(F - full["forces"]).max() <= 1e-12 * np.abs(full["forces"]).max()
    has_q = np.flatnonzero(np.isin(zi, zq) & (zi >= 0))
    ref.check_c(ref.c_from_beta(beta), c, bc, rows=has_q, what="sum of shares")
    mdl.close()


# ---------------------------------------------------------------------------------------------- (f) the device loop
@pytest.mark.parametrize("eta", [3.0, 2.5])
def test_device_loop_equals_the_host_loop(eta):
    """Eight velocity-Verlet steps (friction 0) of md_run on g5_si32's frame against the host loop around predict() on the
    same handle, as test_hip_md.test_device_langevin_equals_the_host_loop_bit_for_bit compares them: energies and the
    largest covloss bit for bit, the temperature to rounding, the final positions and velocities bit for bit."""
    from autoforce_amd.workloads import langevin_nvt, langevin_nvt_device
    from test_hip_md import _PredictCalc
    from test_hip_parity import load
    g = load("g5_si32")
    mdl = fixture_model(g, eta)
    mdl.set_weights(g["mu"], vscale=dict(zip(g["vscale_z"].tolist(), g["vscale"].tolist())), choli=g["choli"])
    numbers, pos, cell, pbc = g["numbers"], g["positions"], g["cell"], g["pbc"]
    steps = 8
    calc = _PredictCalc(mdl)
    host = [(s, E, Tk, w, p.copy(), v.copy()) for s, E, Tk, w, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, friction=0.0, seed=3)]
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, steps, temperature=600.0, dt_fs=1.0, friction=0.0, seed=3, chunk=32))
    assert len(dev) == len(host) == steps + 1
    for (s0, E0, T0, _, _, _), (s1, E1, T1, bmax), b0 in zip(host, dev, calc.betas):
        assert s0 == s1
        assert E0 == E1, (s0, E0, E1)
        assert abs(T0 - T1) <= 1e-12 * T0
        assert bmax == b0
    assert len({E for _, E, _, _, _, _ in host}) == steps + 1 and np.all(np.isfinite([E for _, E, _, _, _, _ in host]))
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][4])
    assert np.array_equal(st["velocities"], host[-1][5])
    mdl.close()
