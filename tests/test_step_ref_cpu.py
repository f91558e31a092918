"""The step references of tests/step_ref.py on host data (no GPU): the checks pass the reference's own float64 rounding and
reject the defects a tile table could cause: a 1e-9 relative error in one K_nm entry, one 32-wide k-slice dropped from one
atom's covloss sum (an error of about 1e-12 in c), one nonzero cross-species K entry, a swapped species range in the
energy.  Also the restated tile-count arithmetic of csrc/api.hip on hand cases."""
import numpy as np
import pytest

import step_ref as ref

ETA = 4.0
SLICE = np.arange(64, 96)     # a 32-aligned k-slice inside species 1's inducing block [33, 103)
I0 = 25                       # the species-1 atom that sees almost nothing of that slice


def _data(seed=0):
    """Three species (33, 70, 5 inducing LCEs; 20, 30, 3 atoms), one lone atom and one lone LCE of species 2, choli scaled
    so that max c = 0.9.  Atom I0 lies nearly orthogonal to the LCEs of SLICE: their K entries are about 1e-10."""
    rng = np.random.default_rng(seed)
    D = 48
    zq = np.repeat([0, 1, 2], [33, 70, 5])
    zi = np.repeat([0, 1, 2], [20, 30, 3])
    Q = rng.normal(size=(len(zq), D))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    P = np.zeros((len(zi), D))
    for i, s in enumerate(zi):
        p = Q[rng.choice(np.flatnonzero(zq == s))] + 0.5 * rng.normal(size=D) / np.sqrt(D)
        P[i] = p / np.linalg.norm(p)
    U = np.linalg.qr(Q[SLICE].T)[0]
    r = rng.normal(size=D)
    r -= U @ (U.T @ r)
    P[I0] = r / np.linalg.norm(r) + 0.02 * U[:, 0]
    P[I0] /= np.linalg.norm(P[I0])
    li, lq = np.zeros(len(zi), bool), np.zeros(len(zq), bool)
    li[-1] = lq[-1] = True
    P[-1], Q[-1] = 0.0, 0.0
    M = ref.knm(Q, Q, zq, zq, lq, lq, ETA)[0].astype(float)
    C = np.linalg.inv(np.linalg.cholesky(M + 1e-10 * np.eye(len(zq))))
    C[zq[:, None] != zq[None, :]] = 0.0
    K, bK = ref.knm(P, Q, zi, zq, li, lq, ETA)
    C *= ref.scale_for_c(ref.covloss(K, bK, C, zi, zq)[0])
    mu = rng.normal(size=len(zq))
    mean = [0.25, -0.5, 1.0]
    return dict(P=P, Q=Q, zi=zi, zq=zq, li=li, lq=lq, C=C, K=K, bK=bK, mu=mu, mean=mean)


@pytest.fixture(scope="module")
def d():
    return _data()


def _device_like(d):
    """What a correct device reports: K rounded to float64, E rounded, beta = sqrt(1 - c) rounded, c read back from it."""
    Kd = d["K"].astype(float)
    E, bE = ref.energy(d["K"], d["bK"], d["mu"], d["zi"], d["mean"])
    c, bc = ref.covloss(d["K"], d["bK"], d["C"], d["zi"], d["zq"])
    beta = np.sqrt(1.0 - c.astype(float))
    return Kd, float(E), ref.c_from_beta(beta), (E, bE, c, bc)


def test_references_agree_with_float64_and_pass_unperturbed(d):
    Kd, Ed, cd, (E, bE, c, bc) = _device_like(d)
    assert c.max() <= 0.9 + 1e-15 and c.max() >= 0.9 - 1e-12
    ref.check_knm(Kd, d["K"], d["bK"], d["zi"], d["zq"])
    ref.check_energy(Ed, E, bE)
    ref.check_c(cd, c, bc)
    # the same quantities in plain float64 land inside the bounds too
    K64 = np.zeros_like(Kd)
    for i, s in enumerate(d["zi"]):
        for q, t in enumerate(d["zq"]):
            if s == t:
                K64[i, q] = 1.0 if (d["li"][i] and d["lq"][q]) else 0.0 if (d["li"][i] or d["lq"][q]) else float(d["P"][i] @ d["Q"][q]) ** 4
    ref.check_knm(K64, d["K"], d["bK"], d["zi"], d["zq"])
    ref.check_c(1.0 - np.sqrt(1.0 - ((K64 @ d["C"].T) ** 2).sum(axis=1)) ** 2, c, bc)
    ref.check_energy(float(np.sum(K64 @ d["mu"])) + 0.25 * 20 - 0.5 * 30 + 1.0 * 3, E, bE)
    # the lone-atom rule: two lone atoms of one species see lone_weight, a lone atom sees 0 elsewhere
    assert d["K"][-1, -1] == 1 and np.all(d["K"][-1, :-1] == 0) and np.all(d["K"][:-1, -1] == 0)
    assert ref.knm(d["P"], d["Q"], d["zi"], d["zq"], d["li"], d["lq"], ETA, lone_weight=3)[0][-1, -1] == 3


def test_knm_check_rejects_a_1e9_error_in_one_entry(d):
    Kd = _device_like(d)[0]
    for i, q in ((0, 0), (40, 60), (I0, 70)):
        bad = Kd.copy()
        bad[i, q] *= 1 + 1e-9
        with pytest.raises(AssertionError, match="K_nm"):
            ref.check_knm(bad, d["K"], d["bK"], d["zi"], d["zq"])


def test_knm_check_rejects_one_nonzero_cross_species_entry(d):
    Kd = _device_like(d)[0]
    bad = Kd.copy()
    bad[3, 50] = 1e-300       # atom of species 0, LCE of species 1
    with pytest.raises(AssertionError, match="cross-species"):
        ref.check_knm(bad, d["K"], d["bK"], d["zi"], d["zq"])


def test_covloss_check_rejects_one_dropped_k_slice(d):
    """The slice [64, 96) of atom I0's reduction, dropped as a tile with kb or ke one slice short would: c moves by
    about 1e-12, far inside the beta tolerances (2e-6) of the older tests."""
    _, _, cd, (_, _, c, bc) = _device_like(d)
    Kd = d["K"].copy()
    Kd[I0, SLICE] = 0
    cb = ref.covloss(Kd, d["bK"], d["C"], d["zi"], d["zq"])[0]
    delta = float(abs(c[I0] - cb[I0]))
    assert 1e-13 < delta <= 1e-10, delta
    bad = cd.copy()
    bad[I0] = ref.c_from_beta(np.sqrt(1.0 - float(cb[I0])))
    with pytest.raises(AssertionError, match="covloss"):
        ref.check_c(bad, c, bc)


def test_energy_check_rejects_a_swapped_species_range(d):
    """E summed with species 0's rows against species 1's inducing range and back (their K entries there are zero)."""
    E, bE = ref.energy(d["K"], d["bK"], d["mu"], d["zi"], d["mean"])
    qoff = ref.qoffsets(d["zq"], 3)
    Kd = d["K"].astype(float)
    rng_of = {0: slice(qoff[1], qoff[2]), 1: slice(qoff[0], qoff[1]), 2: slice(qoff[2], qoff[3])}
    bad = sum(float(Kd[i, rng_of[s]] @ d["mu"][rng_of[s]]) for i, s in enumerate(d["zi"])) + 0.25 * 20 - 0.5 * 30 + 3.0
    ref.check_energy(float(E), E, bE)
    with pytest.raises(AssertionError, match="energy"):
        ref.check_energy(bad, E, bE)


# ---------------------------------------------------------------------------------------------- tile counts
QOFF = [0, 40, 100]   # m = 100: two column tiles, species 1's range [40, 100) starts inside the first


@pytest.mark.parametrize("edge,knm,cov", [
    (32, [(0, 0, 0, 64), (1, 0, 0, 64), (1, 1, 0, 64)],
     [(0, 0, 0, 64), (1, 0, 32, 64), (1, 1, 32, 128)]),
    (31, [(0, 0, 0, 64), (0, 1, 0, 64), (1, 0, 0, 64), (1, 1, 0, 64)],
     [(0, 0, 0, 64), (0, 1, 0, 128), (1, 0, 32, 64), (1, 1, 32, 128)]),
    (33, [(0, 0, 0, 64), (1, 0, 0, 64), (1, 1, 0, 64)],
     [(0, 0, 0, 64), (1, 0, 0, 64), (1, 1, 0, 128)]),
])
def test_tiles_at_a_species_edge_on_and_beside_a_32_row_edge(edge, knm, cov):
    aoff, cnt = [0, edge, 50], 50
    assert ref.tiles(aoff, QOFF, cnt, 100, 64, 0, 32) == knm
    assert ref.tiles(aoff, QOFF, cnt, 100, 64, 2, 32) == cov
    w = ref.tiles(aoff, QOFF, cnt, 100, 64, 1, 32)
    assert w == [(0, 0, 0, 64 if edge >= 32 else 128), (1, 0, 32 if edge <= 32 else 0, 128)]
    # a general (not lower) choli: every covloss tile reduces over the whole range
    assert ref.tiles(aoff, QOFF, cnt, 100, 64, 2, 32, choli_lower=False)[0] == (0, 0, 0, 64 if edge >= 32 else 128)


def test_tiles_of_a_species_without_inducing_lces():
    q = [0, 0, 60]
    assert ref.tiles([0, 10, 40], q, 40, 60, 64, 0, 32) == [(0, 0, 0, 64), (1, 0, 0, 64)]
    assert ref.tiles([0, 10, 40], q, 40, 60, 64, 2, 32) == [(0, 0, 0, 64), (1, 0, 0, 64)]
    for kind in (0, 1, 2):       # atoms of that species only: nothing to compute
        assert ref.tiles([0, 40, 40], q, 40, 60, 64, kind, 32) == []


def test_tiles_of_a_species_without_atoms():
    q = [0, 30, 90]
    assert ref.tiles([0, 0, 40], q, 40, 90, 64, 0, 32) == [(0, 0, 0, 64), (0, 1, 0, 64), (1, 0, 0, 64), (1, 1, 0, 64)]
    assert ref.tiles([0, 0, 40], q, 40, 90, 64, 2, 32) == [(0, 0, 0, 64), (0, 1, 0, 96), (1, 0, 0, 64), (1, 1, 0, 96)]


def test_offsets_with_ghosts_and_shards():
    slots = np.array([1, 0, -1, 1, 0, 0, 2, 1, -1])      # sorted: 0 0 0 1 1 1 2 g g
    a, n = ref.offsets(slots, 3)
    assert list(a) == [0, 3, 6, 7] and n == 9
    a, n = ref.offsets(slots, 3, rank=1, world=2)        # sorted positions 1 3 5 7: 0 1 1 g
    assert list(a) == [0, 1, 3, 3] and n == 4
    # the ghost rows share the last species' row tile: its inducing range
    assert ref.tiles([0, 3, 6, 7], [0, 5, 10, 20], 9, 20, 64, 0, 16) == [(0, 0, 0, 64)]
    assert ref.tiles([0, 7, 7, 7], [0, 5, 10, 20], 9, 20, 64, 0, 8)[1] == (1, 0, 0, 64)


def test_tile_height_thresholds():
    """K_nm: half tiles while 5 n32 <= 2 ncu, 64-row tiles from 3 ncu on; W + covloss: 5 n32 <= 3 ncu, 2 n32 >= 11 ncu."""
    ncu = 40
    q = [0, 64]          # one species, one column tile: n32(K_nm) = n32(W) = n32(cov) = row tiles (Dpad = 64)
    def hk(rows):
        return ref.tile_heights([0, 32 * rows], q, 32 * rows, 64, 64, ncu)
    # K_nm: 16 rows up to 16 tiles (5 * 16 = 80 = 2 * 40), 32 from 17, 64 from 120; W + covloss (2 n32): 16 up to 12 tiles
    # (5 * 24 = 120), 64 from 2 * 2 * rows >= 440: rows >= 110
    assert hk(12) == (16, 16) and hk(13) == (16, 32) and hk(16) == (16, 32) and hk(17) == (32, 32)
    assert hk(109) == (32, 32) and hk(110) == (32, 64) and hk(119) == (32, 64) and hk(120) == (64, 64)
    assert ref.tile_heights([0, 32 * 12], q, 32 * 12, 64, 64, ncu, half=False) == (32, 32)


def test_chaining_window():
    """Per XCD (row tile % 8), more than four and at most five W + covloss entries per CU chain the excess."""
    ncu = 16             # two CUs per XCD: window (8, 10] entries per XCD
    q = [0, 64]
    for rows, want in ((32, 0), (40, 8 * 2), (33, 2), (48, 0)):
        # each row tile carries one W and one covloss entry: rows / 8 row tiles per XCD, two entries each
        assert ref.chained([0, 32 * rows], q, 32 * rows, 64, 64, ncu, 32) == want, rows
    assert ref.chained([0, 32 * 40], q, 32 * 40, 64, 64, ncu, 32, chain=False) == 0
    assert ref.chained([0, 32 * 40], q, 32 * 40, 64, 64, ncu, 64) == 0
