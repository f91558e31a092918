"""The host twin and definition of the velocity-correlation accumulator, workloads.VacfRing, and what transport reads off its
table (Vacf, green_kubo, onsager, vibrational_dos), without a GPU.  The reference has no velocity autocorrelation: the twin is
held to a brute-force evaluation of the written definition over the whole stored series, in arithmetic that is exact (small
integer velocities, masses that are powers of two with a total that is one), so that no summation order can hide an error; and
to the closed forms of a harmonic series and of a geometric curve."""
import numpy as np
import pytest

from autoforce_amd.transport import ASE_FS, Vacf, green_kubo, onsager, vibrational_dos
from autoforce_amd.workloads import FS, VACF_CHUNK, VacfRing, observer_velocities

SPECIES = (3, 15, 16, 35)   # the table: 35 is absent from the frame
EPS = np.finfo(float).eps


def _frame():
    """512 atoms, not sorted: 211 of species 3, 300 of 15 (two chunks, the second ragged), one of 16, none of 35; masses 1, 2
    and 4 with the total 1024, so that the centre-of-mass velocity of integer velocities is a dyadic fraction."""
    rng = np.random.default_rng(5)
    numbers = rng.permutation(np.array([3] * 211 + [15] * 300 + [16] * 1))
    masses = rng.permutation(np.array([1.0] * 256 + [2.0] * 128 + [4.0] * 128))
    assert masses.sum() == 1024.0 and VACF_CHUNK < 300 < 2 * VACF_CHUNK
    return numbers, masses


def _series(n, N, seed=1):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, N, 3)).astype(float)


def _brute(vs, every, lags, origin_every, com, masses, numbers, upto):
    """The definition, sample by sample: samples 0 ... upto - 1 of the series vs[configuration] are the current ones."""
    S = len(SPECIES)
    sam = vs[::every]
    members = [np.flatnonzero(numbers == z) for z in SPECIES]
    tr, col, count = np.zeros((lags, S)), np.zeros((lags, S, S)), np.zeros(lags, dtype=np.int64)
    c = [(masses[:, None] * v).sum(axis=0) / masses.sum() if com else np.zeros(3) for v in sam]
    e = [np.array([(v[i] - cc).sum(axis=0) if len(i) else np.zeros(3) for i in members]) for v, cc in zip(sam, c)]
    for s in range(upto):
        for k in range(lags):
            o = s - k
            if o < 0 or o % origin_every:
                continue
            for z, i in enumerate(members):
                if len(i):
                    tr[k, z] += ((sam[s][i] - c[s]) * (sam[o][i] - c[o])).sum() / len(i)
            col[k] += e[s] @ e[o].T
            count[k] += 1
    return tr, col, count


CASES = {   # (every, lags, origin_every, configurations) and the counts
    "lags-over-samples": ((1, 16, 1, 6), [5, 4, 3, 2, 1] + [0] * 11),
    "ring-wraps": ((1, 4, 1, 40), [39, 38, 37, 36]),
    "every3": ((3, 4, 1, 40), [13, 12, 11, 10]),
    "origin3": ((1, 8, 3, 40), [13, 13, 13, 12, 12, 12, 11, 11]),
}


@pytest.mark.parametrize("com", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_the_twin_is_the_definition_in_exact_arithmetic(case, com):
    (every, lags, oe, nconf), counts = CASES[case]
    numbers, masses = _frame()
    vs = _series(nconf, len(numbers))
    tw = VacfRing(every, lags, oe, com, masses, numbers, SPECIES)
    for v in vs:
        tw.add(v)
    tab = tw.table()
    nsam = -(-nconf // every)
    tr, col, count = _brute(vs, every, lags, oe, com, masses, numbers, nsam - 1)
    assert list(tab["count"]) == counts and list(count) == counts
    assert np.array_equal(tab["tracer"], tr) and np.array_equal(tab["collective"], col)
    assert list(tab["n"]) == [211, 300, 1, 0] and list(tab["species"]) == list(SPECIES)
    assert list(tab["lags"]) == [every * k for k in range(lags)]
    assert np.all(tab["tracer"][:, 3] == 0.0) and np.all(tab["collective"][:, 3] == 0.0) and np.all(tab["collective"][:, :, 3] == 0.0)
    assert tab["samples"] == nsam - 1 and tab["pending"] == 1 and tab["next_due"] == nsam * every
    if counts[-1] > 0:   # (the block is not symmetric at a lag > 0, and it is the one of the definition, not its transpose)
        assert not np.array_equal(col[-1], col[-1].T)
    # the tracer correlation of the one-atom species is the product of its own velocities, less the centre of mass
    if not com:
        i = int(np.flatnonzero(numbers == 16)[0])
        sam = vs[::every]
        want = sum(float(sam[s][i] @ sam[s - 1][i]) for s in range(1, nsam - 1) if (s - 1) % oe == 0) if lags > 1 else 0.0
        assert tab["tracer"][1, 2] == want


def test_the_last_sample_is_pending_until_the_next_arrives():
    numbers, masses = _frame()
    vs = _series(12, len(numbers), seed=2)
    tw = VacfRing(1, 5, 2, True, masses, numbers, SPECIES)
    empty = tw.table()
    assert empty["samples"] == 0 and empty["pending"] == 0 and empty["next_due"] == 0 and not empty["count"].any()
    for m, v in enumerate(vs, start=1):
        tw.add(v)
        tab = tw.table()
        assert tab["samples"] == m - 1 and tab["pending"] == 1 and tab["next_due"] == m
        tr, col, count = _brute(vs, 1, 5, 2, True, masses, numbers, m - 1)   # (one more sample adds what the definition says of sample m - 2)
        assert np.array_equal(tab["tracer"], tr) and np.array_equal(tab["collective"], col) and np.array_equal(tab["count"], count)
    # configurations between two samples change nothing
    tw3 = VacfRing(3, 5, 1, False, masses, numbers, SPECIES)
    for v in vs[:4]:
        tw3.add(v)
    before = tw3.table()
    tw3.add(vs[4]); tw3.add(vs[5])
    after = tw3.table()
    assert before["samples"] == after["samples"] == 1 and after["next_due"] == 6
    assert np.array_equal(before["tracer"], after["tracer"]) and np.array_equal(before["collective"], after["collective"])


def test_a_harmonic_series_gives_the_cosine_and_its_frequency():
    """v_ic(n) = a_ic cos(w n dt + phi_ic) with w dt = 2 pi P / M over M samples: P whole periods.  The product of sample s and
    origin s - k is a_ic^2 / 2 (cos(w k dt) + cos(w (2 s - k) dt + 2 phi_ic)).  The windows s >= k of a lag are not whole periods,
    so the second term is removed atom by atom instead: the components come in pairs of equal amplitude with phases phi and
    phi + pi / 2, whose second terms cancel at every s.  Then tr[k] / count[k] = (sum a^2 / 2 n_z) cos(w k dt) to rounding.
    Tolerance on that mean: the arguments are reduced to [0, 2 pi + phi) exactly (integer (P n) mod M), so a velocity carries a
    few eps of relative error and a product of two about 4 eps; the block sum of a chunk adds at most 10 levels of eps / 2; the
    M sequential additions into tr[k] add M eps / 2 of a partial sum that is at most M sum a^2 / (2 n_z), which the division by
    count ~ M brings to M eps / 4 of sum a^2 / n_z.  Together (16 + M / 4) eps sum a^2 / n_z, within 4 M eps sum a^2 / n_z."""
    M, P, L = 128, 8, 64
    rng = np.random.default_rng(4)
    numbers = np.array([3] * 70 + [15] * 300 + [16] * 2)
    N = len(numbers)
    masses = np.ones(N)
    amp = rng.uniform(0.5, 1.5, size=(N // 2, 3))
    phi = rng.uniform(0.0, 2.0 * np.pi, size=(N // 2, 3))
    amp, phi = np.repeat(amp, 2, axis=0), np.repeat(phi, 2, axis=0)
    phi[1::2] += 0.5 * np.pi   # (consecutive atoms are of one species: 70, 300 and 2 are even)
    tw = VacfRing(1, L, 1, False, masses, numbers, SPECIES)
    for n in range(M + 1):     # (the last one is fed to make sample M - 1 count)
        tw.add(amp * np.cos(2.0 * np.pi * ((P * n) % M) / M + phi))
    tab = tw.table()
    assert tab["samples"] == M and list(tab["count"]) == [M - k for k in range(L)]
    k = np.arange(L)
    for q, z in enumerate(SPECIES[:3]):
        a2, nz = float((amp[numbers == z] ** 2).sum()), int(np.sum(numbers == z))
        mean = tab["tracer"][:, q] / tab["count"]
        want = a2 / (2.0 * nz) * np.cos(2.0 * np.pi * P * k / M)
        err = np.abs(mean - want).max()
        print(f"species {z}: max |mean - closed form| = {err:.3e}, bound {4 * M * EPS * a2 / nz:.3e}")
        assert err <= 4 * M * EPS * a2 / nz
    holder = Vacf(1, L).add(tab)
    f, dos = vibrational_dos(holder, 1.0)
    assert set(dos) == {3, 15, 16}
    for z, g in dos.items():
        assert int(np.argmax(g)) == 2 * L * P // M, (z, int(np.argmax(g)))   # f_j = j / (2 L dt): w / 2 pi = P / (M dt) is bin 2 L P / M
    assert f[2 * L * P // M] == pytest.approx(1e3 * P / M)                # THz at dt = 1 fs


def test_green_kubo_and_onsager_integrate_a_geometric_curve_to_its_closed_form():
    """C(k) = C0 q^k: the trapezoid sum up to lag K is step C0 (1 + q) / 2 (1 - q^K) / (1 - q).  K additions of terms below 2 C0:
    within 4 K eps of the limit."""
    L, q, dt_fs, every = 40, 0.75, 2.0, 3
    C0 = np.array([2.0, 0.5, 0.0])
    n = np.array([4, 12, 0])
    k = np.arange(L)
    count = np.full(L, 7, dtype=np.int64)
    curve = C0[None] * q ** k[:, None]
    block = np.array([[1.0, -0.25, 0.0], [0.5, 2.0, 0.0], [0.0, 0.0, 0.0]])
    tab = dict(tracer=7 * curve, collective=7 * block[None] * q ** k[:, None, None], count=count, lags=every * k, species=np.array([3, 15, 16]), n=n, samples=50)
    holder = Vacf(every, L).add(tab).add(tab)   # (two runs add up: the means stay)
    assert holder.samples == 100 and np.array_equal(holder.count, 2 * count)
    step = every * dt_fs * FS ** 2
    assert ASE_FS == FS
    closed = step * 0.5 * (1.0 + q) * (1.0 - q ** k) / (1.0 - q)
    D = green_kubo(holder, dt_fs, at_fs=every * dt_fs * 10)
    assert set(D) == {3, 15}
    for z, c0 in ((3, 2.0), (15, 0.5)):
        assert np.array_equal(D[z]["t"], every * dt_fs * k)
        assert np.abs(D[z]["D"] - c0 * closed / 3.0).max() <= 4 * L * EPS * c0 * closed[-1] / 3.0
        assert D[z]["value"] == D[z]["D"][10]
    assert green_kubo(holder, dt_fs)[3]["value"] == D[3]["D"][-1]
    t, Lab = onsager(holder, dt_fs)
    assert np.array_equal(t, every * dt_fs * k) and Lab.shape == (L, 3, 3)
    want = block[None] * closed[:, None, None] / (3.0 * 16)
    assert np.abs(Lab - want).max() <= 4 * L * EPS * 2.0 * closed[-1] / (3.0 * 16)
    assert Lab[-1, 0, 1] < 0.0 < Lab[-1, 1, 0]   # (the block keeps its order)


def test_observer_velocities_is_the_formula_element_by_element():
    rng = np.random.default_rng(8)
    N, hdt = 7, 0.5 * 1.0 * FS
    v, F, m = rng.normal(size=(N, 3)), rng.normal(size=(N, 3)), rng.uniform(1.0, 40.0, size=N)
    fixed = rng.random(size=(N, 3)) < 0.3
    assert fixed.any() and not fixed.all()
    got = observer_velocities(v, F, m, hdt, 1, fixed)
    got0 = observer_velocities(v, F, m, hdt, 0, fixed)
    free = observer_velocities(v, F, m, hdt, 1)
    for i in range(N):
        for k in range(3):
            kicked = float(v[i, k]) + hdt * float(F[i, k]) / float(m[i])
            assert free[i, k] == kicked
            assert got[i, k] == (0.0 if fixed[i, k] else kicked)
            assert got0[i, k] == (0.0 if fixed[i, k] else v[i, k])
    assert got is not v and np.array_equal(observer_velocities(v, F, m, hdt, 0), v)
