"""workloads.SqRing — the host twin and definition of the structure-factor accumulator of the device MD loop (md_sq.inc) — against
things that are not the twin: a direct np.exp(1j * positions @ q.T) correlated with plain loops over the whole history, a simple
cubic lattice whose densities are known, lattice translations and wrapping, the sign flip of the wave vectors, a trajectory whose
S x S block is asymmetric by construction, and the bookkeeping of every, origin_every and a ring shorter than the run.  Everything
is held to the a-priori bound of the issue, restated here (not read from workloads.sq_bounds, which is checked against it):
    |d rho_z(q)| <= B_z = 128 hmax (1 + smax) n_z 2^-52,   |d f[k, j, a, b]| <= count[k] (n_a B_b + n_b B_a + count[k] n_a n_b 2^-52).
And transport.q_vectors against a brute-force enumeration, and the readers on synthetic tables."""
import numpy as np
import pytest

import accumulator_refs
from autoforce_amd import transport
from autoforce_amd.workloads import SqRing, sq_bounds, sq_vectors

CELL = np.array([[9.1, 0.0, 0.0], [1.3, 8.2, 0.0], [-0.7, 2.1, 10.4]])
SPECIES = [3, 15, 16]   # the table; 16 has no atom in NUMBERS
NUMBERS = np.array([3] * 37 + [15] * 19)
PBC = (True, True, True)


def _bounds(hmax, smax, nz, count):
    n, c = np.asarray(nz, float), np.asarray(count, float)
    B = 128.0 * hmax * (1.0 + smax) * n * 2.0 ** -52
    F = np.zeros((len(c), len(n), len(n)))
    for k in range(len(c)):
        for a in range(len(n)):
            for b in range(len(n)):
                F[k, a, b] = c[k] * (n[a] * B[b] + n[b] * B[a] + c[k] * n[a] * n[b] * 2.0 ** -52)
    return B, F


def _smax(frames, cell=CELL):
    return float(np.abs(np.asarray(frames) @ np.linalg.inv(cell)).max())


def _frames(count=23, seed=5, spread=4.0):
    """A random walk of unwrapped positions that reaches scaled coordinates of about `spread`."""
    rng = np.random.default_rng(seed)
    s0 = rng.uniform(-spread, spread, size=(len(NUMBERS), 3))
    steps = rng.normal(scale=0.02, size=(count, len(NUMBERS), 3)).cumsum(axis=0)
    return (s0[None] + steps) @ CELL


def _hkl(seed=2, nq=41, hmax=16):
    rng = np.random.default_rng(seed)
    hkl = rng.integers(-hmax, hmax + 1, size=(nq, 3))
    hkl[0] = (hmax, 0, 0); hkl[1] = (0, -hmax, 0); hkl[2] = (0, 0, hmax); hkl[3] = (-1, 2, 0); hkl[4] = (0, 1, -3); hkl[5] = (-5, 0, 7)
    assert not np.any(np.all(hkl == 0, axis=1))
    return hkl


def _direct(frames, hkl, every, lags, origin_every, numbers=NUMBERS, species=SPECIES, cell=CELL):
    """The definition with nothing shared with the twin (accumulator_refs.sq: exp(1j x . q) per atom, summed per species in
    extended precision, every density of the run kept, the correlations by plain loops over (sample, lag))."""
    return accumulator_refs.sq(frames, hkl, every, lags, origin_every, numbers, species, cell)


def _twin(frames, hkl, every=1, lags=1, origin_every=1, numbers=NUMBERS, species=SPECIES, cell=CELL):
    tw = SqRing(every, hkl, lags, origin_every, numbers, species, cell, PBC)
    for x in frames:
        tw.add(x)
    return tw, tw.table()


def _within(tab, want, hmax, smax, what):
    B, F = _bounds(hmax, smax, tab["n"], want["count"])
    assert np.array_equal(tab["count"], want["count"]) and tab["samples"] == want["samples"], (what, tab["count"], want["count"])
    df = np.abs(tab["f"] - want["f"]).max(axis=1)           # [lags, S, S]
    dm = np.abs(tab["mean"] - want["mean"]).max(axis=0)     # [S]
    live = F > 0
    print(f"{what}: max |df| / bound {np.max(df[live] / F[live]) if live.any() else 0.0:.3g}, max |dmean| / (samples B) "
          f"{np.max(dm[B > 0] / (want['samples'] * B[B > 0])):.3g}")
    assert np.all(df <= F), (what, df, F)
    assert np.all(dm <= want["samples"] * B), (what, dm, want["samples"] * B)


def test_the_twin_equals_direct_numpy_within_the_bound():
    frames, hkl = _frames(), _hkl()
    tw, tab = _twin(frames, hkl, lags=6)
    want = _direct(frames, hkl, 1, 6, 1)
    smax = _smax(frames)
    assert 3.0 < smax < 6.0 and tw.smax == pytest.approx(smax, rel=1e-12) and np.abs(hkl).max() == 16
    assert np.array_equal(tab["n"], [37, 19, 0]) and list(tab["count"]) == [23, 22, 21, 20, 19, 18]
    assert np.abs(tab["f"][:, :, :2, :2]).min() > 1e-6    # (no entry is zero by accident: the comparison means something)
    _within(tab, want, 16, smax, "direct numpy")
    B, F = sq_bounds(16, smax, tab["n"], tab["count"])
    B0, F0 = _bounds(16, smax, tab["n"], tab["count"])
    assert np.allclose(B, B0, rtol=1e-14, atol=0) and np.allclose(F, F0, rtol=1e-14, atol=0)
    assert np.allclose(tab["q"], sq_vectors(hkl, CELL)) and np.allclose(tab["q"] @ CELL.T, 2.0 * np.pi * hkl, atol=1e-12)


def test_an_index_of_32_stays_within_the_bound():
    frames, hkl = _frames(count=4, seed=8), _hkl(seed=4, nq=17, hmax=32)
    _, tab = _twin(frames, hkl, lags=2)
    _within(tab, _direct(frames, hkl, 1, 2, 1), 32, _smax(frames), "hmax 32")


@pytest.mark.parametrize("m", [3, 4])
def test_a_simple_cubic_lattice_scatters_at_its_own_reciprocal_lattice_only(m):
    """m^3 atoms on a lattice in the (sheared) cell: rho = N where all three indices are multiples of m, 0 elsewhere."""
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    x = (g / m) @ CELL
    numbers = np.full(len(x), 3)
    top = 2 * m
    hkl = np.stack(np.meshgrid(*[np.arange(-top, top + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    hkl = hkl[np.any(hkl != 0, axis=1)][::5]
    tw = SqRing(1, hkl, 1, 1, numbers, [3], CELL, PBC)
    rho = tw.density(x)[:, 0]
    B, _ = _bounds(np.abs(hkl).max(), _smax(x), [len(x)], [1])
    bragg = np.all(hkl % m == 0, axis=1)
    assert bragg.sum() >= 5 and (~bragg).sum() > 100
    print(f"lattice m = {m}: max |rho - N| {np.abs(rho[bragg] - len(x)).max():.3g}, off the lattice {np.abs(rho[~bragg]).max():.3g}, B {B[0]:.3g}")
    assert np.all(np.abs(rho[bragg] - len(x)) <= B[0])
    assert np.all(np.abs(rho[~bragg]) <= B[0])


def test_lattice_translations_and_wrapping_leave_the_table():
    frames, hkl = _frames(count=9, spread=0.9), _hkl(nq=23)
    _, tab = _twin(frames, hkl, lags=3)
    shift = np.random.default_rng(1).integers(-3, 4, size=(len(frames),) + frames.shape[1:])   # (per frame and atom: any image will do)
    moved = frames + shift @ CELL
    s = frames @ np.linalg.inv(CELL)
    wrapped = (s - np.floor(s)) @ CELL
    smax = max(_smax(frames), _smax(moved), _smax(wrapped))
    assert _smax(moved) > 2.5 and _smax(wrapped) <= 1.0 + 1e-12
    for what, other in (("translated", moved), ("wrapped", wrapped)):
        _, tab2 = _twin(other, hkl, lags=3)
        _within(tab2, tab, 16, smax, what)


def test_the_sign_flip_of_the_wave_vectors_leaves_f():
    frames, hkl = _frames(count=7), _hkl(nq=19)
    _, tab = _twin(frames, hkl, lags=4, origin_every=2)
    _, flip = _twin(frames, -hkl, lags=4, origin_every=2)
    assert np.array_equal(flip["f"], tab["f"])                    # (every operation commutes with the conjugation, bit for bit)
    assert np.array_equal(flip["mean"], np.conj(tab["mean"]))
    assert np.abs(tab["mean"].imag).max() > 1e-3


def test_the_block_is_asymmetric_at_positive_lags_where_the_trajectory_makes_it_so():
    """Species a drifts by d per configuration, species b stands still: rho_a(s) = exp(i q.d s) rho_a(0), so f[k][a][b] sums
    Re(exp(i q.d s) z) and f[k][b][a] sums Re(exp(i q.d (s - k)) z), z = rho_a(0) conj rho_b(0): equal at k = 0 only."""
    rng = np.random.default_rng(12)
    x0 = rng.uniform(0.0, 1.0, size=(len(NUMBERS), 3)) @ CELL
    d = np.array([0.013, 0.0, 0.0]) @ CELL   # (scaled drift along the first axis)
    count, lags = 12, 4
    frames = np.array([x0 + s * d * (NUMBERS == 3)[:, None] for s in range(count)])
    hkl = np.array([[5, 0, 0], [3, 1, -2], [0, 2, 1]])   # (the last does not see the drift)
    _, tab = _twin(frames, hkl, lags=lags)
    rho0 = _direct(frames[:1], hkl, 1, 1, 1)["rho"][0]
    z = rho0[:, 0] * np.conj(rho0[:, 1])
    phase = 2.0 * np.pi * hkl[:, 0] * 0.013
    _, F = _bounds(5, _smax(frames), tab["n"], tab["count"])
    for k in range(lags):
        ab = sum((np.exp(1j * phase * s) * z).real for s in range(k, count))
        ba = sum((np.exp(1j * phase * (s - k)) * z).real for s in range(k, count))
        assert np.all(np.abs(tab["f"][k, :, 0, 1] - ab) <= F[k, 0, 1]) and np.all(np.abs(tab["f"][k, :, 1, 0] - ba) <= F[k, 1, 0])
        gap = np.abs(tab["f"][k, :, 0, 1] - tab["f"][k, :, 1, 0])
        if k == 0:
            assert np.all(gap <= F[0, 0, 1])
        else:
            assert np.all(gap[:2] > 1e3 * F[k, 0, 1]) and gap[2] <= 2 * F[k, 0, 1], (k, gap, F[k, 0, 1])


@pytest.mark.parametrize("every,lags,origin_every", [(1, 5, 1), (2, 5, 3), (3, 4, 2), (1, 64, 1), (1, 1, 1), (1, 13, 3)])
def test_counts_ring_slots_and_an_absent_species(every, lags, origin_every):
    frames, hkl = _frames(count=40, seed=3), _hkl(nq=7)
    tw, tab = _twin(frames, hkl, every=every, lags=lags, origin_every=origin_every)
    samples = -(-40 // every)
    pairs = [sum(1 for s in range(samples) if s - k >= 0 and (s - k) % origin_every == 0) for k in range(lags)]
    assert list(tab["count"]) == pairs and tab["samples"] == samples and tab["next_due"] == samples * every
    assert list(tab["lags"]) == [every * k for k in range(lags)]
    assert tw.ring.shape[0] == lags   # (slots are reused wherever the run is longer than the lags)
    _within(tab, _direct(frames, hkl, every, lags, origin_every), 16, _smax(frames), f"every {every} lags {lags} origin_every {origin_every}")
    assert np.all(tab["f"][:, :, 2, :] == 0.0) and np.all(tab["f"][:, :, :, 2] == 0.0) and np.all(tab["mean"][:, 2] == 0.0)
    assert np.all(tab["f"][tab["count"] == 0] == 0.0)


def test_bad_settings_are_refused():
    hkl = _hkl(nq=7)
    for bad in (dict(every=0), dict(lags=0), dict(origin_every=0), dict(lags=8193)):
        kw = dict(every=1, lags=1, origin_every=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            SqRing(kw["every"], hkl, kw["lags"], kw["origin_every"], NUMBERS, SPECIES, CELL, PBC)
    for rows in ([[0, 0, 0]], [[33, 0, 0]], [[1, 0, 0]] * 8193, [[0.5, 1, 0]]):
        with pytest.raises(ValueError):
            SqRing(1, np.array(rows), 1, 1, NUMBERS, SPECIES, CELL, PBC)
    with pytest.raises(ValueError):
        SqRing(1, np.array([[1, 0, 2]]), 1, 1, NUMBERS, SPECIES, CELL, (True, True, False))
    SqRing(1, np.array([[1, -2, 0]]), 1, 1, NUMBERS, SPECIES, CELL, (True, True, False))


@pytest.mark.parametrize("qmax", [1.1, 2.4, 3.3])
def test_q_vectors_against_brute_force(qmax):
    hkl = transport.q_vectors(CELL, qmax)
    rec = 2.0 * np.pi * np.linalg.inv(CELL).T
    top = 12
    every = np.stack(np.meshgrid(*[np.arange(-top, top + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    qn = np.linalg.norm(every @ rec, axis=1)
    inside = every[(qn > 0) & (qn <= qmax)]
    assert np.abs(inside).max() < top                                  # (the brute-force box holds the sphere)
    assert len(inside) % 2 == 0 and len(hkl) == len(inside) // 2       # the count: one of each +- pair
    got = {tuple(v) for v in hkl.tolist()}
    assert len(got) == len(hkl) and got <= {tuple(v) for v in inside.tolist()}
    assert not any(tuple(-np.array(v)) in got for v in got)            # no pair twice
    for v in hkl:                                                      # the kept one: first non-zero index positive
        assert v[np.flatnonzero(v)[0]] > 0
    q = np.linalg.norm(hkl @ rec, axis=1)
    keys = [(float(a),) + tuple(v) for a, v in zip(q, hkl.tolist())]
    assert keys == sorted(keys)                                        # ordered by |q|, then by the triple
    with pytest.raises(ValueError):
        transport.q_vectors(CELL, qmax, limit=len(hkl) - 1)
    assert len(transport.q_vectors(CELL, qmax, limit=len(hkl))) == len(hkl)


def _synthetic(lags=8, count0=50, tau=3.0):
    """A table whose answers are known: S_ab = delta_ab on every vector, decaying as exp(-k / tau); a Bragg peak of weight 1 on
    the first vector of species 0."""
    cell = np.diag([10.0, 10.0, 10.0])
    hkl = transport.q_vectors(cell, 1.3)
    n = np.array([40, 10, 0])
    count = np.array([count0 - k for k in range(lags)])
    f = np.zeros((lags, len(hkl), 3, 3))
    for k in range(lags):
        for a in range(2):
            f[k, :, a, a] = count[k] * n[a] * np.exp(-k / tau)
    mean = np.zeros((len(hkl), 3), dtype=complex)
    mean[0, 0] = count0 * np.sqrt(n[0]) * np.exp(0.3j)
    return dict(f=f, mean=mean, count=count, lags=2 * np.arange(lags), hkl=hkl, q=sq_vectors(hkl, cell), species=np.array([3, 15, 16]), n=n,
                origin_every=1, samples=count0, next_due=2 * count0)


def test_the_readers_on_a_synthetic_table():
    t = _synthetic()
    q, S = transport.structure_factor(t)
    lengths = np.unique(np.round(np.linalg.norm(t["q"], axis=1), 9))
    assert np.allclose(q, lengths) and S.shape == (len(q), 3, 3)
    assert np.allclose(S[:, :2, :2], np.eye(2)[None]) and np.all(np.isnan(S[:, 2, :])) and np.all(np.isnan(S[:, :, 2]))
    q2, S2 = transport.structure_factor(t, dq=0.5)
    assert len(q2) < len(q) and np.all(np.diff(q2) > 0) and np.allclose(S2[:, 0, 0], 1.0)
    _, tot = transport.structure_factor(t, weights={3: -1.9, 15: 5.1})
    assert np.allclose(tot, 1.0)
    _, Sd = transport.structure_factor(t, diffuse=True)
    shell0 = int(np.sum(np.round(np.linalg.norm(t["q"], axis=1), 9) == lengths[0]))
    assert np.isclose(Sd[0, 0, 0], 1.0 - 1.0 / shell0) and np.allclose(Sd[1:, 0, 0], 1.0) and np.allclose(Sd[:, 1, 1], 1.0)
    qs, lag, F, Fn = transport.intermediate_scattering(t)
    assert list(lag) == list(t["lags"]) and np.allclose(Fn[:, :, 0, 0], np.exp(-np.arange(8) / 3.0)[:, None]) and np.allclose(F[0], S, equal_nan=True)
    holder = transport.Sq(2, t["hkl"], lags=8)
    holder.add(t).add(t)
    assert holder.samples == 100 and np.array_equal(holder.count, 2 * t["count"]) and np.allclose(transport.structure_factor(holder)[1], S, equal_nan=True)
    assert holder.settings()[0] == 2 and holder.md == "md_sq" and holder.twin_of == "SqRing" and holder.constant_cell
    with pytest.raises(ValueError):
        transport.Sq(2, t["hkl"][:-1], lags=8).add(t)
    with pytest.raises(ValueError):
        transport.Sq(1, t["hkl"], lags=8).add(t)
    with pytest.raises(ValueError, match="origin_every"):
        transport.Sq(2, t["hkl"], lags=8, origin_every=3).add(t)
    for reader in (transport.Sq(2, t["hkl"], lags=8).table, lambda: transport.structure_factor(transport.Sq(2, t["hkl"], lags=8))):
        with pytest.raises(ValueError, match="no table"):   # (an empty holder says so)
            reader()


def test_the_dynamic_structure_factor_finds_an_oscillation():
    lags, dt_fs, every = 64, 2.0, 2
    t = _synthetic(lags=lags, count0=200)
    f0 = 1e3 * 8 / (2.0 * lags * every * dt_fs)   # bin 8 of the transform's axis, THz
    k = np.arange(lags)
    for j in range(lags):
        t["f"][j, :, 0, 0] = t["count"][j] * t["n"][0] * np.cos(2.0 * np.pi * f0 * 1e-3 * k[j] * every * dt_fs)
    f, q, S = transport.dynamic_structure_factor(t, dt_fs)
    assert f.shape == (lags,) and S.shape == (lags, len(q), 3, 3) and np.isclose(f[8], f0)
    assert np.all(np.argmax(S[:, :, 0, 0], axis=0) == 8)
    f1, _, S1 = transport.dynamic_structure_factor(t, dt_fs, window=None)
    assert np.all(np.argmax(S1[:, :, 0, 0], axis=0) == 8) and S1[8, 0, 0, 0] > S[8, 0, 0, 0]
    with pytest.raises(ValueError):
        transport.dynamic_structure_factor(t, dt_fs, window="blackman")
