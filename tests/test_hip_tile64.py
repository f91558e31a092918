"""GPU tests of the 64-neighbour tiles of the step kernels (nl_fwd_kernel, desc_rev_kernel: descriptor.hip, WaveLds::CHS).
A list of up to 64 neighbours is one tile (lane = neighbour), longer lists take further tiles of 64 and read the list back
from memory; the boundaries that matter are 48 (the rows whose virial / own-force sums are added first), 64 (one tile or
two) and 96 (where the forward kernel's hit buffers used to end).

(a) a density-graded frame whose list lengths straddle all of them, every output against the CPU oracle at the
    tolerances of test_hip_parity.py, the same frame through the sharded (scatter) form of the reverse kernel and
    through its training-rows form;
(b) the device Langevin loop on a compressed frame with lists of 49 - 64 against the host loop, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RC, ETA, SPECIES, M = 6.0, 4.0, [3, 15, 16], 48


def graded_frame(seed=0):
    """550 atoms, three species: 25 layers of 5 x 5 sites (2.5 A) along x whose spacing falls from 3.3 A (five layers) to
    1.45 A (nine layers) and back, rattled by 0.1 A — 39 to 110 neighbours inside 6 A."""
    rng = np.random.default_rng(seed)
    sp = np.concatenate([np.full(5, 3.3), np.linspace(3.3, 1.45, 6)[1:-1], np.full(9, 1.45), np.linspace(1.45, 3.3, 6)[1:-1]])
    x = np.concatenate([[0.0], np.cumsum(sp)[:-1]])
    a, n = 2.5, 5
    g = np.array([(xx, j * a, k * a) for xx in x for j in range(n) for k in range(n)], float)
    pos = g + 0.1 * rng.normal(size=g.shape)
    N = len(pos)
    numbers = rng.permutation(np.array([3] * (3 * N // 8) + [15] * (N // 8) + [16] * (N - 3 * N // 8 - N // 8))).astype(np.int32)
    return numbers, pos, np.diag([sp.sum(), n * a, n * a]), [True] * 3


def inducing(numbers, pos, cell, m, seed):
    from oracle import oracle as orc
    from autoforce_amd import Local
    rng = np.random.default_rng(seed)
    ptr, j, off = orc.neighbors(pos, cell, [True] * 3, RC)
    X = []
    for a in rng.choice(len(numbers), size=m, replace=False):
        s = slice(ptr[a], ptr[a + 1])
        r = pos[j[s]] - pos[a] + off[s].astype(float) @ cell
        r = r + 0.05 * rng.normal(size=r.shape)
        keep = np.linalg.norm(r, axis=1) < RC - 1e-3
        X.append(Local(int(numbers[a]), numbers[j[s]][keep], r[keep]))
    return X


@pytest.fixture(scope="module")
def graded():
    """The frame, the model on the device and the oracle's results for it: computed once, read by the three tests."""
    from oracle import oracle as orc
    from autoforce_amd import SGPRModel
    numbers, pos, cell, pbc = graded_frame(0)
    _, pos2, _, _ = graded_frame(1)
    X = inducing(numbers, pos2, cell, M, seed=5)
    mu = np.random.default_rng(6).normal(size=M)
    mdl = SGPRModel(3, 3, ETA, RC, species=SPECIES)
    mdl.set_inducing(X)
    ind_z = np.array([x.number for x in X], np.int32)
    ind_ptr = np.concatenate([[0], np.cumsum([len(x._b) for x in X])])
    Pm, nnm = orc.inducing_descriptors(3, 3, RC, SPECIES, ind_z, ind_ptr, np.concatenate([x._b for x in X]),
                                       np.concatenate([x._r for x in X]))
    L, _ = orc.jitcholesky(orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, ETA))
    choli = orc.tril_inverse(L)
    mdl.set_weights(mu, choli=choli)
    nl = orc.neighbors(pos, cell, pbc, RC)
    ref = orc.frame(3, 3, RC, ETA, SPECIES, numbers, pos, cell, nl, ind_z, nnm, Pm, mu, choli=choli)
    yield dict(mdl=mdl, frame=(numbers, pos, cell, pbc), nl=nl, ref=ref, ind=(ind_z, nnm, Pm), mu=mu)
    mdl.close()


def pair_set(ptr, j, off):
    i = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return set(map(tuple, np.column_stack([i, j, off]).tolist()))


def test_lists_across_the_tile_boundaries_against_the_oracle(graded):
    mdl, (numbers, pos, cell, pbc), ref = graded["mdl"], graded["frame"], graded["ref"]
    N = len(numbers)
    out = mdl.predict(numbers, pos, cell, pbc, cov=True)
    ptr, j, off = mdl.neighbors(N)
    nn = np.diff(ptr)
    # the frame does straddle the boundaries — by the list the library itself built
    assert (nn <= 48).any() and ((nn >= 49) & (nn <= 63)).any() and (nn == 64).any() and ((nn >= 65) & (nn <= 96)).any() and (nn > 96).any(), \
        np.bincount(nn)
    assert pair_set(ptr, j, off) == pair_set(*graded["nl"])
    np.testing.assert_allclose(mdl.descriptors(N), ref["p"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(out["cov"], ref["cov"], rtol=1e-10, atol=1e-13)
    assert abs(out["energy"] - ref["energy"]) <= 1e-10 * max(1.0, abs(ref["energy"]))
    assert np.abs(out["forces"] - ref["forces"]).max() <= 1e-8 * np.abs(ref["forces"]).max()
    assert np.abs(out["stress"] - ref["stress"]).max() <= 1e-8 * np.abs(ref["stress"]).max()
    np.testing.assert_allclose(out["beta"], ref["beta"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(out["beta"] ** 2, ref["beta"] ** 2, rtol=1e-9, atol=1e-11)  # (see test_hip_parity.test_golden_frames)
    assert np.abs(out["forces"].sum(0)).max() <= 1e-10 * np.abs(out["forces"]).max()


def test_sharded_scatter_form_on_the_same_frame(graded):
    """World 2: every rank's reverse pass scatters with atomics (no reverse index); the partial sums equal the whole,
    compared as test_hip_parity.test_sharded_partials_sum_to_the_whole compares."""
    mdl, (numbers, pos, cell, pbc) = graded["mdl"], graded["frame"]
    whole = mdl.predict(numbers, pos, cell, pbc, cov=True)
    acc = None
    for r in range(2):
        part = mdl.predict(numbers, pos, cell, pbc, rank=r, world=2, cov=True)
        acc = {k: np.array(v, dtype=float) for k, v in part.items()} if acc is None else {k: acc[k] + part[k] for k in acc}
    assert abs(acc["energy"] - whole["energy"]) <= 1e-12 * max(1.0, abs(whole["energy"]))
    for k in ("forces", "stress", "beta", "cov"):
        np.testing.assert_allclose(acc[k], whole[k], rtol=0, atol=1e-12 * max(1.0, np.abs(whole[k]).max()))
    # ... and the whole is the oracle's (the previous test checked it before the sharded calls re-bound the frame)
    ref = graded["ref"]
    assert np.abs(whole["forces"] - ref["forces"]).max() <= 1e-8 * np.abs(ref["forces"]).max()


def test_training_rows_form_on_the_same_frame(graded):
    """kernel_rows on a frame whose longest list is above 64 runs the ROWS form of desc_rev_kernel (one column per wave;
    the sixteen-column kernel takes lists up to 64 only): its fourth row block and its second virial addition.  One column
    per species against the oracle (the frame evaluated with a unit weight vector: oracle.kernel_rows does the same for
    every column), at the tolerances of test_hip_rows.py; all columns against the predict pass."""
    from oracle import oracle as orc
    mdl, (numbers, pos, cell, pbc), nl = graded["mdl"], graded["frame"], graded["nl"]
    ind_z, nnm, Pm = graded["ind"]
    assert np.diff(nl[0]).max() > 64
    Ke, Kf, Kv = mdl.kernel_rows(numbers, pos, cell, pbc)
    vol = abs(np.linalg.det(cell))
    for z in SPECIES:
        q = int(np.flatnonzero(ind_z == z)[0])
        e = np.zeros(M)
        e[q] = 1.0
        o = orc.frame(3, 3, RC, ETA, SPECIES, numbers, pos, cell, nl, ind_z, nnm, Pm, e, want_p=False)
        assert abs(Ke[q] - o["energy"]) <= 1e-11 * abs(o["energy"]) + 1e-13
        assert np.abs(Kf[:, q] - o["forces"].reshape(-1)).max() <= 1e-9 * np.abs(o["forces"]).max()
        assert np.abs(Kv[:, q] - o["stress"] * vol).max() <= 1e-9 * np.abs(o["stress"] * vol).max()
    mu = graded["mu"]
    out = mdl.predict(numbers, pos, cell, pbc, beta=False)
    assert abs(Ke @ mu - out["energy"]) <= 1e-10 * max(1.0, abs(out["energy"]))
    assert np.abs((Kf @ mu).reshape(-1, 3) - out["forces"]).max() <= 1e-9 * np.abs(out["forces"]).max()
    assert np.abs(Kv @ mu / vol - out["stress"]).max() <= 1e-9 * np.abs(out["stress"]).max()


class _PredictCalc:
    """The library behind the three ASE getters (as in test_hip_md.py)."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, mdl):
        self.mdl, self.betas, self.nn = mdl, [], []
        self._key, self.results = None, {}

    def get_property(self, name, atoms=None):
        key = atoms.positions.tobytes()
        if key != self._key:
            out = self.mdl.predict(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc)
            self.results = dict(energy=out["energy"], forces=out["forces"], stress=out["stress"], free_energy=out["energy"])
            self.betas.append(float(out["beta"].max()))
            self.nn.append(np.diff(self.mdl.neighbors(len(atoms.numbers))[0]))
            self._key = key
        return self.results[name]


def test_device_langevin_with_lists_of_49_to_64_bit_for_bit():
    """The LiPS lattice compressed to 0.94 of its spacing: every list has 49 - 61 neighbours at the start — one tile of
    64 where there were two of 48.  Thirty steps of the device loop against the host loop around the same library."""
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, langevin_nvt, langevin_nvt_device, lips
    f = 0.94
    numbers, pos, cell, pbc = lips(8, seed=0)
    pos, cell = pos * f, cell * f
    mdl = SGPRModel(3, 3, 4, RC, species=sorted(set(int(z) for z in numbers)))
    n2, p2, c2, b2 = lips(8, seed=1)
    mdl.set_inducing(inducing_from_frame(mdl, n2, p2 * f, c2 * f, b2, M, seed=1))
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(64, M)), rng.normal(size=64))
    mdl.set_weights(0.02 * rng.normal(size=M), choli=mdl.choli, vscale=mdl.make_vscale())
    steps = 30
    calc = _PredictCalc(mdl)
    host = [(s, E, T, w, p.copy(), v.copy()) for s, E, T, w, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, steps, temperature=1200.0, dt_fs=1.0, friction=0.05, seed=3)]
    nn = np.concatenate(calc.nn)
    assert nn.min() >= 40 and ((nn >= 49) & (nn <= 64)).mean() > 0.9, (nn.min(), nn.max())   # lists of 49 - 64 all the way
    r0 = mdl.list_rebuilds()
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, steps, temperature=1200.0, dt_fs=1.0, friction=0.05, seed=3, chunk=16))
    assert mdl.list_rebuilds() - r0 >= 2, (r0, mdl.list_rebuilds())   # the first build and at least one rebuild inside the thirty steps
    assert len(dev) == len(host) == steps + 1
    for (s0, E0, T0, _, _, _), (s1, E1, T1, bmax), b0 in zip(host, dev, calc.betas):
        assert s0 == s1
        assert E0 == E1, (s0, E0, E1)
        assert abs(T0 - T1) <= 1e-12 * T0
        assert bmax == b0
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][4])
    assert np.array_equal(st["velocities"], host[-1][5])
    mdl.close()
