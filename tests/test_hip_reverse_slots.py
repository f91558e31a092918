"""GPU tests of the hand-over slots of the reverse pass (descriptor.hip: desc_rev_kernel, gather form) on steps that REUSE
the candidate lists.  The gradient of a pair (i -> j) is stored at j's own list position, which the reverse pass finds through
the reverse index of the candidate build (cidx -> aux -> T: the position of i among j's candidates, fixed by the build) and a
popcount of j's hit mask of THIS step.  On a step that rebuilds the candidates every atom's candidates are new and the hit
masks belong to them; on a reuse step T is older than the list it is applied to.

The oracle is the library itself with the skin set to 0: that handle rebuilds every step.  A list is a subsequence of the
sorted candidates, so a skin > 0 gives the same pairs in the same order, and forces, covloss, energy and stress are equal
bit for bit, frame by frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RC, ETA, M = 6.0, 4.0, 48
KEYS = ("energy", "forces", "stress", "beta")


def _skin0(mdl):
    from autoforce_amd import _lib
    _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 0))


def _pair(species, X, seed, **kw):
    """Two handles with one inducing set and one set of weights: the default skin (0.5 A) and skin 0."""
    from autoforce_amd import SGPRModel
    m = len(X)
    fast, slow = SGPRModel(3, 3, ETA, RC, species=species, **kw), SGPRModel(3, 3, ETA, RC, species=species, **kw)
    _skin0(slow)
    fast.set_inducing(X)
    slow.set_inducing(X)
    rng = np.random.default_rng(seed)
    fast.solve(rng.normal(size=(2 * m, m)), rng.normal(size=2 * m))
    choli, vs = fast.choli.copy(), fast.make_vscale()
    mu = 0.02 * rng.normal(size=m)
    fast.set_weights(mu, choli=choli, vscale=vs)
    slow.set_weights(mu, choli=choli, vscale=vs)
    return fast, slow


def _walk(pos, frames, sigma, seed):
    rng = np.random.default_rng(seed)
    out = [np.array(pos, float)]
    for _ in range(frames - 1):
        out.append(out[-1] + sigma * rng.normal(size=pos.shape))
    return out


def _same_frames(fast, slow, numbers, walk, cell, pbc):
    """Every frame through both handles, bit for bit (lists included); returns (reuse steps, rebuild steps) of `fast`."""
    N, kinds = len(numbers), []
    for step, p in enumerate(walk):
        r0 = fast.list_rebuilds()
        a = fast.predict(numbers, p, cell, pbc)
        kinds.append(1 if fast.list_rebuilds() > r0 else 0)
        r1 = slow.list_rebuilds()
        b = slow.predict(numbers, p, cell, pbc)
        assert slow.list_rebuilds() > r1, step
        for k in KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (step, k, kinds[-1])
        for x, y in zip(fast.neighbors(N), slow.neighbors(N)):
            assert np.array_equal(x, y), (step, "lists")
    return kinds.count(0), kinds.count(1)


def _lips_pair(seed=0, ghosts=None):
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, lips
    numbers, pos, cell, pbc = lips(6, seed=0)
    species = sorted(set(int(z) for z in numbers))
    n2, p2, c2, b2 = lips(6, seed=1)
    tmp = SGPRModel(3, 3, ETA, RC, species=species)
    X = inducing_from_frame(tmp, n2, p2, c2, b2, M, seed=1)
    tmp.close()
    kw = dict(unknown_species="ignore") if ghosts is not None else {}
    fast, slow = _pair(species, X, seed + 2, **kw)
    if ghosts is not None:
        numbers = numbers.copy()
        numbers[ghosts] = 79
    return fast, slow, (numbers, pos, cell, pbc)


def test_reuse_and_rebuild_steps_alternate():
    """lips(6): 216 atoms, three species.  Thirty frames of a random walk (0.03 A per step and component): an atom is 0.25 A
    from where the candidates were built every six steps or so, so the walk has both kinds of step."""
    fast, slow, (numbers, pos, cell, pbc) = _lips_pair()
    assert len(numbers) == 216 and len(set(numbers.tolist())) == 3
    reuse, rebuild = _same_frames(fast, slow, numbers, _walk(pos, 30, 0.03, seed=4), cell, pbc)
    assert reuse >= 5 and rebuild >= 3, (reuse, rebuild)   # (the first frame and at least two inside the walk)
    fast.close(); slow.close()


def graded_frame(seed=0):
    """The density-graded frame of test_hip_tile64.py: 550 atoms, three species, 25 layers of 5 x 5 sites (2.5 A) along x
    whose spacing falls from 3.3 A (five layers) to 1.45 A (nine layers) and back, rattled by 0.1 A — 39 to 110 neighbours
    inside 6 A."""
    rng = np.random.default_rng(seed)
    sp = np.concatenate([np.full(5, 3.3), np.linspace(3.3, 1.45, 6)[1:-1], np.full(9, 1.45), np.linspace(1.45, 3.3, 6)[1:-1]])
    x = np.concatenate([[0.0], np.cumsum(sp)[:-1]])
    a, n = 2.5, 5
    g = np.array([(xx, j * a, k * a) for xx in x for j in range(n) for k in range(n)], float)
    pos = g + 0.1 * rng.normal(size=g.shape)
    N = len(pos)
    numbers = rng.permutation(np.array([3] * (3 * N // 8) + [15] * (N // 8) + [16] * (N - 3 * N // 8 - N // 8))).astype(np.int32)
    return numbers, pos, np.diag([sp.sum(), n * a, n * a]), [True] * 3


def test_long_lists_on_reuse_steps():
    """Lists of 39 - 110 from candidate rows of more than 64 (a second round of the filter), positions
    among a neighbour's candidates of 64 and more (hit masks of more than one word) and a second pair tile.  Three frames of a
    small walk: the second and third reuse the candidates.  Against the skin-0 handle bit for bit, and the last frame against
    the CPU oracle at the tolerances of test_hip_parity.py."""
    from oracle import oracle as orc
    from autoforce_amd import Local, SGPRModel
    species = [3, 15, 16]
    numbers, pos, cell, pbc = graded_frame(0)
    _, pos2, _, _ = graded_frame(1)
    rng = np.random.default_rng(5)
    ptr, j, off = orc.neighbors(pos2, cell, [True] * 3, RC)
    X = []
    for a in rng.choice(len(numbers), size=M, replace=False):
        s = slice(ptr[a], ptr[a + 1])
        r = pos2[j[s]] - pos2[a] + off[s].astype(float) @ cell
        r = r + 0.05 * rng.normal(size=r.shape)
        keep = np.linalg.norm(r, axis=1) < RC - 1e-3
        X.append(Local(int(numbers[a]), numbers[j[s]][keep], r[keep]))
    ind_z = np.array([x.number for x in X], np.int32)
    ind_ptr = np.concatenate([[0], np.cumsum([len(x._b) for x in X])])
    Pm, nnm = orc.inducing_descriptors(3, 3, RC, species, ind_z, ind_ptr, np.concatenate([x._b for x in X]),
                                       np.concatenate([x._r for x in X]))
    L, _ = orc.jitcholesky(orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, ETA))
    choli = orc.tril_inverse(L)
    mu = np.random.default_rng(6).normal(size=M)
    fast, slow = SGPRModel(3, 3, ETA, RC, species=species), SGPRModel(3, 3, ETA, RC, species=species)
    _skin0(slow)
    for mdl in (fast, slow):
        mdl.set_inducing(X)
        mdl.set_weights(mu, choli=choli)
    walk = _walk(pos, 3, 0.01, seed=7)
    reuse, rebuild = _same_frames(fast, slow, numbers, walk, cell, pbc)
    assert (reuse, rebuild) == (2, 1)
    nn = np.diff(fast.neighbors(len(numbers))[0])
    assert nn.min() < 48 and (nn > 64).any() and nn.max() > 96, (nn.min(), nn.max())
    out = fast.predict(numbers, walk[-1], cell, pbc)   # (the same positions again: a reuse step)
    nl = orc.neighbors(walk[-1], cell, pbc, RC)
    ref = orc.frame(3, 3, RC, ETA, species, numbers, walk[-1], cell, nl, ind_z, nnm, Pm, mu, choli=choli, want_p=False)
    assert abs(out["energy"] - ref["energy"]) <= 1e-10 * max(1.0, abs(ref["energy"]))
    assert np.abs(out["forces"] - ref["forces"]).max() <= 1e-8 * np.abs(ref["forces"]).max()
    assert np.abs(out["stress"] - ref["stress"]).max() <= 1e-8 * np.abs(ref["stress"]).max()
    np.testing.assert_allclose(out["beta"], ref["beta"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(out["beta"] ** 2, ref["beta"] ** 2, rtol=1e-9, atol=1e-11)
    assert np.abs(out["forces"].sum(0)).max() <= 1e-10 * np.abs(out["forces"]).max()
    fast.close(); slow.close()


def test_self_images_on_reuse_steps():
    """si_diamond((2, 2, 1)): 32 atoms, L_z = 5.431 A < rc.  An atom is its own neighbour under several images, so several
    entries of one row of T belong to one j."""
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, si_diamond
    numbers, pos, cell, pbc = si_diamond((2, 2, 1), seed=0)
    n2, p2, c2, b2 = si_diamond((2, 2, 1), seed=1)
    tmp = SGPRModel(3, 3, ETA, RC, species=[14])
    X = inducing_from_frame(tmp, n2, p2, c2, b2, 8, seed=1)
    tmp.close()
    fast, slow = _pair([14], X, 3)
    reuse, rebuild = _same_frames(fast, slow, numbers, _walk(pos, 5, 0.01, seed=8), cell, pbc)
    assert (reuse, rebuild) == (4, 1)
    ptr, j, _ = fast.neighbors(len(numbers))
    own = [int((j[ptr[i]:ptr[i + 1]] == i).sum()) for i in range(len(numbers))]
    assert min(own) >= 2, own   # every atom meets itself under +z and -z at the least
    fast.close(); slow.close()


def test_species_outside_the_table_on_a_reuse_step():
    """Option ignore_unknown_species: the wave of a foreign atom returns early in both kernels; nobody's neighbour."""
    ghosts = np.array([5, 40, 41, 130, 215])
    fast, slow, (numbers, pos, cell, pbc) = _lips_pair(seed=1, ghosts=ghosts)
    walk = _walk(pos, 3, 0.01, seed=9)
    reuse, rebuild = _same_frames(fast, slow, numbers, walk, cell, pbc)
    assert (reuse, rebuild) == (2, 1)
    out = fast.predict(numbers, walk[-1], cell, pbc)
    assert np.abs(out["forces"][ghosts]).max() == 0.0 and np.abs(out["beta"][ghosts]).max() == 0.0
    assert np.abs(out["forces"]).max() > 0.0
    fast.close(); slow.close()


def test_md_loop_against_a_fresh_build_at_its_last_configuration():
    """Forty evaluations of the device Langevin loop at 600 K on the 216-atom frame: the candidates are rebuilt several times
    and reused in between.  Forces and covloss of the last evaluated configuration against predict() of a skin-0 handle at
    those positions, bit for bit."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    fast, slow, (numbers, pos, cell, pbc) = _lips_pair(seed=2)
    N = len(numbers)
    mass = np.array([MASS[int(z)] for z in numbers])
    v0 = np.random.default_rng(11).normal(size=(N, 3)) * np.sqrt(kB * 600.0 / mass[:, None])
    fast.md_begin(numbers, pos, cell, pbc, mass, v0, dt=FS, friction=1e-3, kT=kB * 600.0, seed=11)
    r0 = fast.list_rebuilds()
    done = 0
    for _ in range(12):   # (halt code 2: a capacity was outgrown at evaluation `done`; the rows before it stand, the call is repeated)
        sc, code = fast.md_run(40 - done, None)
        assert code in (0, 2) and (code == 2 or len(sc) == 40 - done), (done, len(sc), code)
        done += len(sc)
        if done == 40:
            break
    assert done == 40
    rebuilds = fast.list_rebuilds() - r0
    assert 3 <= rebuilds <= 20, rebuilds   # several rebuilds, and reuse steps between them
    st = fast.md_state(which=-1, results=True)
    ref = slow.predict(numbers, st["positions"], cell, pbc)
    assert np.array_equal(st["forces"], ref["forces"])
    assert np.array_equal(st["beta"], ref["beta"])
    assert np.abs(st["positions"] - pos).max() > 0.05   # the walk is not trivial
    fast.close(); slow.close()
