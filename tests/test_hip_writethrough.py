"""GPU tests of the step's hand-over arrays (the GEMM epilogues store theirs write-through, csrc/sgpr_internal.h): a store
that is dropped or lands in the wrong place leaves the PREVIOUS frame's bytes in an array that the next kernel reads, so a handle
that has seen another frame must give, bit for bit, what a fresh handle gives; the two places where the list kernel reads
back what it has just stored (more than 96 neighbours, more than 256 candidates) against the oracle; and the device
Langevin loop against its host twin at a size whose last workgroups are partly empty."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPECIES = {1: [3], 3: [3, 15, 16]}
_inducing = {}


def _sites(N, seed, spacing=2.72):
    """N atoms on a rattled simple-cubic grid with vacancies: the smallest grid that holds them; one atom sits in a 4 A box
    and meets its own images."""
    rng = np.random.default_rng(seed)
    if N == 1:
        dims, spacing = (1, 1, 1), 4.0
    else:
        n = int(np.ceil(N ** (1.0 / 3.0) - 1e-9))
        dims = (n, n, n)
        while (dims[0] - 1) * n * n >= N:
            dims = (dims[0] - 1, n, n)
    grid = np.stack(np.meshgrid(*[np.arange(k) for k in dims], indexing="ij"), -1).reshape(-1, 3)
    pick = np.sort(rng.choice(len(grid), size=N, replace=False))
    pos = grid[pick] * spacing + rng.uniform(-0.25, 0.25, size=(N, 3))
    return pos, np.diag([k * spacing for k in dims]).astype(float)


def _frame(N, nspec, seed):
    pos, cell = _sites(N, seed)
    rng = np.random.default_rng(100 + seed)
    numbers = rng.choice(SPECIES[nspec], size=N).astype(np.int32)
    return numbers, pos, cell, np.array([True, True, True])


def _inducing_set(nspec, m):
    """m LCEs of a 64-atom frame, drawn once per (species, m) by a handle of their own."""
    key = (nspec, m)
    if key not in _inducing:
        from autoforce_amd import SGPRModel
        from autoforce_amd.workloads import inducing_from_frame, lips
        numbers, pos, cell, pbc = lips(4, seed=1)
        if nspec == 1:
            numbers = np.full(len(numbers), 3, np.int32)
        mdl = SGPRModel(3, 3, 4, 6.0, species=SPECIES[nspec])
        _inducing[key] = inducing_from_frame(mdl, numbers, pos, cell, pbc, m, seed=1)
        mdl.close()
    return _inducing[key]


def _handle(nspec, m):
    from autoforce_amd import SGPRModel
    mdl = SGPRModel(3, 3, 4, 6.0, species=SPECIES[nspec])
    mdl.set_inducing(_inducing_set(nspec, m))
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(64, m)), rng.normal(size=64))
    mdl.set_weights(0.02 * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
    return mdl


def _evaluate(mdl, frame):
    """One step through sgpr_compute_view: forces, covloss, energy, virial (the packed results where the device wrote them)
    and the descriptors the step left on the device."""
    from autoforce_amd import _lib
    numbers, pos, cell, pbc = frame
    N = len(numbers)
    out = C.c_void_p(0)
    _lib.check(_lib.load().sgpr_compute_view(mdl.handle, N, _lib.ptr(_lib.i32(numbers)), _lib.ptr(_lib.f64(pos)),
                                             _lib.ptr(_lib.f64(cell)), _lib.ptr(_lib.i32(np.asarray(pbc, np.int32))), 0, 1,
                                             C.addressof(out)))
    buf = np.frombuffer((C.c_double * (4 * N + 17)).from_address(out.value), dtype=np.float64).copy()
    return dict(forces=buf[:3 * N], covloss=buf[3 * N:4 * N], energy=buf[4 * N:4 * N + 1], virial=buf[4 * N + 1:4 * N + 10],
                descriptors=mdl.descriptors(N))


@pytest.mark.parametrize("m", [8, 48])
@pytest.mark.parametrize("nspec", [1, 3])
@pytest.mark.parametrize("N", [1, 5, 130, 257])
def test_a_handle_that_saw_another_frame_equals_a_fresh_one(N, nspec, m):
    """Frame A, then frame B of the same size (other vacancies, other species, other list lengths) on one handle: every
    result of B equals, bit for bit, that of a handle that only saw B.  N = 1, 5: waves beyond the last atom in the only
    workgroup; 130, 257: a partly filled last row tile and last workgroup behind full ones; one species: packed rows of 40
    in a stride of 64 (the zero pad is stored every step); m = 8, 48: partial and full column tiles."""
    a, b = _frame(N, nspec, 1), _frame(N, nspec, 2)
    used = _handle(nspec, m)
    ra = _evaluate(used, a)
    rb = _evaluate(used, b)
    fresh = _handle(nspec, m)
    ref = _evaluate(fresh, b)
    for k in ("forces", "covloss", "energy", "virial", "descriptors"):
        assert np.isfinite(ref[k]).all(), k
        assert np.array_equal(rb[k], ref[k]), (k, np.abs(rb[k] - ref[k]).max())
    if N > 1:
        assert not np.array_equal(ra["forces"], ref["forces"])  # (the frames do differ)
    used.close()
    fresh.close()


def test_long_lists_read_back_inside_the_list_kernel_against_the_oracle():
    """216 atoms on a dense cubic grid (1.58 A): every atom has more than 128 neighbours inside rc = 6, so the forward tiles
    beyond the second read the list entries back from memory, and more than 256 candidates inside rc + skin (0.5 A), so the
    unsorted tail of the candidate list is read back too.  Tolerances of test_hip_calculator.py."""
    from autoforce_amd import _lib
    from oracle import oracle as orc
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = g * 1.58 + rng.uniform(-0.15, 0.15, size=(216, 3))
    cell = np.diag([6 * 1.58] * 3)
    pbc = np.array([True, True, True])
    numbers = rng.choice(SPECIES[3], size=216).astype(np.int32)
    mdl = _handle(3, 48)
    _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 500))
    out = mdl.predict(numbers, pos, cell, pbc, cov=True)
    nl = orc.neighbors(pos, cell, pbc, 6.0)
    assert np.diff(nl[0]).min() > 128
    assert np.diff(orc.neighbors(pos, cell, pbc, 6.5)[0]).min() > 256
    p, j, off = mdl.neighbors(216)
    assert np.array_equal(np.diff(p), np.diff(nl[0]))
    X = mdl.X
    species = np.array(mdl.species, np.int32)
    ind_z = np.array([x.number for x in X], np.int32)
    ind_ptr = np.concatenate([[0], np.cumsum([len(x._b) for x in X])])
    Pm, nnm = orc.inducing_descriptors(3, 3, 6.0, species, ind_z, ind_ptr, np.concatenate([x._b for x in X]),
                                       np.concatenate([x._r for x in X]))
    ref = orc.frame(3, 3, 6.0, 4.0, species, numbers, pos, cell, nl, ind_z, nnm, Pm, mdl.mu, choli=mdl.choli)
    np.testing.assert_allclose(out["cov"], ref["cov"], rtol=1e-9, atol=1e-12)
    assert abs(out["energy"] - ref["energy"]) <= 1e-9 * abs(ref["energy"])
    assert np.abs(out["forces"] - ref["forces"]).max() <= 1e-8 * np.abs(ref["forces"]).max()
    assert np.abs(out["stress"] - ref["stress"]).max() <= 1e-8 * np.abs(ref["stress"]).max()
    mdl.close()


class _PredictCalc:
    """The library behind the ASE getters (a prediction-only step of the calculator)."""

    def __init__(self, mdl):
        self.mdl, self.betas, self._key, self.results = mdl, [], None, {}

    def get_property(self, name, atoms=None):
        key = atoms.positions.tobytes()
        if key != self._key:
            out = self.mdl.predict(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc)
            self.results = dict(energy=out["energy"], forces=out["forces"], stress=out["stress"], free_energy=out["energy"])
            self.betas.append(float(out["beta"].max()))
            self._key = key
        return self.results[name]


def test_device_langevin_at_130_atoms_equals_its_host_twin_bit_for_bit():
    """Thirty steps of the device loop at N = 130 (33 workgroups of four waves, the last half empty; a partly filled last row
    tile) against the host loop around the same library: energies and largest covloss of every step and the final state,
    bit for bit.  A skin of 0.1 A: thermal motion at 600 K crosses skin / 2 every few femtoseconds, so the thirty steps hold
    several rebuilds of the candidate lists with reuse steps between them."""
    from autoforce_amd import _lib
    from autoforce_amd.workloads import langevin_nvt, langevin_nvt_device
    numbers, pos, cell, pbc = _frame(130, 3, 3)
    steps = 30
    kw = dict(temperature=600.0, dt_fs=1.0, friction=0.05, seed=3)
    mdl = _handle(3, 48)
    _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"skin_milliangstrom", 100))
    calc = _PredictCalc(mdl)
    host = [(s, E, T, p.copy(), v.copy()) for s, E, T, w, p, v in langevin_nvt(calc, numbers, pos, cell, pbc, steps, **kw)]
    r0 = mdl.list_rebuilds()
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, steps, chunk=16, **kw))
    assert len(dev) == len(host) == steps + 1
    for (s0, E0, T0, _, _), (s1, E1, T1, bmax), b0 in zip(host, dev, calc.betas):
        assert s0 == s1
        assert E0 == E1, (s0, E0, E1)
        assert abs(T0 - T1) <= 1e-12 * T0  # (the sum over atoms runs in another order)
        assert bmax == b0
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][3])
    assert np.array_equal(st["velocities"], host[-1][4])
    rebuilds = mdl.list_rebuilds() - r0
    assert 2 <= rebuilds < steps, rebuilds
    mdl.close()
