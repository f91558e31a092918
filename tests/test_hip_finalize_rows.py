"""GPU tests of the last kernel's row layout (finalize_next_kernel: one 16-lane row per atom, four atoms per wave) where
that layout has edges: atoms with more than 64 neighbours (pair slots beyond the first trip over the row) and atom counts
that leave rows of the last workgroup empty.  The device MD loop — Langevin with deviates drawn on the device, and
Nose-Hoover — against its host twin around the same library, bit for bit; the resident-frames form against predict()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _PredictCalc:
    """The library behind the three ASE getters (what ActiveCalculator.calculate does on a prediction-only step)."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, mdl):
        self.mdl, self.betas = mdl, []
        self._key, self.results = None, {}

    def get_property(self, name, atoms=None):
        key = atoms.positions.tobytes()
        if key != self._key:
            out = self.mdl.predict(atoms.numbers, atoms.positions, atoms.cell, atoms.pbc)
            self.results = dict(energy=out["energy"], forces=out["forces"], stress=out["stress"], free_energy=out["energy"])
            self.betas.append(float(out["beta"].max()))
            self._key = key
        return self.results[name]


def _model(frame, rc, m, seed=1, scale=0.02):
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame
    numbers, pos, cell, pbc = frame
    mdl = SGPRModel(3, 3, 4, rc, species=sorted(set(int(z) for z in numbers)))
    mdl.set_inducing(inducing_from_frame(mdl, numbers, pos, cell, pbc, m, seed=seed))
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(64, m)), rng.normal(size=64))
    mdl.set_weights(scale * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
    return mdl


def _dense():
    """LiPS at rc = 7.5 A: about 88 neighbours per atom, none with fewer than 64."""
    from autoforce_amd.workloads import lips
    frame = lips(8, seed=0)
    return _model(frame, 7.5, 24), frame


def _subset(dims, n, model_side):
    """The first n sites of a LiPS lattice (n not a multiple of 16); the model is fitted on a whole frame."""
    from autoforce_amd.workloads import lips
    numbers, pos, cell, pbc = lips(dims, seed=3)
    return _model(lips(model_side, seed=0), 6.0, 32), (numbers[:n].copy(), pos[:n].copy(), cell, pbc)


def _max_neighbours(mdl, frame):
    numbers, pos, cell, pbc = frame
    mdl.predict(numbers, pos, cell, pbc)
    return int(np.diff(mdl.neighbors(len(numbers))[0]).max())


def _langevin_against_the_host(mdl, frame, steps):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS, langevin_nvt
    numbers, pos, cell, pbc = frame
    N, T = len(numbers), 600.0
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(4).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=FS, friction=0.05, kT=kB * T, seed=91)
    sc, code = mdl.md_run(steps + 1, None, final=True)
    assert code == 0 and len(sc) == steps + 1
    st = mdl.md_state(results=True)
    xi = mdl.md_deviates(0, steps)

    class Rows:   # deals the device's deviates to the host loop
        def __init__(self):
            self.k = 0

        def normal(self, size):
            self.k += 1
            return xi[self.k - 1]

    calc = _PredictCalc(mdl)
    host = [(E, p.copy(), v.copy()) for s, E, Tk, w, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, steps, T, 1.0, 0.05, vel=vel, rng=Rows())]
    assert [h[0] for h in host] == sc[:, 0].tolist()
    assert sc[:, 11].tolist() == calc.betas                                   # the largest covloss of every step
    assert np.array_equal(host[-1][1], st["positions"]) and np.array_equal(host[-1][2], st["velocities"])


def _nose_hoover_against_the_host(mdl, frame, steps):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS, nose_hoover_nvt
    numbers, pos, cell, pbc = frame
    N, T, tdamp = len(numbers), 700.0, 20.0
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(8).normal(size=(N, 3)) * np.sqrt(kB * T / mass[:, None])
    calc = _PredictCalc(mdl)
    host = [(E, p.copy(), v.copy(), z, zi) for s, E, Tk, w, p, v, z, zi in
            nose_hoover_nvt(calc, numbers, pos, cell, pbc, steps, temperature=T, dt_fs=1.0, tdamp_fs=tdamp, vel=vel)]
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=0.0, kT=kB * T, ttime=tdamp * FS)
    sc, code = mdl.md_run(steps + 1, None, final=True)
    assert code == 0 and len(sc) == steps + 1
    assert sc[:, 0].tolist() == [h[0] for h in host]
    assert np.array_equal(sc[:, 14], np.array([h[3] for h in host])) and np.array_equal(sc[:, 15], np.array([h[4] for h in host]))
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][1]) and np.array_equal(st["velocities"], host[-1][2])


def test_md_with_more_than_64_neighbours_equals_the_host_twin():
    mdl, frame = _dense()
    assert _max_neighbours(mdl, frame) > 80    # (slots of a second and a third row of the second trip)
    _langevin_against_the_host(mdl, frame, 24)
    _nose_hoover_against_the_host(mdl, frame, 16)
    mdl.close()


@pytest.mark.parametrize("dims,n,model_side", [((17, 17, 15), 4099, 16), ((4, 4, 4), 5, 4)])
def test_md_at_atom_counts_that_leave_rows_empty_equals_the_host_twin(dims, n, model_side):
    mdl, frame = _subset(dims, n, model_side)
    assert n % 16 != 0
    _langevin_against_the_host(mdl, frame, 12)
    _nose_hoover_against_the_host(mdl, frame, 8)
    mdl.close()


def test_resident_frames_on_a_dense_frame_equal_predict():
    """sgpr_step_dev_next over resident frames (finalize_next_kernel<1>: each launch also bins the next frame) against
    predict() (the six-launch path, finalize_gather_kernel) frame by frame: forces and beta bit for bit."""
    import torch
    from autoforce_amd import _lib
    mdl, (numbers, pos, cell, pbc) = _dense()
    lib = _lib.load()
    N = len(numbers)
    rng = np.random.default_rng(6)
    frames = [pos]
    for _ in range(12):
        frames.append(frames[-1] + 0.012 * rng.normal(size=pos.shape))
    ref = [mdl.predict(numbers, p, cell, pbc) for p in frames]
    assert _max_neighbours(mdl, (numbers, frames[0], cell, pbc)) > 64
    dev = torch.device("cuda:0")
    fr = torch.tensor(np.stack(frames), device=dev)
    cl = torch.tensor(cell, device=dev)
    out = torch.zeros((len(frames), 4 * N + 11), dtype=torch.float64, device=dev)
    h = mdl.handle
    for k in range(len(frames)):
        nxt = fr[k + 1].data_ptr() if k + 1 < len(frames) else None
        _lib.check(lib.sgpr_step_dev_next(h, fr[k].data_ptr(), cl.data_ptr(), out[k].data_ptr(), nxt, None))
    _lib.check(lib.sgpr_sync_check(h, None))
    o = out.cpu().numpy()
    for k, r in enumerate(ref):
        assert np.array_equal(o[k, :3 * N].reshape(N, 3), r["forces"]), k
        assert np.array_equal(o[k, 3 * N:4 * N], r["beta"]), k
        assert o[k, 4 * N] == r["energy"], k
    mdl.close()
