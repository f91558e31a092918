"""GPU tests of path-integral MD inside the device loop (sgpr_md_pimd: a ring polymer under BAOAB with the PILE-L thermostat): P
plain steps of the one live handle per evaluation with md_pimd_sums_kernel, md_pimd_gate_kernel and md_pimd_move_kernel behind
them, against the host twin workloads.pimd_baoab around the same library, bit for bit — the sixteen scalars of every evaluation,
the record, the final beads and their velocities —, as one call and cut into several; one bead against the Langevin loop that
exists (md_begin + md_run); deviates drawn on the device; frames off the kernels' grids (a part wave and a part tile, odd P, P = 2,
P = 32); a covloss halt in the middle, resumed; two identical runs; the refusals, in both directions.  Frame, model and the
calculator are those of test_hip_npt_device.py."""
import numpy as np
import pytest

from test_hip_npt_device import _PredictCalc, _model

pytestmark = pytest.mark.gpu

EVALS = 24
T, DT_FS, FRICTION, LAMBDA = 600.0, 1.0, 1e-2, 0.5
CUTS = ((EVALS,), (7, 1, 6, 10))


class _Calc(_PredictCalc):
    """_PredictCalc with the third getter of the twin: the covloss of the frame it evaluated last (its largest value is all
    the polymer asks for)."""

    def get_covloss(self):
        return np.array(self.betas[-1:])


def _polymer(numbers, pos, P, seed=5, spread=0.03, keep=None):
    """P beads rattled a little around the frame, Maxwell-Boltzmann velocities at P T, masses."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS
    rng = np.random.default_rng(seed)
    if keep is not None:
        numbers, pos = numbers[keep], pos[keep]
    mass = np.array([MASS[int(z)] for z in numbers])
    beads = pos[None] + spread * rng.normal(size=(P,) + pos.shape)
    vel = rng.normal(size=beads.shape) * np.sqrt(P * kB * T / mass)[None, :, None]
    return numbers, beads, vel, mass


def _noise(evals, P, N, seed=9):
    return np.random.default_rng(seed).normal(size=(evals, P, N, 3))


def _twin(mdl, numbers, beads, vel, cell, pbc, noise, evals=EVALS, **kw):
    from autoforce_amd.workloads import pimd_baoab
    return list(pimd_baoab(_Calc(mdl), numbers, beads, cell, pbc, evals, temperature=T, dt_fs=DT_FS, friction=FRICTION, pile_lambda=LAMBDA, vel=vel,
                           species=mdl.species, noise=lambda n: noise[n], **kw))


def _begin(mdl, numbers, beads, vel, mass, cell, pbc, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    par = dict(dt=DT_FS * FS, kT=kB * T, friction=FRICTION, pile_lambda=LAMBDA)
    par.update(kw)
    mdl.pimd_begin(numbers, beads, cell, pbc, mass, vel, **par)


def _device(mdl, cuts, noise):
    rows, Es, covs, at = [], [], [], 0
    for n in cuts:
        sc, code = mdl.md_run(n, None if noise is None else noise[at:at + n])
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        E, cov = mdl.pimd_info()
        assert len(E) == n
        rows.extend(sc)
        Es.extend(E)
        covs.extend(cov)
        at += n
    return np.array(rows), np.array(Es), np.array(covs)


def _same_rows(sc, E, cov, host):
    """Device scalars and record of consecutive evaluations against the twin's rows, bit for bit."""
    hE, hc = np.array([h["energies"] for h in host]), np.array([h["covmax"] for h in host])
    print("max |dE|", np.abs(E - hE).max(), "max |d mv2|", np.abs(sc[:, 12] - np.array([h["mv2"] for h in host])).max(),
          "max |d cv|", np.abs(sc[:, 14] - np.array([h["cv"] for h in host])).max())
    assert np.array_equal(E, hE) and np.array_equal(cov, hc)
    assert [int(r[1]) for r in sc] == [h["cbead"] for h in host]
    assert np.array_equal(sc[:, 11], hc.max(axis=1))
    for col, key in ((0, "energy"), (12, "mv2"), (13, "mv2_pre"), (14, "cv"), (15, "spring")):
        d = np.nonzero(sc[:, col] != np.array([h[key] for h in host]))[0]
        assert not len(d), (key, d[:3], sc[d[:3], col], [host[i][key] for i in d[:3]])
    assert not sc[:, 2:11].any()                                     # the spare columns and the overflow word


def test_device_loop_is_the_twin_bit_for_bit():
    mdl, (numbers, pos, cell, pbc) = _model()
    P = 4
    numbers, beads, vel, mass = _polymer(numbers, pos, P)
    noise = _noise(EVALS, P, len(numbers))
    host = _twin(mdl, numbers, beads, vel, cell, pbc, noise)
    assert len(host) == EVALS + 1
    out = {}
    for cuts in CUTS:
        _begin(mdl, numbers, beads, vel, mass, cell, pbc)
        sc, E, cov = _device(mdl, cuts, noise)
        _same_rows(sc, E, cov, host[:EVALS])
        st = mdl.pimd_state()
        assert st["pending"]
        assert np.array_equal(st["positions"], host[EVALS]["beads"]) and np.array_equal(st["velocities_pre"], host[EVALS]["velocities_pre"])
        prev = mdl.pimd_state(which=-1, results=True)
        assert np.array_equal(prev["positions"], host[EVALS - 1]["beads"]) and np.array_equal(prev["velocities_pre"], host[EVALS - 1]["velocities_pre"])
        assert np.array_equal(prev["forces"], host[EVALS - 1]["forces"]) and np.array_equal(prev["energy"], host[EVALS - 1]["energies"])
        assert np.array_equal(prev["velocities"], host[EVALS - 1]["velocities"])   # (the closing half kick applied)
        out[cuts] = (sc, E, cov, st["positions"], st["velocities_pre"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                  # however the run is cut into calls
    assert np.abs(host[EVALS]["beads"] - beads).max() > 1e-2         # the walk is not trivial
    assert host[3]["spring"] > 0.0 and host[3]["mv2"] != host[3]["mv2_pre"] and host[0]["mv2"] == host[0]["mv2_pre"]
    mdl.close()


def test_one_bead_has_the_bits_of_the_langevin_loop():
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl, (numbers, pos, cell, pbc) = _model()
    numbers, beads, vel, mass = _polymer(numbers, pos, 1, spread=0.0)
    N = len(numbers)
    noise = _noise(EVALS, 1, N)
    mdl.md_begin(numbers, beads[0], cell, pbc, mass, vel[0], dt=DT_FS * FS, friction=FRICTION, kT=kB * T)
    sc0, code = mdl.md_run(EVALS, noise[:, 0])
    assert code == 0 and len(sc0) == EVALS
    st0 = mdl.md_state()
    _begin(mdl, numbers, beads, vel, mass, cell, pbc)
    sc1, E, cov = _device(mdl, (EVALS,), noise)
    st1 = mdl.pimd_state()
    print("max |dx|", np.abs(st1["positions"][0] - st0["positions"]).max(), "max |dE|", np.abs(sc1[:, 0] - sc0[:, 0]).max())
    assert np.array_equal(st1["positions"][0], st0["positions"]) and np.array_equal(st1["velocities_pre"][0], st0["velocities_pre"])
    assert np.array_equal(sc1[:, 0], sc0[:, 0]) and np.array_equal(sc1[:, 11], sc0[:, 11])
    assert np.array_equal(E[:, 0], sc0[:, 0]) and np.array_equal(cov[:, 0], sc0[:, 11])
    assert not sc1[:, 15].any() and (sc1[:, 1] == 1.0).all()         # no springs, one bead
    assert np.abs(st1["positions"][0] - beads[0]).max() > 1e-2
    mdl.close()


def test_deviates_drawn_on_the_device():
    mdl, (numbers, pos, cell, pbc) = _model()
    P, evals = 3, 8
    numbers, beads, vel, mass = _polymer(numbers, pos, P)
    N = len(numbers)
    got = []
    for cuts in ((evals,), (3, 5)):
        _begin(mdl, numbers, beads, vel, mass, cell, pbc, seed=5)
        sc, E, cov = _device(mdl, cuts, None)
        st = mdl.pimd_state()
        got.append((sc, E, cov, st["positions"], st["velocities_pre"]))
    dev = mdl.md_deviates(0, evals * P).reshape(evals, P, N, 3)      # (t = n P + k)
    assert abs(dev.std() - 1.0) < 0.02 and not np.array_equal(dev[0, 0], dev[0, 1])
    _begin(mdl, numbers, beads, vel, mass, cell, pbc)
    sc, E, cov = _device(mdl, (evals,), dev)
    st = mdl.pimd_state()
    got.append((sc, E, cov, st["positions"], st["velocities_pre"]))
    for q in got[1:]:
        for a, c in zip(got[0], q):
            assert np.array_equal(a, c)
    mdl.close()


@pytest.mark.parametrize("N,P", [(200, 3), (512, 2), (200, 32)], ids=["part-wave-odd-P", "P=2", "P=32"])
def test_frames_off_the_kernels_grids(N, P):
    """N = 200: less than the 256 threads of the sums (the last wave takes eight atoms), and the move kernel's last tile of sixteen
    atoms takes eight; P = 3: odd, no Nyquist column in C.  P = 2: the centroid and the Nyquist mode only, no sine column.  P = 32:
    the most a polymer may have, six trips of the move kernel's 256 threads over the tile."""
    mdl, (numbers, pos, cell, pbc) = _model()
    keep = None if N == len(numbers) else np.sort(np.random.default_rng(11).choice(len(numbers), size=N, replace=False))
    numbers, beads, vel, mass = _polymer(numbers, pos, P, keep=keep)
    evals = 6
    noise = _noise(evals, P, N)
    host = _twin(mdl, numbers, beads, vel, cell, pbc, noise, evals=evals)
    _begin(mdl, numbers, beads, vel, mass, cell, pbc)
    sc, E, cov = _device(mdl, (2, 4), noise)
    _same_rows(sc, E, cov, host[:evals])
    st = mdl.pimd_state()
    assert np.array_equal(st["positions"], host[evals]["beads"]) and np.array_equal(st["velocities_pre"], host[evals]["velocities_pre"])
    mdl.close()


def test_a_covloss_halt_returns_that_configuration_and_the_run_resumes():
    mdl, (numbers, pos, cell, pbc) = _model()
    P = 4
    numbers, beads, vel, mass = _polymer(numbers, pos, P)
    noise = _noise(EVALS, P, len(numbers))
    host = _twin(mdl, numbers, beads, vel, cell, pbc, noise)
    b = np.array([h["covmax"].max() for h in host])
    print("largest covloss per evaluation", b)
    # the gate between two observed values: below the first evaluation behind the third that exceeds every earlier one — or, on a
    # walk without one, below the largest value of all (its first occurrence: evaluation 0 where the covloss only falls)
    later = [k for k in range(3, EVALS) if b[k] > b[:k].max()]
    k = later[0] if later else int(np.argmax(b[:EVALS]))
    ediff = 0.5 * (b[:k].max() + b[k]) if k else 0.5 * (b[0] + b[1:EVALS].max())
    assert (b[:k] < ediff).all() and b[k] >= ediff
    _begin(mdl, numbers, beads, vel, mass, cell, pbc)
    sc1, code = mdl.md_run(EVALS, noise, ediff=ediff)
    assert code == 1 and len(sc1) == k + 1, (code, len(sc1), k)
    E1, cov1 = mdl.pimd_info()
    _same_rows(sc1, E1, cov1, host[:k + 1])
    assert sc1[k, 11] == b[k] and int(sc1[k, 1]) == host[k]["cbead"]  # the bead that carried the largest covloss
    st = mdl.pimd_state(results=True)
    assert np.array_equal(st["positions"], host[k]["beads"]) and np.array_equal(st["velocities_pre"], host[k]["velocities_pre"])   # nothing has moved
    assert np.array_equal(st["energy"], host[k]["energies"]) and np.array_equal(st["beta"].max(axis=1), host[k]["covmax"])
    assert np.array_equal(st["velocities"], host[k]["velocities"])
    sc2, code = mdl.md_run(EVALS - k, noise[k:])                     # the model as it was: the bits of the run that was never cut
    assert code == 0 and len(sc2) == EVALS - k
    E2, cov2 = mdl.pimd_info()
    _same_rows(sc2, E2, cov2, host[k:EVALS])
    st = mdl.pimd_state()
    assert np.array_equal(st["positions"], host[EVALS]["beads"]) and np.array_equal(st["velocities_pre"], host[EVALS]["velocities_pre"])
    mdl.close()


def test_two_identical_runs_give_the_same_bits():
    mdl, (numbers, pos, cell, pbc) = _model()
    numbers, beads, vel, mass = _polymer(numbers, pos, 4)
    noise = _noise(10, 4, len(numbers))
    got = []
    for _ in range(2):
        _begin(mdl, numbers, beads, vel, mass, cell, pbc)
        sc, E, cov = _device(mdl, (10,), noise)
        st = mdl.pimd_state()
        got.append((sc, E, cov, st["positions"], st["velocities_pre"]))
    for a, c in zip(*got):
        assert np.array_equal(a, c)
    mdl.close()


def test_pimd_error_cases_leave_the_handle_working():
    """Every refusal of sgpr_md_pimd but one — a run begun on several ranks needs a second process with its own device — and the
    refusal of every other attach function behind it."""
    from autoforce_amd import _lib
    from autoforce_amd._lib import SgprError, f64, ptr
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    mdl, (numbers, pos, cell, pbc) = _model()
    N = len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    lib = _lib.load()
    numbers, beads, vel, mass = _polymer(numbers, pos, 3)

    def pimd(P=3, kT=kB * T, friction=FRICTION, lam=LAMBDA):
        R = f64(np.repeat(pos[None], max(P, 1), axis=0))
        return lib.sgpr_md_pimd(mdl.handle, int(P), ptr(R), None, float(kT), float(friction), float(lam))

    def begin(**kw):
        mdl.md_begin(numbers, pos, cell, pbc, mass, None, dt=DT_FS * FS, friction=0.0, kT=kB * T, **kw)

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    begin()
    assert pimd(P=0) == _lib.E_INVALID and pimd(P=33) == _lib.E_INVALID
    assert pimd(kT=0.0) == _lib.E_INVALID and pimd(friction=-1.0) == _lib.E_INVALID and pimd(lam=-0.5) == _lib.E_INVALID
    works()
    begin(ttime=25.0 * FS)
    assert pimd() == _lib.E_INVALID                                  # another thermostat
    begin(ttime=25.0 * FS, pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
    assert pimd() == _lib.E_INVALID                                  # ... and a barostat
    begin(ml_filter=0.8)
    assert pimd() == _lib.E_UNSUPPORTED                              # a filter
    begin(fixed=np.arange(N) < 5)
    assert pimd() == _lib.E_UNSUPPORTED                              # a mask
    member, _ = _model(seed=2)
    begin()
    mdl.md_committee([member])
    assert pimd() == _lib.E_UNSUPPORTED                              # a committee
    mdl.md_committee([])
    works()
    begin()
    mdl.md_meta([("distance", 0, 1)], [0.1], 0.01)
    assert pimd() == _lib.E_UNSUPPORTED                              # a bias
    begin()
    mdl.md_record(2)
    assert pimd() == _lib.E_UNSUPPORTED                              # an armed frame record
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    assert pimd() == _lib.E_UNSUPPORTED                              # a relaxation
    mdl.neb_begin(numbers, np.array([pos, pos + 0.01, pos + 0.02]), cell, pbc, 0.05)
    assert pimd() == _lib.E_UNSUPPORTED                              # a band
    works()
    begin()
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert pimd() == _lib.E_INVALID                                  # the run has started
    works()
    with pytest.raises(ValueError):
        mdl.pimd_begin(numbers, beads[:0], cell, pbc, mass, dt=FS, kT=kB * T)
    with pytest.raises(SgprError):
        mdl.pimd_begin(numbers, np.repeat(pos[None], 33, axis=0), cell, pbc, mass, dt=FS, kT=kB * T)
    with pytest.raises(RuntimeError, match="no run on this model"):   # a refused polymer leaves no run behind, and md_run says so
        mdl.md_run(1)
    with pytest.raises(RuntimeError, match="no polymer on this model"):
        mdl.pimd_state()
    # ... and behind sgpr_md_pimd every other attach function refuses
    _begin(mdl, numbers, beads, vel, mass, cell, pbc)
    assert pimd() == _lib.E_INVALID                                  # a polymer already
    held = np.zeros((N, 3), np.uint8)
    held[:5] = 1
    assert lib.sgpr_md_fix(mdl.handle, ptr(held)) == _lib.E_UNSUPPORTED
    assert lib.sgpr_md_thermostat(mdl.handle, 1, 25.0 * FS, kB * T) == _lib.E_INVALID
    ext = f64([0.0] * 6)
    assert lib.sgpr_md_barostat(mdl.handle, 1.0, ptr(ext), None, 1.0) == _lib.E_UNSUPPORTED
    assert lib.sgpr_md_relax(mdl.handle, 0.05, None, 0, None) == _lib.E_UNSUPPORTED
    band = f64(np.array([pos, pos + 0.01, pos + 0.02]))
    assert lib.sgpr_md_neb(mdl.handle, 1, ptr(band), 0.05, 0.1, 0, None) == _lib.E_UNSUPPORTED
    assert lib.sgpr_md_filter(mdl.handle, 0.8, None, None) == _lib.E_UNSUPPORTED
    assert lib.sgpr_md_record(mdl.handle, 1, 3) == _lib.E_UNSUPPORTED
    with pytest.raises(SgprError):
        mdl.md_committee([member])
    with pytest.raises(NotImplementedError):
        mdl.md_meta([("distance", 0, 1)], [0.1], 0.01)
    assert lib.sgpr_md_state(mdl.handle, None, None, None, None, 0) == _lib.E_INVALID
    assert lib.sgpr_md_velocities(mdl.handle, ptr(np.empty((N, 3)))) == _lib.E_INVALID
    member.close()
    sc, code = mdl.md_run(3, None, final=True)                       # and after all that, the real thing runs (no noise: the O step adds none)
    assert code == 0 and len(sc) == 3
    st = mdl.pimd_state(results=True)
    assert st["energy"].mean() == pytest.approx(sc[-1, 0], rel=1e-14)   # `final`: the current configuration is the one evaluated last
    assert pimd() == _lib.E_INVALID                                  # ... and a polymer that has started
    works()
    mdl.close()
