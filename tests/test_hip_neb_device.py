"""GPU tests of the nudged elastic band inside the device loop (sgpr_md_neb: ASE's default `aseneb` method under FIRE on all
interior images at once): K plain steps of the one live handle per evaluation with md_neb_sums_kernel, md_neb_fire_kernel and
md_neb_move_kernel behind them, against the host twin workloads.neb_fire around the same library, bit for bit — the sixteen
scalars of every evaluation, the band record, the final band and its velocity —, as one call and cut into several, with the
climbing image and with held components; frames off the kernels' grids (an idle part-wave, K = 1, K = 16); a covloss halt in
the middle, resumed with and without a reset of the optimizer; convergence as the third halt code; the error cases of
sgpr_md_neb; two identical runs.  Frame, model and the calculator are those of test_hip_npt_device.py."""
import numpy as np
import pytest

from test_hip_npt_device import _PredictCalc, _model

pytestmark = pytest.mark.gpu

EVALS = 40
FMAX = 1e-9   # (far below anything 40 evaluations reach on this frame: the bit-for-bit walks never converge)
CUTS = ((EVALS,), (7, 1, 12, 20))


class _Calc(_PredictCalc):
    """_PredictCalc with the third getter of the twin: the covloss of the frame it evaluated last (its largest value is all
    the band asks for)."""

    def get_covloss(self):
        return np.array(self.betas[-1:])


def _band(pos, K, seed=5, amp=0.08, jitter=0.02, keep=None):
    """K + 2 images: the frame, a rattled copy of it, and K interior images interpolated between the two and rattled a little."""
    rng = np.random.default_rng(seed)
    end = pos + np.clip(amp * rng.normal(size=pos.shape), -0.2, 0.2)
    imgs = [pos + (i / (K + 1.0)) * (end - pos) + (jitter * rng.normal(size=pos.shape) if 0 < i < K + 1 else 0.0) for i in range(K + 2)]
    return np.array(imgs if keep is None else [r[keep] for r in imgs])


def _twin(mdl, numbers, images, cell, pbc, evals=EVALS, fmax=FMAX, **kw):
    from autoforce_amd.workloads import neb_fire
    return list(neb_fire(_Calc(mdl), numbers, images, cell, pbc, evals, fmax, species=mdl.species, **kw))


def _device(mdl, cuts):
    rows, Es, covs = [], [], []
    for n in cuts:
        sc, code = mdl.md_run(n, None)
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        E, cov = mdl.neb_info()
        assert len(E) == n
        rows.extend(sc)
        Es.extend(E)
        covs.extend(cov)
    return np.array(rows), np.array(Es), np.array(covs)


def _same_rows(sc, E, cov, host):
    """Device scalars and band record of consecutive evaluations against the twin's rows, bit for bit."""
    hE, hc = np.array([h["energies"] for h in host]), np.array([h["covmax"] for h in host])
    print("max |dE|", np.abs(E - hE).max(), "max |dgmax2|", np.abs(sc[:, 12] - np.array([h["gmax2"] for h in host])).max())
    assert np.array_equal(E, hE) and np.array_equal(cov, hc)
    assert [r[0] for r in sc] == [h["energies"][h["imax"] - 1] for h in host]
    assert [int(r[1]) for r in sc] == [h["imax"] for h in host] and [int(r[2]) for r in sc] == [h["cimg"] for h in host]
    assert np.array_equal(sc[:, 11], hc.max(axis=1))
    for col, key in ((12, "gmax2"), (13, "P"), (14, "dt"), (15, "a")):
        d = np.nonzero(sc[:, col] != np.array([h[key] for h in host]))[0]
        assert not len(d), (key, d[:3], sc[d[:3], col], [host[i][key] for i in d[:3]])
    assert not sc[:, 3:11].any()                                     # the spare columns and the overflow word


@pytest.mark.parametrize("case", ["plain", "climb", "held"])
def test_device_loop_is_the_twin_bit_for_bit(case):
    mdl, (numbers, pos, cell, pbc) = _model()
    N, K = len(numbers), 3
    images = _band(pos, K)
    kw = dict(climb=(case == "climb"))
    if case == "held":   # a quarter of the components
        kw["fixed"] = np.random.default_rng(9).random((N, 3)) < 0.25
    host = _twin(mdl, numbers, images, cell, pbc, **kw)
    assert len(host) == EVALS + 1 and not host[-1]["converged"]
    out = {}
    for cuts in CUTS:
        mdl.neb_begin(numbers, images, cell, pbc, FMAX, **kw)
        sc, E, cov = _device(mdl, cuts)
        _same_rows(sc, E, cov, host[:EVALS])
        st = mdl.neb_state()
        assert np.array_equal(st["positions"], host[EVALS]["band"]) and np.array_equal(st["velocities"], host[EVALS]["velocities"])
        prev = mdl.neb_state(which=-1, results=True)
        assert np.array_equal(prev["positions"], host[EVALS - 1]["band"])
        assert np.array_equal(prev["forces"], host[EVALS - 1]["forces"]) and np.array_equal(prev["energy"], host[EVALS - 1]["energies"])
        out[cuts] = (sc, E, cov, st["positions"], st["velocities"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                  # however the run is cut into calls
    assert len({(h["dt"], h["a"]) for h in host}) > 3                # the time step has been raised (the walk is not trivial)
    assert np.abs(host[EVALS]["band"] - images[1:-1]).max() > 1e-4
    if case == "held":
        fx = kw["fixed"]
        assert 0.2 < fx.mean() < 0.3
        assert np.array_equal(out[CUTS[0]][3][:, fx], images[1:-1][:, fx])   # held coordinates keep their bits
        assert not out[CUTS[0]][4][:, fx].any() and out[CUTS[0]][4][:, ~fx].all()
    mdl.close()


@pytest.mark.parametrize("N,K", [(200, 3), (512, 1), (200, 16)], ids=["part-wave", "K=1", "K=16"])
def test_frames_off_the_kernels_grids(N, K):
    """N = 200: not a multiple of the move kernel's 64 atoms per workgroup and less than the 256 threads of the sums — the
    last wave of md_neb_sums_kernel takes eight atoms and has 56 idle lanes.  K = 1: the only image is imax, its tangent t_1 + t_2,
    both neighbours ends.  K = 16: the most a band may have."""
    mdl, (numbers, pos, cell, pbc) = _model()
    keep = np.arange(len(numbers)) if N == len(numbers) else np.sort(np.random.default_rng(11).choice(len(numbers), size=N, replace=False))
    images = _band(pos, K, keep=keep)
    numbers = numbers[keep]
    evals = 10
    host = _twin(mdl, numbers, images, cell, pbc, evals=evals, climb=True)
    if K == 1:
        assert all(h["imax"] == 1 for h in host)
    mdl.neb_begin(numbers, images, cell, pbc, FMAX, climb=True)
    sc, E, cov = _device(mdl, (4, 6))
    _same_rows(sc, E, cov, host[:evals])
    assert np.array_equal(mdl.neb_state()["positions"], host[evals]["band"])
    mdl.close()


@pytest.mark.parametrize("reset", [False, True], ids=["resumed", "reset"])
def test_a_covloss_halt_returns_that_band_and_the_run_resumes(reset):
    mdl, (numbers, pos, cell, pbc) = _model()
    images = _band(pos, 3)
    host = _twin(mdl, numbers, images, cell, pbc)
    b = np.array([h["covmax"].max() for h in host])
    later = np.nonzero(b[:EVALS] > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    ediff = 0.5 * (b[:k].max() + b[k])
    if reset:   # the twin that re-initialises its optimizer in front of evaluation k
        host = _twin(mdl, numbers, images, cell, pbc, reset_at=(k,))
    mdl.neb_begin(numbers, images, cell, pbc, FMAX)
    sc1, code = mdl.md_run(EVALS, None, ediff=ediff)
    assert code == 1 and len(sc1) == k + 1, (code, len(sc1), k)
    E1, cov1 = mdl.neb_info()
    _same_rows(sc1[:k], E1[:k], cov1[:k], host[:k])
    assert sc1[k, 11] == b[k] and int(sc1[k, 2]) == host[k]["cimg"]  # the image that carried the largest covloss
    st = mdl.neb_state(results=True)
    assert np.array_equal(st["positions"], host[k]["band"])          # nothing has moved
    assert np.array_equal(st["energy"], host[k]["energies"]) and np.array_equal(st["beta"].max(axis=1), host[k]["covmax"])
    if reset:
        mdl.neb_reset()
    sc2, code = mdl.md_run(EVALS - k, None)
    assert code == 0 and len(sc2) == EVALS - k
    E2, cov2 = mdl.neb_info()
    _same_rows(sc2, E2, cov2, host[k:EVALS])
    assert np.array_equal(mdl.neb_state()["positions"], host[EVALS]["band"])
    mdl.close()


def test_convergence_is_the_third_halt_code():
    """The threshold comes from the twin alone: the first evaluation k in 15..35 whose largest projected force falls below every
    earlier one, and an fmax half-way between that value and the smallest earlier one."""
    mdl, (numbers, pos, cell, pbc) = _model()
    images = _band(pos, 3)
    host = _twin(mdl, numbers, images, cell, pbc, climb=True)
    g = np.sqrt(np.array([h["gmax2"] for h in host]))
    ks = [k for k in range(15, 36) if g[k] < g[:k].min()]
    assert ks, "no evaluation in 15..35 undercuts all earlier ones on this walk: take another seed"
    k = ks[0]
    fmax = 0.5 * (g[k] + g[:k].min())
    twin = _twin(mdl, numbers, images, cell, pbc, fmax=fmax, climb=True)
    assert len(twin) == k + 1 and twin[-1]["converged"]
    mdl.neb_begin(numbers, images, cell, pbc, fmax, climb=True)
    sc, code = mdl.md_run(EVALS, None)
    assert code == 3 and len(sc) == k + 1, (code, len(sc), k)
    E, cov = mdl.neb_info()
    _same_rows(sc, E, cov, twin)
    assert np.array_equal(mdl.neb_state()["positions"], host[k]["band"])
    assert sc[-1, 12] < fmax * fmax and (sc[:-1, 12] >= fmax * fmax).all()
    sc, code = mdl.md_run(5, None)                # asked again, the converged band answers again: nothing moves
    assert code == 3 and len(sc) == 1 and sc[0, 0] == host[k]["energies"][host[k]["imax"] - 1]
    mdl.close()


def test_two_identical_runs_give_the_same_bits():
    mdl, (numbers, pos, cell, pbc) = _model()
    images = _band(pos, 3)
    got = []
    for _ in range(2):
        mdl.neb_begin(numbers, images, cell, pbc, FMAX, climb=True)
        sc, E, cov = _device(mdl, (12,))
        st = mdl.neb_state()
        got.append((sc, E, cov, st["positions"], st["velocities"]))
    for a, c in zip(*got):
        assert np.array_equal(a, c)
    mdl.close()


def test_neb_error_cases_leave_the_handle_working():
    """Every refusal of sgpr_md_neb but one: a run begun on several ranks (SGPR_E_UNSUPPORTED) needs a second process with its
    own device and is not reached here."""
    from autoforce_amd import _lib
    from autoforce_amd._lib import SgprError, f64, ptr
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, MASS
    mdl, (numbers, pos, cell, pbc) = _model()
    N = len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    lib = _lib.load()
    mass = np.array([MASS[int(z)] for z in numbers])
    band3 = f64(_band(pos, 3))

    def neb(K=3, images=band3, fmax=0.05, k=0.1):
        return lib.sgpr_md_neb(mdl.handle, int(K), ptr(f64(images)), float(fmax), float(k), 0, None)

    def begin(**kw):
        mdl.md_begin(numbers, pos, cell, pbc, mass, None, dt=1.0 * FS, friction=0.0, kT=kB * 300.0, **kw)

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    begin()
    assert neb(K=0) == _lib.E_INVALID and neb(K=17, images=_band(pos, 17)) == _lib.E_INVALID   # K < 1, K > 16
    assert neb(fmax=0.0) == _lib.E_INVALID and neb(k=0.0) == _lib.E_INVALID
    far = band3.copy()
    far[2, 7] = far[1, 7] + 0.5 * cell[0]                            # an atom half a cell away from itself in the next image
    assert neb(images=far) == _lib.E_INVALID
    far = band3.copy()
    far[2, 7] = far[1, 7] + 0.4 * (cell[0] + cell[1] + cell[2])      # every fraction below 1/2, longer than half the cell's width
    assert neb(images=far) == _lib.E_INVALID
    works()
    begin(ttime=25.0 * FS)
    assert neb() == _lib.E_INVALID                                   # a thermostat
    from autoforce_amd.npt import GPA
    begin(ttime=25.0 * FS, pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
    assert neb() == _lib.E_INVALID                                   # ... and a barostat
    begin(ml_filter=0.8)
    assert neb() == _lib.E_UNSUPPORTED                               # a filter
    member, _ = _model(seed=2)
    begin()
    mdl.md_committee([member])
    assert neb() == _lib.E_UNSUPPORTED                               # a committee
    mdl.md_committee([])
    works()
    member.close()
    begin()
    mdl.md_record(2)
    assert neb() == _lib.E_UNSUPPORTED                               # an armed frame record
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    assert neb() == _lib.E_UNSUPPORTED                               # a relaxation
    works()
    begin()
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert neb() == _lib.E_INVALID                                   # the run has started
    works()
    with pytest.raises(SgprError):
        mdl.neb_begin(numbers, _band(pos, 17), cell, pbc, 0.05)
    with pytest.raises(RuntimeError, match="no run on this model"):   # a refused band leaves no run behind, and md_run says so
        mdl.md_run(1)
    with pytest.raises(RuntimeError, match="no band on this model"):
        mdl.neb_state()
    with pytest.raises(TypeError):
        mdl.neb_begin(numbers, band3, cell, pbc, 0.05, timestep=0.1)
    mdl.neb_begin(numbers, band3, cell, pbc, 0.05, climb=True)       # and after all that, the real thing runs
    assert lib.sgpr_md_record(mdl.handle, 1, 3) == _lib.E_UNSUPPORTED   # a band records no frames
    assert lib.sgpr_md_state(mdl.handle, None, None, None, None, 0) == _lib.E_INVALID
    assert lib.sgpr_md_relax(mdl.handle, 0.05, None, 0, None) == _lib.E_UNSUPPORTED
    assert lib.sgpr_md_thermostat(mdl.handle, 1, 25.0 * FS, kB * 300.0) == _lib.E_INVALID
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    st = mdl.neb_state(results=True)
    assert st["energy"][int(sc[-1, 1]) - 1] == sc[-1, 0]             # `final`: the current band is the one evaluated last
    assert neb() == _lib.E_INVALID                                   # ... and a band that has started
    works()
    mdl.close()
