"""GPU tests of the filter of model-update jumps inside the device MD loop (sgpr_md_filter: the reference's FilterDeltas,
calculator/active.py:47-76, by evaluation index): finalize_next_kernel<5>, <6>, <7> and md_npt_kernel's stress accumulator
against the host twins with ml_filter= around the same library — BAOAB Langevin with uploaded and with on-device deviates,
velocity Verlet, Nose-Hoover, held components, the moving cell with and without `iso`.  The jumps are synthetic deltas pushed
between md_run calls at configurations 7 and 8 (forces of order 0.3 eV/A with a handful at +-5, so both clamps act; stress of
order 1e-3 eV/A^3); the twin runs around a calculator that publishes the same `deltas` at the same configurations.
  Bit for bit: the energy and the largest covloss of every evaluation, zeta and its integral, cells and strain rates, the
final positions and velocities, and the accumulators md_filter_state returns — however the run is cut into calls.  The rows'
kinetic terms are sums over the atoms in the device's order and are held, as everywhere in test_hip_fixed_device.py, to
rtol = 1e-12 against the twin's temperature; against the other cut of the same run rows [:, :14] are compared bit for bit.
  Also: what the run reports stays the model's (md_state, a recorded frame); a filter that is never pushed is the run without
one; a covloss halt leaves the accumulators of the halted configuration as they were, and the resume behind a push is the
twin's; ActiveCalculator.run_md(ml_filter=0.8) with a teacher against the twin around calculate(); the error cases.
Frame, model and helpers are those of test_hip_npt_device.py and test_hip_fixed_device.py."""
import numpy as np
import pytest

from test_hip_fixed_device import _Rows, _active, _begin, _mask, _setup
from test_hip_npt_device import _PredictCalc
from test_hip_npt_device import _begin as _begin_npt, _setup as _setup_npt

pytestmark = pytest.mark.gpu

STEPS, T, FRICTION, TDAMP, SHRINK = 60, 600.0, 0.05, 20.0, 0.8
CUTS_A, CUTS_B = (7, 1, 53), (7, 1, 20, 33)     # 61 evaluations, the last call `final`; both end calls in front of 7 and 8


def _deltas(N, at=(7, 8), seed=11):
    rng = np.random.default_rng(seed)
    out = {}
    for n in at:
        dF = 0.3 * rng.normal(size=(N, 3))
        idx = rng.permutation(N)[:6]
        dF[idx[:3], rng.integers(0, 3, 3)] = 5.0
        dF[idx[3:], rng.integers(0, 3, 3)] = -5.0
        out[n] = (dF, 1e-3 * rng.normal(size=6))
    return out


class _PushCalc(_PredictCalc):
    """_PredictCalc that publishes given `deltas` at given configurations (counted by evaluations), None elsewhere."""

    def __init__(self, mdl, pushes):
        super().__init__(mdl)
        self.pushes, self.deltas = pushes, None

    def get_property(self, name, atoms=None):
        before = self.calls
        out = super().get_property(name, atoms)
        if self.calls != before:
            d = self.pushes.get(self.calls - 1)
            self.deltas = None if d is None else dict(energy=0.0, forces=d[0], stress=d[1])
        return out


def _run(mdl, cuts, pushes, noise=None, steps=STEPS, npt=False):
    """The run in calls of `cuts` evaluations; the jump of configuration n is pushed in front of the call that begins with n."""
    rows, cells, etas = [], [], []
    for n in cuts:
        if len(rows) in pushes:
            mdl.md_filter_push(*pushes[len(rows)])
        xi = None if noise is None else noise[len(rows):len(rows) + n]
        if xi is not None and len(xi) < n:   # (the last, `final` evaluation moves nothing)
            xi = np.concatenate([xi, np.zeros((n - len(xi),) + xi.shape[1:])])
        sc, code = mdl.md_run(n, xi, final=(len(rows) + n == steps + 1))
        assert code == 0 and len(sc) == n, (code, len(sc), n)
        rows.extend(sc)
        if npt:
            c, e = mdl.md_cells()
            cells.extend(c)
            etas.extend(e)
    assert all(k in np.cumsum((0,) + tuple(cuts)) for k in pushes)
    return (np.array(rows), np.array(cells), np.array(etas)) if npt else np.array(rows)


@pytest.mark.parametrize("how", ["uploaded", "on-device", "verlet", "nose-hoover", "uploaded-held", "nose-hoover-held"])
def test_constant_cell_loops_with_pushes_are_the_twin_bit_for_bit(how):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS, langevin_nvt, nose_hoover_nvt
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    held = how.endswith("-held")
    how = how.replace("-held", "")
    hold = dict(fixed=fx) if held else {}
    g = 3 * N - (int(fx.sum()) if held else 0)
    nh = how == "nose-hoover"
    friction = 0.0 if how in ("verlet", "nose-hoover") else FRICTION
    pushes = _deltas(N)
    out = {}
    for cuts in (CUTS_A, CUTS_B):
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=friction, seed=77 if how == "on-device" else 0,
               ttime=TDAMP * FS if nh else None, ml_filter=SHRINK, **hold)
        if how == "uploaded":
            xi = np.random.default_rng(9).normal(size=(STEPS, N, 3))
            sc = _run(mdl, cuts, pushes, noise=xi)
        else:
            sc = _run(mdl, cuts, pushes)
            xi = mdl.md_deviates(0, STEPS) if how == "on-device" else np.zeros((STEPS, N, 3))
        st = mdl.md_state(results=True)
        f, s = mdl.md_filter_state()
        out[cuts] = (sc[:, :14], sc[:, 14:] if nh else sc[:, :0], st["positions"], st["velocities"], f, s)
        # what the run reports stays the model's own
        assert np.array_equal(st["forces"], mdl.predict(numbers, st["positions"], cell, pbc)["forces"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)                                   # however the run is cut into calls
    calc = _PushCalc(mdl, pushes)
    if nh:
        host = [(E, Tk, p.copy(), v.copy(), acc, z, zi) for _, E, Tk, _, p, v, z, zi, acc in
                nose_hoover_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=1.0, tdamp_fs=TDAMP, vel=vel, ml_filter=SHRINK, **hold)]
    else:
        host = [(E, Tk, p.copy(), v.copy(), acc) for _, E, Tk, _, p, v, acc in
                langevin_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=1.0, friction=friction, vel=vel, rng=_Rows(xi),
                             ml_filter=SHRINK, **hold)]
    sc, zz, x, v, f, s = out[CUTS_B]
    assert [r[0] for r in sc] == [h[0] for h in host]                 # energies: same positions, every evaluation
    assert np.array_equal(sc[:, 11], np.array(calc.betas))
    np.testing.assert_allclose(sc[:, 12] / (g * kB), [h[1] for h in host], rtol=1e-12)   # (the sum over atoms runs in another order)
    if nh:
        assert np.array_equal(zz[:, 0], np.array([h[5] for h in host])) and np.array_equal(zz[:, 1], np.array([h[6] for h in host]))
        assert np.abs(zz[:, 0]).max() > 0
    assert np.array_equal(x, host[-1][2]) and np.array_equal(v, host[-1][3])
    assert np.array_equal(f, host[-1][4][0]) and np.array_equal(s, host[-1][4][1])
    assert np.abs(f).max() > 0 and not s.any()
    # both clamps acted on the way: the accumulators configuration 8 found
    f8 = host[8][4][0]
    assert f8.max() > 1.0 and f8.min() < -1.0
    if held:
        assert np.array_equal(x[fx], pos[fx]) and np.array_equal(v[fx], np.zeros(fx.sum()))
        assert np.abs(f[fx]).max() > 0
    # ... and the walk is not the unfiltered one
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=friction, seed=77 if how == "on-device" else 0,
           ttime=TDAMP * FS if nh else None, **hold)
    sc0, code = mdl.md_run(STEPS + 1, np.concatenate([xi, np.zeros((1, N, 3))]) if how == "uploaded" else None, final=True)
    assert code == 0 and np.array_equal(sc0[:8, 0], sc[:8, 0]) and not np.array_equal(sc0[9:, 0], sc[9:, 0])
    mdl.close()


@pytest.mark.parametrize("iso", [False, True], ids=["full", "iso"])
def test_moving_cell_with_force_and_stress_pushes_is_the_twin_bit_for_bit(iso):
    from autoforce_amd.workloads import npt_moving_cell
    mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup_npt()
    N = len(numbers)
    pushes = _deltas(N)
    calc = _PushCalc(mdl, pushes)
    host = [(s, E, Tk, p.copy(), v.copy(), h.copy(), e.copy(), z, zi, acc) for s, E, Tk, w, p, v, h, e, z, zi, acc in
            npt_moving_cell(calc, numbers, pos, cell, pbc, STEPS, temperature=600.0, dt_fs=1.0, tdamp_fs=25.0, vel=vel, iso=iso, ml_filter=SHRINK,
                            **baro)]
    out = {}
    for cuts in (CUTS_A, CUTS_B):
        _begin_npt(mdl, numbers, pos, cell, pbc, mass, vel, baro, iso=iso, ml_filter=SHRINK)
        sc, cells, etas = _run(mdl, cuts, pushes, npt=True)
        st = mdl.md_state(results=True)
        f, s = mdl.md_filter_state()
        out[cuts] = (sc, cells, etas, st["positions"], st["velocities"], st["cell"], f, s)
        assert np.array_equal(st["forces"], mdl.predict(numbers, st["positions"], st["cell"], pbc)["forces"])
    for a, c in zip(*out.values()):
        assert np.array_equal(a, c)
    sc, cells, etas, x, v, h, f, s = out[CUTS_B]
    # (the standard of test_hip_npt_device.py)
    assert [r[0] for r in sc] == [hh[1] for hh in host]
    assert np.array_equal(sc[:, 11], np.array(calc.betas))
    assert np.array_equal(sc[:, 14], np.array([hh[7] for hh in host]))
    assert np.array_equal(sc[:, 15], np.array([hh[8] for hh in host]))
    assert np.array_equal(cells, np.array([hh[5] for hh in host]))
    assert np.array_equal(etas, np.array([hh[6] for hh in host]))
    assert np.array_equal(x, host[-1][3]) and np.array_equal(v, host[-1][4]) and np.array_equal(h, host[-1][5])
    assert np.array_equal(f, host[-1][9][0]) and np.array_equal(s, host[-1][9][1])
    assert np.abs(f).max() > 0 and np.abs(s).min() > 0
    # the stress accumulator alone moves the cell: the same run with the force jumps only
    _begin_npt(mdl, numbers, pos, cell, pbc, mass, vel, baro, iso=iso, ml_filter=SHRINK)
    sc1, cells1, etas1 = _run(mdl, CUTS_A, {k: (d[0], None) for k, d in pushes.items()}, npt=True)
    assert np.array_equal(cells1[:8], cells[:8]) and not np.array_equal(cells1[12:], cells[12:])
    mdl.close()


def test_reported_results_stay_the_models_own():
    """After pushes the forces of md_state and of a recorded frame are predict's at those positions, bit for bit, while the
    closing half kick — what the integrator used — is the filtered force's."""
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    pushes = _deltas(N)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=FRICTION, seed=5, ml_filter=SHRINK)
    mdl.md_record(1, velocities=True, results=True)
    _run(mdl, (7, 1, 4), pushes, steps=11)
    fr = mdl.md_frames()
    assert len(fr["index"]) >= 2 and fr["index"][-1] == 11 and "velocities" not in fr
    for k in range(len(fr["index"])):
        assert np.array_equal(fr["forces"][k], mdl.predict(numbers, fr["positions"][k], cell, pbc)["forces"])
    st = mdl.md_state(results=True)
    F = mdl.predict(numbers, st["positions"], cell, pbc)["forces"]
    assert np.array_equal(st["forces"], F) and np.array_equal(fr["forces"][-1], F)
    f, _ = mdl.md_filter_state()
    seen = F - np.clip(f * SHRINK, -1.0, 1.0)
    assert np.abs(np.clip(f * SHRINK, -1.0, 1.0)).max() == 1.0                    # a clamped component among them
    hdt = 0.5 * FS
    assert np.array_equal(st["velocities"], st["velocities_pre"] + hdt * seen / mass[:, None])
    assert not np.array_equal(st["velocities"], st["velocities_pre"] + hdt * F / mass[:, None])
    mdl.close()


def test_a_filter_that_is_never_pushed_is_the_run_without_one():
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    xi = np.random.default_rng(9).normal(size=(21, N, 3))
    kinds = [dict(noise=True), dict(seed=5), dict(friction=0.0), dict(friction=0.0, ttime=TDAMP * FS), dict(friction=0.0, ttime=TDAMP * FS, fixed=fx)]
    for kw in kinds:
        kw = dict(kw)
        noise = xi if kw.pop("noise", False) else None
        got = []
        for filt in (dict(), dict(ml_filter=SHRINK), dict(ml_filter=SHRINK, filter_init=(np.zeros((N, 3)), np.zeros(6)))):
            _begin(mdl, numbers, pos, cell, pbc, mass, vel, **kw, **filt)
            sc = np.concatenate([mdl.md_run(5, None if noise is None else noise[:5])[0],
                                 mdl.md_run(16, None if noise is None else noise[5:], final=True)[0]])
            st = mdl.md_state(results=True)
            got.append((sc, st["positions"], st["velocities"]))
            if filt:
                f, s = mdl.md_filter_state()
                assert not f.any() and not s.any()
        for other in got[1:]:
            for a, c in zip(got[0], other):
                assert np.array_equal(a, c)
    mdl.close()
    mdl, numbers, pos, cell, pbc, mass, vel, baro = _setup_npt()
    got = []
    for filt in (dict(), dict(ml_filter=SHRINK)):
        _begin_npt(mdl, numbers, pos, cell, pbc, mass, vel, baro, **filt)
        sc, cells, etas = _run(mdl, (5, 16), {}, steps=20, npt=True)
        st = mdl.md_state(results=True)
        got.append((sc, cells, etas, st["positions"], st["velocities"]))
    for a, c in zip(*got):
        assert np.array_equal(a, c)
    mdl.close()


def test_a_halt_leaves_the_accumulators_and_the_resume_behind_a_push_is_the_twin():
    from autoforce_amd.workloads import FS, nose_hoover_nvt
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    early = _deltas(N, at=(2,))

    def twin(pushes):
        calc = _PushCalc(mdl, pushes)
        rows = [(E, p.copy(), v.copy(), z, zi, acc) for _, E, _, _, p, v, z, zi, acc in
                nose_hoover_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=1.0, tdamp_fs=TDAMP, vel=vel, ml_filter=SHRINK)]
        return rows, np.array(calc.betas)

    # (ediff as test_hip_fixed_device.py chooses it; the jump of configuration k acts behind k only, so k is found without it)
    host0, b = twin(early)
    later = np.nonzero(b > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    assert k > 2
    ediff = 0.5 * (b[:k].max() + b[k])
    pushes = dict(early)
    pushes[k] = _deltas(N, at=(k,), seed=12)[k]
    host, b2 = twin(pushes)
    assert np.array_equal(b2[:k + 1], b[:k + 1])
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=TDAMP * FS, ml_filter=SHRINK)
    sc0, code = mdl.md_run(2, None, ediff=ediff)
    assert code == 0 and len(sc0) == 2
    mdl.md_filter_push(*pushes[2])
    sc1, code = mdl.md_run(STEPS + 1 - 2, None, ediff=ediff, final=True)
    assert code == 1 and len(sc1) == k + 1 - 2
    sth = mdl.md_state(results=True)
    # (the halted evaluation knew nothing of the jump that calculate() is about to publish: its centred velocity is that of the
    # twin without the jump at k; the repeated evaluation behind the push gives the twin's with it)
    assert np.array_equal(sth["positions"], host[k][1]) and np.array_equal(sth["velocities"], host0[k][2])
    assert not np.array_equal(host0[k][2], host[k][2])
    f, s = mdl.md_filter_state()
    assert np.array_equal(f, host[k][5][0]) and np.abs(f).max() > 0   # as configuration k found them: the discarded evaluation shrank nothing
    mdl.md_filter_push(*pushes[k])
    sc2, code = mdl.md_run(STEPS + 1 - k, None, ediff=0.0, final=True)
    assert code == 0 and [r[0] for r in sc2] == [h[0] for h in host[k:]]
    assert np.array_equal(sc2[:, 14], np.array([h[3] for h in host[k:]])) and np.array_equal(sc2[:, 15], np.array([h[4] for h in host[k:]]))
    st2 = mdl.md_state(results=True)
    assert np.array_equal(st2["positions"], host[-1][1]) and np.array_equal(st2["velocities"], host[-1][2])
    f2, _ = mdl.md_filter_state()
    assert np.array_equal(f2, host[-1][5][0])
    mdl.close()


def test_run_md_with_a_filter_equals_the_twin_around_calculate(tmp_path):
    """ActiveCalculator.run_md(ml_filter=0.8) with a teacher — the gate fires behind step 0, calculate() updates the model and
    publishes deltas, run_md pushes them — against workloads.langevin_nvt(ml_filter=0.8) around calculate() of the same
    calculator class, compared as test_hip_fixed_device.py compares run_md on constrained atoms with its twin."""
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.workloads import FilterState, langevin_nvt
    steps = 50
    res = {}
    for mode in ("host", "device", "plain"):
        calc, numbers, pos, cell, log = _active(tmp_path, mode)
        vel = 0.02 * np.random.default_rng(3).normal(size=pos.shape)
        if mode == "host":
            out, jumps = [], []
            for st, E, Tk, _, p, v, acc in langevin_nvt(calc, numbers, pos, cell, True, steps, 300.0, 1.0, 0.02, vel=vel, rng=np.random.default_rng(9),
                                                        ml_filter=0.8):
                out.append((st, E, Tk, bool(calc.updated)))
                if calc.deltas:
                    jumps.append(st)
                last = (p.copy(), v.copy(), acc)
            res[mode] = (out, last, calc.size, jumps)
        else:
            at = Atoms(numbers, pos, cell, True, velocities=vel)
            flt = FilterState(0.8) if mode == "device" else None
            out = [(s, E, Tk, bool(u)) for s, E, Tk, u, w in
                   calc.run_md(at, steps, 300.0, dt_fs=1.0, chunk=16, friction=0.02, rng=np.random.default_rng(9), ml_filter=flt)]
            if mode == "device":
                assert calc.engine._md.get("shrink") == 0.8                # the device loop has run, with the filter
                assert flt.pushes >= 1
            res[mode] = (out, (at.positions.copy(), at.get_velocities(), None if flt is None else (flt.f, flt.s)), calc.size,
                         None if flt is None else flt.pushes)
        calc.engine.close()
    (ho, hl, hs, jumps), (do, dl, ds, pushes), (po, pl, ps, _) = res["host"], res["device"], res["plain"]
    assert len(jumps) >= 1 and min(jumps) > 0 and pushes == len(jumps)     # an update at a step > 0 published deltas, each was pushed
    assert hs == ds and hs[1] > 2, (hs, ds)
    assert [o[0] for o in ho] == [o[0] for o in do] and [o[3] for o in ho] == [o[3] for o in do]
    assert [o[1] for o in ho] == [o[1] for o in do]
    np.testing.assert_allclose([o[2] for o in do], [o[2] for o in ho], rtol=1e-12)
    assert np.array_equal(hl[0], dl[0]) and np.array_equal(hl[1], dl[1])
    assert np.array_equal(hl[2][0], dl[2][0]) and np.abs(dl[2][0]).max() > 0
    # without the filter the trajectory is another one behind the first jump, the same one up to it
    j = min(jumps)
    assert [o[1] for o in po[:j + 1]] == [o[1] for o in do[:j + 1]]
    assert [o[1] for o in po[j + 2:]] != [o[1] for o in do[j + 2:]]


def test_the_scatter_form_refuses_the_filter_inside_the_step_and_the_handle_runs_on():
    """The filter has no check in front of the run: with option reverse_scatter set, the step itself refuses it (behind its
    reverse pass, before the last kernel).  Back in the gather form the same run, begun again, gives the rows of a handle that
    never saw the option, bit for bit."""
    from autoforce_amd import _lib
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    lib = _lib.load()
    kw = dict(friction=FRICTION, seed=5, ml_filter=SHRINK)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, **kw)
    _lib.check(lib.sgpr_set_option(mdl.handle, b"reverse_scatter", 1))
    with pytest.raises(_lib.SgprError) as e:
        mdl.md_run(3)
    assert e.value.code == _lib.E_UNSUPPORTED and "gather form of the fused last kernel only" in str(e.value), str(e.value)
    _lib.check(lib.sgpr_set_option(mdl.handle, b"reverse_scatter", 0))
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, **kw)
    sc, code = mdl.md_run(3)
    assert code == 0 and len(sc) == 3
    fresh = _setup()[0]
    _begin(fresh, numbers, pos, cell, pbc, mass, vel, **kw)
    ref, code = fresh.md_run(3)
    assert code == 0 and len(ref) == 3 and np.array_equal(sc, ref)
    fresh.close()
    mdl.close()


def test_error_cases_leave_the_handle_working():
    from autoforce_amd import _lib
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc, mass, vel, fx = _setup()
    N = len(numbers)
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    lib = _lib.load()
    dF = np.zeros((N, 3))

    def works():
        assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0

    _begin(mdl, numbers, pos, cell, pbc, mass, vel)
    for bad in (0.0, 1.0, -0.2, 1.7, float("nan")):
        assert lib.sgpr_md_filter(mdl.handle, bad, None, None) == _lib.E_INVALID       # shrink outside (0, 1)
    assert lib.sgpr_md_filter_push(mdl.handle, _lib.ptr(dF), None) == _lib.E_INVALID   # a push without a filter
    assert lib.sgpr_md_filter_state(mdl.handle, _lib.ptr(dF), None) == _lib.E_INVALID
    works()
    _begin(mdl, numbers, pos, cell, pbc, mass, vel)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    assert lib.sgpr_md_filter(mdl.handle, SHRINK, None, None) == _lib.E_INVALID        # the run has started
    works()
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    assert lib.sgpr_md_filter(mdl.handle, SHRINK, None, None) == _lib.E_UNSUPPORTED    # a relaxation
    works()
    other, _ = __import__("test_hip_npt_device")._model(seed=2)
    _begin(mdl, numbers, pos, cell, pbc, mass, vel)
    mdl.md_committee([other])
    assert lib.sgpr_md_filter(mdl.handle, SHRINK, None, None) == _lib.E_UNSUPPORTED    # a committee
    works()
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, ml_filter=SHRINK)
    with pytest.raises(_lib.SgprError):
        mdl.md_committee([other])                                                        # ... and a committee behind a filter
    assert lib.sgpr_md_relax(mdl.handle, 0.05, None, 0, None) == _lib.E_UNSUPPORTED    # a relaxation behind a filter
    works()
    with pytest.raises(_lib.SgprError):
        _begin(mdl, numbers, pos, cell, pbc, mass, vel, ml_filter=1.0)                   # as the Python surface reports it
    works()
    _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, ttime=TDAMP * FS, ml_filter=SHRINK)   # and after all that, the real thing runs
    mdl.md_filter_push(dF + 0.1)
    sc, code = mdl.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    other.close()
    mdl.close()
