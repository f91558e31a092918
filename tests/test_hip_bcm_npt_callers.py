"""GPU: BCMActiveCalculator.run_md(pfactor=..., tdamp_fs=...) — a learning committee with one frozen member under a barostat
— through the device loop (SGPRModel.md_committee on a run begun with a barostat) against the host loop
workloads.npt_moving_cell around calculate() of the same calculator, started from the same state: 12 steps on the 343-atom LiPS
frame with a sampling threshold at which the gate halts the device in the middle and calculate() updates the live model."""
import numpy as np
import pytest

from test_hip_bcm_npt_device import T, TDAMP, _baro, _twin_bounds

pytestmark = pytest.mark.gpu

STEPS = 12
# the sampling thresholds: with these the committee's largest covloss reaches the gate once within the 12 steps (step 9 on an
# MI355X; at ediff = 0.05 twice, at 0.08 never) — the test prints the steps at which the model was updated
KW = dict(ediff=0.06, ediff_tot=0.12, fdiff=0.12, noise_f=0.02)


def _committee():
    """A learning committee: a model seeded from another LiPS frame frozen as member, a fresh live model beside it."""
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator_bcm import BCMActiveCalculator
    from autoforce_amd.workloads import lips
    from helpers import PairTeacher
    numbers, pos, cell, pbc = lips(7, seed=0)
    species = sorted(set(int(z) for z in numbers))
    calc = BCMActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=species), calculator=PairTeacher(rc=4.0), logfile=None, pckl=None,
                               tape=None, **KW)
    n1, p1, c1, b1 = lips(7, seed=1)
    at = Atoms(n1, p1, c1, b1)
    at.calc = calc
    at.get_forces()
    calc.initiate_bcm()
    assert len(calc.model_dict) == 1 and calc.size == (0, 0)
    return calc, (numbers, pos, cell, pbc)


def _run(mode):
    """run_md on the device loop ("device") or, with md_on_device_ok() answering no, on the host loop ("host")."""
    import bcm_md_common as bc
    from autoforce_amd.ase_shim import Atoms
    np.random.seed(1234)
    calc, (numbers, pos, cell, pbc) = _committee()
    vel = bc.thermal_velocities(numbers, temperature=T, seed=4)
    seen = []
    if mode == "host":
        calc.md_on_device_ok = lambda: False
    else:
        eng, attach = calc.engine, calc.engine.md_committee

        def counted(members, **kw):
            seen.append((len(members), bool(eng._md.get("npt")), kw))
            return attach(members, **kw)
        eng.md_committee = counted
    at = Atoms(numbers, pos.copy(), cell, pbc, velocities=vel.copy())
    out = [(st, E, Tk, bool(u)) for st, E, Tk, u, w in calc.run_md(at, STEPS, T, dt_fs=1.0, tdamp_fs=TDAMP, sync_every=4, **_baro())]
    got = (out, at.positions.copy(), np.array(at.cell, float), dict(calc.bcm_weights), seen, calc.size, np.asarray(cell, float))
    for post in calc.model_dict.values():
        post.engine.close()
    calc.engine.close()
    return got


def test_run_md_of_a_committee_with_a_barostat_on_the_device_equals_the_host_loop():
    res = {mode: _run(mode) for mode in ("host", "device")}
    cell = res["host"][6]
    (ho, hp, hc, hw, _, hsize, _), (do, dp, dc, dw, seen, dsize, _) = res["host"], res["device"]
    upd = [o[0] for o in do if o[3]]
    print(f"updates at steps {upd} (host loop: {[o[0] for o in ho if o[3]]}), model size {dsize}, weights {dw}")
    bx, be, bh, bn = _twin_bounds("callers")
    dE = max(abs(a[1] - b[1]) / abs(b[1]) for a, b in zip(do, ho))
    dT = max(abs(a[2] - b[2]) for a, b in zip(do, ho)) / max(b[2] for b in ho)
    dx, dh = np.abs(dp - hp).max(), np.abs(dc - hc).max() / np.abs(hc).max()
    print(f"run_md device against host: max|dE|/|E| {dE:.3e}  max|dT|/max T {dT:.3e}  max|dx| {dx:.3e} A  max|dh|/max|h| {dh:.3e} "
          f"(asserted at {be:.1e}, 1e-9, {bx:.1e}, {bh:.1e})")
    assert [o[0] for o in do] == list(range(STEPS + 1)) == [o[0] for o in ho]
    assert [o[3] for o in do] == [o[3] for o in ho] and dsize == hsize
    assert len(upd) == 1 and 0 < upd[0] < STEPS, upd        # the gate halted the device once, in the middle, and the model was updated
    assert dE <= be and dT <= 1e-9 and dx <= bx and dh <= bh
    assert np.abs(dc - cell).max() > 1e-6                   # the cell has moved
    assert set(dw) == set(hw) and len(dw) == 2 and abs(sum(dw.values()) - 1.0) <= 1e-12
    assert all(abs(dw[k] - hw[k]) <= 1e-9 for k in dw)
    # the run went through md_committee on a run with a barostat: once per run_md call, one member
    assert seen == [(1, True, dict(moving_cell=True))], seen
