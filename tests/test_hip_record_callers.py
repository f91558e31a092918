"""GPU tests of the callers of the frame record (tests/test_hip_record_device.py has the record itself):
ActiveCalculator.run_md(sync_every=k) no longer cuts its batches at the multiples of k — what a caller observes is what the
cutting path (record=False, the code before the record) shows, with fewer md_run calls —, and
ActiveCalculator.run_relax(on_frame=) / cl.relax.relax(algo="FIRE", trajectory=) report every evaluation of a relaxation
that stays on the device.  The scenario is active_common's: a calculator that learns from nothing, so halts occur."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _log(path):
    return [re.sub(r"^\S+ \S+ ", "", ln) for ln in open(path).read().splitlines()]


def _run_md_legs(tmp, record, kind, k, steps=(24, 48)):
    """Two legs of run_md around one calculator: an active one (the gate fires, the model grows), then the same calculator
    without its teacher (evaluate only).  Returns per leg: the yields (wall time aside) with self.step, what the atoms show at
    the yields a caller may look at, the final atoms, the md_run calls made; and the log."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    from helpers import PairTeacher
    np.random.seed(1234)
    rng0, numbers, pos, cell = ac.start(0)
    tmp.mkdir()
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                            logfile=str(tmp / "active.log"), pckl=None, tape=None, **ac.KW)
    kw = (dict(tdamp_fs=20.0, pfactor=(75.0 * FS) ** 2 * 40.0 * GPA, externalstress=1.0 * GPA) if kind == "npt" else
          dict(friction=0.02, seed=7))
    vel = 0.02 * np.random.default_rng(3).normal(size=pos.shape)
    eng, calls = calc.engine, []
    md_run = eng.md_run
    eng.md_run = lambda *a, **kwa: (calls.append(a[0]), md_run(*a, **kwa))[1]
    legs = []
    for leg, n in enumerate(steps):
        if leg == 1:
            calc._calc = None                      # evaluate only: the gate never fires
            assert not calc.active
        at = Atoms(numbers, pos, cell, True, velocities=vel)
        out, seen, n0 = [], {}, len(calls)
        for st, E, Tk, u, w in calc.run_md(at, n, 300.0, dt_fs=1.0, chunk=16, sync_every=k, record=record, **kw):
            out.append((st, E, Tk, bool(u), calc.step if st % k == 0 else None))
            if st % k == 0 or u:                   # a multiple of k, or behind an update: the atoms are that configuration
                seen[st] = (at.positions.copy(), at.get_velocities().copy(), np.array(at.cell, float))
        last = (at.positions.copy(), at.get_velocities().copy(), np.array(at.cell, float), calc.step)
        assert len(out) == n + 1
        legs.append((out, seen, last, calc.size, len(calls) - n0))
        pos, vel, cell = last[0] + 0.01, last[1], last[2]
    log = _log(tmp / "active.log")
    assert (eng._md.get("record") is not None) == record
    eng.close()
    return legs, log


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("kind", ["langevin", "npt"])
def test_run_md_records_instead_of_cutting(tmp_path, kind, k):
    (cut, cut_log), (rec, rec_log) = (_run_md_legs(tmp_path / mode, mode == "rec", kind, k) for mode in ("cut", "rec"))
    assert rec_log == cut_log                                            # the log files, line by line
    for leg, ((co, cs, cl, csize, ccalls), (ro, rs, rl, rsize, rcalls)) in enumerate(zip(cut, rec)):
        assert ro == co                                                  # every yielded tuple (and self.step at the multiples of k)
        assert rsize == csize
        assert sorted(rs) == sorted(cs) and len(rs) >= len(co) // k
        for st in cs:
            for a, b in zip(cs[st], rs[st]):
                assert np.array_equal(a, b), (leg, st)
        for a, b in zip(cl, rl):
            assert np.array_equal(a, b), leg
        print(f"leg {leg}: md_run calls cut {ccalls} recorded {rcalls}")
        assert rcalls <= ccalls
    upd = [o[0] for o in rec[0][0] if o[3]]
    assert len(upd) >= 1 and rec[0][3][1] > 2, upd                       # first leg: the gate fired and the model grew
    assert not any(o[3] for o in rec[1][0])                              # second leg: nothing halts the device
    assert rec[1][4] < cut[1][4]                                         # fewer calls
    if k == 1:
        assert cut[1][4] >= 48 and rec[1][4] < 24, (cut[1][4], rec[1][4])    # 48 steps: one call per step before, now batches


def test_run_relax_reports_every_evaluation(tmp_path):
    """run_relax(on_frame=) against the host loop (workloads.fire_relax around calculate()) of the same calculator class, an
    active calculator that learns from nothing: every evaluation is reported once, in order, with the host loop's positions,
    cell and energy — an evaluation handed to calculate() with the results of its re-evaluation; with interval = 3 the
    multiples of three and the final structure."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.workloads import PairTeacher, fire_relax
    steps, fmax = 40, 1e-3
    res = {}
    for mode in ("host", "device", "device-3"):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        teacher = PairTeacher(ac.SPECIES, rc=4.0)
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=teacher, logfile=None, pckl=None, tape=None, **ac.KW)
        got = []
        if mode == "host":
            for o in fire_relax(calc, numbers, pos, cell, True, steps, fmax, cell_relax=True, species=calc.engine.species):
                got.append((o["n"], o["positions"].copy(), o["cell"].copy(), float(o["energy"])))
            n_eval = o["n"] + 1
        else:
            at = Atoms(numbers, pos, cell, True)
            out = calc.run_relax(at, fmax=fmax, steps=steps, cell=True, chunk=16, interval=3 if mode == "device-3" else 1,
                                 on_frame=lambda n, fr: got.append((n, fr["positions"].copy(), np.array(fr["cell"], float), fr["energy"], fr["forces"].copy())))
            assert calc.engine._md.get("relax") and calc.engine._md.get("record")
            n_eval = out["evaluations"]
            assert np.array_equal(got[-1][1], at.positions) and got[-1][3] == float(calc.results["energy"])
            assert np.array_equal(got[-1][4], calc.results["forces"])
        res[mode] = (got, n_eval, teacher.calls)
        calc.engine.close()
    (hg, hn, hcalls), (dg, dn, dcalls), (tg, tn, tcalls) = res["host"], res["device"], res["device-3"]
    assert hn == dn == tn and hcalls == dcalls == tcalls and dcalls >= 1
    assert [g[0] for g in dg] == list(range(dn)) == [g[0] for g in hg]       # every evaluation, once, in order
    for h, d in zip(hg, dg):
        assert np.array_equal(h[1], d[1]) and np.array_equal(h[2], d[2]) and h[3] == d[3], h[0]
    want = sorted(set(range(0, dn, 3)) | {dn - 1})
    assert [g[0] for g in tg] == want
    for g in tg:
        assert np.array_equal(g[1], dg[g[0]][1]) and np.array_equal(g[2], dg[g[0]][2]) and g[3] == dg[g[0]][3]


def test_relaxation_driver_writes_a_frame_per_evaluation(tmp_path, monkeypatch):
    """cl.relax.relax(algo="FIRE", trajectory=...) on the device: relax.xyz holds one frame per evaluation of every run_relax
    the driver made, the last one the final structure."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from autoforce_amd.cl.relax import relax
    from autoforce_amd.sgprio import parse_extxyz
    from helpers import PairTeacher
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    rng0, numbers, pos, cell = ac.start(0)
    calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0), logfile=None, pckl=None,
                            tape=None, **ac.KW)
    evals = []
    run_relax = calc.run_relax
    calc.run_relax = lambda *a, **k: (lambda r: (evals.append(r["evaluations"]), r)[1])(run_relax(*a, **k))
    atoms = Atoms(numbers, pos, cell, True)
    relax(atoms, fmax=0.1, cell=True, algo="FIRE", trajectory="relax.xyz", rattle=0.02, calc=calc, seed=5, confirm=False)
    assert evals and sum(evals) > 1 and calc.engine._md.get("relax")
    assert open("relax.xyz").read().count("Lattice=") == sum(evals)
    last = parse_extxyz(open("relax.xyz").read().splitlines()[-(len(numbers) + 2):])
    assert np.allclose(last.positions, atoms.positions, rtol=0, atol=1e-7) and abs(last.energy - float(calc.results["energy"])) < 1e-7
    calc.engine.close()
