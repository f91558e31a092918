"""The callers of metadynamics (tests/test_hip_meta_device.py has the device loop itself, tests/test_meta_twin_cpu.py the
definition): ActiveCalculator(meta=Meta(...)).run_md stays on the device where the collective variables are built in — asserted
through the engine's md_run calls, as the record callers test does —, writes meta.hist with one line per deposit, logs `meta:`
on every step, and leaves the host Meta with the hills the device holds, on-the-fly updates in the middle of the run included; a
Meta with a colvar of the caller's takes the host loop around calculate(), where the bias now acts.  The scenario is
active_common's: a calculator that learns from nothing, so halts occur.  The last test needs no GPU: the host loop around the
CPU oracle."""
import re

import numpy as np
import pytest

import active_common as ac

ENERGY_LINE = re.compile(r"^\S+ \S+ \d+ -?\d+\.\d+(e[-+]\d+)? ")   # date time step energy ...


def _lines(path):
    return [ln for ln in open(path).read().splitlines() if ENERGY_LINE.match(ln)]


def _calc(tmp, engine, meta):
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import PairTeacher
    tmp.mkdir()
    np.random.seed(1234)
    return ActiveCalculator(engine=engine, calculator=PairTeacher(rc=4.0), logfile=str(tmp / "active.log"), pckl=None, tape=None, meta=meta, **ac.KW)


@pytest.mark.gpu
def test_run_md_with_a_built_in_meta_stays_on_the_device(tmp_path):
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    rng0, numbers, pos, cell = ac.start(0)
    steps = 40
    meta = Meta(Catvar(Posvar(1, select=9), Distance(0, 5)), sigma=0.05, w=0.05, hist=str(tmp_path / "meta.hist"))
    calc = _calc(tmp_path / "dev", SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), meta)
    eng, calls = calc.engine, []
    md_run = eng.md_run
    eng.md_run = lambda *a, **k: (calls.append(a[0]), md_run(*a, **k))[1]
    at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
    out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, seed=7, chunk=16))
    assert len(out) == steps + 1 and calc.md_on_device_ok()
    assert calls and sum(calls) >= steps + 1 and len(calls) < steps          # the device loop, in batches
    updates = [o[0] for o in out if o[3]]
    assert updates and calc.size[1] > 2                                       # the gate fired in the middle of the run, the model grew
    # one line of meta.hist per deposit: the configurations 0 ... steps
    hist = open(str(tmp_path / "meta.hist")).read().splitlines()
    assert hist[0] == "# 0.05" and len(hist) == 1 + steps + 1 and all(len(ln.split()) == 4 for ln in hist[1:])
    # the host Meta holds the hills the device holds
    cvd, Vd = eng.md_meta_hills()
    assert len(meta.hills) == steps + 1 and np.array_equal(np.array(meta.hills), cvd)
    np.testing.assert_array_equal(np.loadtxt(str(tmp_path / "meta.hist"), comments="#"), cvd)
    # `meta:` on every step's log line, the device's and calculate()'s
    lines = _lines(str(tmp_path / "dev" / "active.log"))
    assert len(lines) >= steps + 1 and all("meta: " in ln for ln in lines), [ln for ln in lines if "meta: " not in ln][:3]
    assert max(float(ln.split("meta: ")[1]) for ln in lines) > 0
    # a run goes on from a Meta only at a multiple of its pace: the device counts the run's configurations from 0
    meta.pace, n_hills = 2, len(meta.hills)
    assert meta.n == steps + 1 and meta.n % 2 == 1
    with pytest.raises(ValueError, match="pace"):
        list(calc.run_md(at, 2, 300.0, dt_fs=1.0, friction=0.02, seed=7))
    meta.n += 1
    out = list(calc.run_md(at, 4, 300.0, dt_fs=1.0, friction=0.02, seed=7))
    assert len(out) == 5 and len(meta.hills) == n_hills + 3           # configurations 0, 2, 4 of this run
    eng.close()


@pytest.mark.gpu
def test_a_colvar_of_the_callers_takes_the_host_loop_and_the_bias_acts(tmp_path):
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Meta
    rng0, numbers, pos, cell = ac.start(0)
    meta = Meta(lambda numbers, xyz, cell, pbc, nl: (xyz[5] - xyz[0]).norm().view(1), sigma=0.05, w=0.05, hist=str(tmp_path / "meta.hist"))
    assert meta.device_spec() is None
    calc = _calc(tmp_path / "host", SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), meta)
    eng, calls = calc.engine, []
    md_run = eng.md_run
    eng.md_run = lambda *a, **k: (calls.append(a[0]), md_run(*a, **k))[1]
    at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
    steps = 12
    out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, seed=7))
    assert len(out) == steps + 1 and not calls and not calc.md_on_device_ok()
    assert len(meta.hills) == steps + 1 and len(open(str(tmp_path / "meta.hist")).read().splitlines()) == steps + 2
    # calculate() at the last configuration: the forces are the model's plus Meta.bias
    calc._calc = None
    calc.results = {}
    calc.calculate(Atoms(numbers, at.positions, cell, True))
    V, Fb, Sb = meta.bias(at.positions, cell, numbers)
    plain = eng.predict(numbers, at.positions, cell, [True] * 3)
    assert V > 0 and np.abs(Fb).max() > 0
    assert np.abs(calc.results["forces"] - (plain["forces"] + Fb)).max() <= 1e-13 * np.abs(plain["forces"]).max()
    assert abs(float(calc.results["energy"]) - (plain["energy"] + V)) <= 1e-13 * max(1.0, abs(plain["energy"]))
    assert np.abs(calc.results["stress"] - (plain["stress"] + Sb)).max() <= 1e-13 * max(np.abs(plain["stress"]).max(), np.abs(Sb).max())
    eng.close()


def test_host_loop_around_the_oracle_deposits_per_step_and_the_bias_acts(tmp_path):
    """Without a device engine run_md is the host loop around calculate(): the Meta's bias is in every result, update() runs
    once per configuration (the reference's dyn.attach(meta.update)), meta.hist and the log follow."""
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Distance, Meta
    from helpers import OracleModel
    rng0, numbers, pos, cell = ac.start(0)
    meta = Meta(Distance(0, 5), sigma=0.05, w=0.05, hist=str(tmp_path / "meta.hist"))
    calc = _calc(tmp_path / "cpu", OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), meta)
    assert not calc.md_on_device_ok() and calc._meta_spec() is None
    at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
    steps = 5
    out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, seed=7))
    assert len(out) == steps + 1 and len(meta.hills) == steps + 1
    hist = open(str(tmp_path / "meta.hist")).read().splitlines()
    assert hist[0] == "# 0.05" and len(hist) == steps + 2
    np.testing.assert_array_equal(np.loadtxt(str(tmp_path / "meta.hist"), comments="#"), np.array(meta.hills)[:, 0])
    lines = _lines(str(tmp_path / "cpu" / "active.log"))
    assert len(lines) >= steps + 1 and all("meta: " in ln for ln in lines)
    assert max(float(ln.split("meta: ")[1]) for ln in lines) > 0             # behind the first deposit the bias is there
    assert out[-1][1] == float(calc.results["energy"])
