"""The callers of the Q_l colvar (tests/test_hip_qlvar_device.py has the device loop itself, tests/test_qlvar_twin_cpu.py the
definition): ActiveCalculator(meta=Meta(Qlvar(...))).run_md attaches the Meta to the device loop — asserted through the engine's
md_run calls —, resolves Qlvar(index=None) to the first atom of its species, writes meta.hist with one line per deposit and leaves
the host Meta with the hills the device holds; calculate() at the end adds the bias of the twin, which is the bias of the last
device row.  The scenario is active_common's: a calculator that learns from nothing, so halts and host evaluations occur."""
import numpy as np
import pytest

import active_common as ac
from test_hip_meta_callers import _calc, _lines

pytestmark = pytest.mark.gpu


def test_run_md_attaches_a_meta_over_a_qlvar_and_calculate_adds_the_same_bias(tmp_path):
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Meta, Qlvar
    rng0, numbers, pos, cell = ac.start(0)
    steps = 40
    var = Qlvar(3, 3, cutoff=4.5, l=[4, 6])                                   # the first Li over the Li of its own layer: four at 3.0 A, four at 4.2
    meta = Meta(var, sigma=0.01, w=0.05, hist=str(tmp_path / "meta.hist"))
    assert meta.device_spec() == [("qlvar", None, 3, 4.5, (4, 6))]
    calc = _calc(tmp_path / "dev", SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), meta)
    eng, calls = calc.engine, []
    md_run = eng.md_run
    eng.md_run = lambda *a, **k: (calls.append(a[0]), md_run(*a, **k))[1]
    at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
    out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, seed=7, chunk=16))
    assert len(out) == steps + 1 and calc.md_on_device_ok()
    assert calls and sum(calls) >= steps + 1 and len(calls) < steps          # the device loop, in batches
    assert var.index == 0 and calc._meta_spec() == [("qlvar", 0, 3, 4.5, (4, 6))] and meta.rc == 4.5
    assert eng.md_meta_info()["D"] == 2
    # one line of meta.hist per deposit, and the host Meta holds the hills the device holds
    hist = open(str(tmp_path / "meta.hist")).read().splitlines()
    assert hist[0] == "# 0.01" and len(hist) == 1 + steps + 1 and all(len(ln.split()) == 2 for ln in hist[1:])
    cvd, Vd = eng.md_meta_hills()
    assert len(meta.hills) == steps + 1 and np.array_equal(np.array(meta.hills), cvd)
    assert (cvd > 0.05).all() and (cvd < 1.0).all() and Vd.max() > 0          # Q4, Q6 of a square net; the walk met its hills
    lines = _lines(str(tmp_path / "dev" / "active.log"))
    assert len(lines) >= steps + 1 and all("meta: " in ln for ln in lines)
    # calculate() at the last configuration: the model's results plus the twin's bias of the hills BELOW it — the bias the device
    # evaluated there and kept in its last row
    x = np.array(at.positions)
    assert np.array_equal(x, eng.md_state()["positions"])
    hills = list(meta.hills)
    meta.hills = hills[:-1]
    calc._calc = None
    calc.results = {}
    calc.calculate(Atoms(numbers, x, cell, True))
    V, Fb, Sb = meta.bias(x, cell, numbers, pbc=[True] * 3)
    meta.hills = hills
    plain = eng.predict(numbers, x, cell, [True] * 3)
    assert V > 0 and np.abs(Fb).max() > 1e-4
    assert abs(V - Vd[-1]) <= 1e-12 * max(V, np.abs(Fb).max())                # the twin's tolerance (test_hip_qlvar_device)
    assert np.abs(meta._cv - cvd[-1]).max() <= 1e-13
    assert np.abs(calc.results["forces"] - (plain["forces"] + Fb)).max() <= 1e-13 * max(np.abs(plain["forces"]).max(), np.abs(Fb).max())
    assert abs(float(calc.results["energy"]) - (plain["energy"] + V)) <= 1e-13 * max(1.0, abs(plain["energy"]))
    assert np.abs(calc.results["stress"] - (plain["stress"] + Sb)).max() <= 1e-13 * max(np.abs(plain["stress"]).max(), np.abs(Sb).max())
    eng.close()
