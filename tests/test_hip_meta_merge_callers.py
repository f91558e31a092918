"""ActiveCalculator(meta=Meta(..., merge=)).run_md: the merged form of the bias through the caller that drives it
(tests/test_hip_meta_callers.py has the unmerged flow, tests/test_hip_meta_merge_device.py the device loop): run_md hands
meta.merge to the engine and nothing else in its flow changes — meta.hist keeps one line per deposit, the host Meta mirrors the
hills, its histogram() is the engine's table, and calculate() on the final configuration adds the merged bias the loop added."""
import numpy as np
import pytest

import active_common as ac
from test_hip_meta_callers import _calc


@pytest.mark.gpu
def test_run_md_hands_the_merge_to_the_engine(tmp_path):
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    rng0, numbers, pos, cell = ac.start(0)
    steps = 40
    meta = Meta(Catvar(Posvar(1, select=9), Distance(0, 5)), sigma=0.05, w=0.05, hist=str(tmp_path / "meta.hist"), merge=8)
    calc = _calc(tmp_path / "dev", SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), meta)
    eng, seen = calc.engine, []
    md_meta = eng.md_meta
    eng.md_meta = lambda *a, **k: (seen.append(k.get("merge")), md_meta(*a, **k))[1]
    at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
    out = list(calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, seed=7, chunk=16))
    assert len(out) == steps + 1 and calc.md_on_device_ok() and seen == [8]
    assert [o[0] for o in out if o[3]]                                        # the gate fired in the middle of the run: halts and updates
    # meta.hist: one line per deposit, as before; the Meta holds the hills the device holds
    hist = open(str(tmp_path / "meta.hist")).read().splitlines()
    assert hist[0] == "# 0.05" and len(hist) == 1 + steps + 1
    cvd, Vd = eng.md_meta_hills()
    assert len(meta.hills) == steps + 1 and np.array_equal(np.array(meta.hills), cvd) and Vd.max() > 0
    # the histogram of the Meta is the table of the engine
    centres, counts, rows = eng.md_meta_table()
    hc, hn = meta.histogram()
    assert rows == (steps // 8) * 8 == hn.sum() and np.array_equal(hc, centres) and np.array_equal(hn, counts)
    # calculate() on the final configuration: the energy the loop reported for it (the hills below it: its own row set aside)
    own = meta.hills.pop()
    calc._calc = None                                                         # (no teacher: calculate() evaluates, nothing is learnt)
    at.calc = calc
    calc.results = {}
    calc.calculate(at)
    e_loop = out[-1][1]
    assert abs(float(calc.results["energy"]) - e_loop) <= 1e-13 * max(1.0, abs(e_loop)), (float(calc.results["energy"]), e_loop)
    assert abs(meta.energy - Vd[-1]) <= 1e-13 * max(1.0, abs(e_loop)) and meta.energy > 0
    meta.hills.append(own)
    eng.close()
