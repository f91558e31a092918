"""The committee under a barostat without a GPU, with the means of test_bcm_md_cpu.py (the CPU oracle behind test_record_cpu's
LoopEngine): the host twin workloads.npt_moving_cell around a BCMActiveCalculator — the definition of what the device loop
computes (sgpr_md_committee on a run with sgpr_md_barostat) — moves its cell by the committee's stress, and run_md sends a
committee with a barostat to the device loop where md_on_device_ok() holds."""
import numpy as np

import bcm_md_common as bc
from helpers import load
from test_record_cpu import _loop_engine

T, TDAMP = 600.0, 25.0


def _make_engine():
    g = load("g5_big40")
    LoopEngine = _loop_engine()
    return lambda: LoopEngine(int(g["lmax"]), int(g["nmax"]), float(g["eta"]), float(g["rc"]), species=g["species"].tolist())


def _baro():
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    return dict(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)


def test_the_40_atom_frame_qualifies_for_the_barostat():
    """Periodic in all three directions, and upper triangular with a positive diagonal after npt.make_cell_upper_triangular —
    which leaves this cubic cell and its positions as they are."""
    from autoforce_amd.npt import make_cell_upper_triangular
    g = load("g5_big40")
    pos, cell, R = make_cell_upper_triangular(g["positions"], g["cell"])
    assert all(bool(b) for b in g["pbc"])
    assert cell[1, 0] == 0.0 and cell[2, 0] == 0.0 and cell[2, 1] == 0.0 and (np.diag(cell) > 0.0).all()
    assert np.array_equal(cell, g["cell"]) and np.array_equal(pos, g["positions"])


def test_the_twin_moves_its_cell_by_the_committees_stress():
    """h_2 = h_0 + 2 dt h_1 eta_1 with h_1 = h_0 and eta_1 = -deta(dt) + deta(2 dt) of the stress at configuration 0 less its
    ideal-gas part: the cell of evaluation 2 is the one _npt_deta gives for the COMMITTEE's stress, bit for bit, and not the one
    the live model alone moves to."""
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.npt import zero_mean_momentum
    from autoforce_amd.workloads import FS, MASS, _device_order_sum, _m3_mul, _npt_deta, npt_moving_cell
    from oracle import oracle as orc
    import os
    orc.set_num_threads(1)   # (a fixed summation order in the oracle: two evaluations of a configuration are the same bits)
    try:
        make = _make_engine()
        calc, g = bc.g12_calculator(make)
        numbers, pos, cell, pbc = g["numbers"], g["positions"], g["cell"], g["pbc"]
        species = calc.engine.species
        vel, baro = bc.thermal_velocities(numbers, temperature=T), _baro()
        kw = dict(temperature=T, dt_fs=1.0, tdamp_fs=TDAMP, vel=vel, species=species, **baro)
        both = [h.copy() for _, E, Tk, _, x, v, h, e, z, zi in npt_moving_cell(calc, numbers, pos, cell, pbc, 2, **kw)]
        alone_calc, _ = bc.g12_calculator(make, members=False)
        alone = [h.copy() for _, E, Tk, _, x, v, h, e, z, zi in npt_moving_cell(alone_calc, numbers, pos, cell, pbc, 2, **kw)]
        probe, _ = bc.g12_calculator(make)
        at = Atoms(numbers, pos.copy(), cell, pbc)
        at.calc = probe
        stress6 = np.asarray(at.get_stress(), float)
    finally:
        orc.set_num_threads(os.cpu_count() or 1)
    assert set(probe.bcm_weights) == {"a", "live"} and 0.0 < probe.bcm_weights["a"] < 1.0
    mass = np.array([MASS[int(z)] for z in numbers])
    v0 = zero_mean_momentum(vel, mass)
    order = np.argsort([species.index(int(z)) for z in numbers], kind="stable")
    voigt = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    S = [_device_order_sum((mass * (v0[:, a] * v0[:, b]))[order]) for a, b in voigt]
    h0 = [[float(v) for v in row] for row in np.asarray(cell, float)]
    vol = abs((h0[0][0] * h0[1][1]) * h0[2][2])
    sig = [stress6[k] - S[k] / vol for k in range(6)]
    dt = 2.0 * (0.5 * (1.0 * FS))
    pfact = 1.0 / (float(baro["pfactor"]) * ((h0[0][0] * h0[1][1]) * h0[2][2]))
    ext6 = [-float(baro["externalstress"])] * 3 + [0.0] * 3
    ones = [[1.0] * 3 for _ in range(3)]
    d0 = _npt_deta(dt, pfact, h0, sig, ext6, ones, 1.0)
    d = _npt_deta(2.0 * dt, pfact, h0, sig, ext6, ones, 1.0)
    eta1 = [[(0.0 - d0[r][c]) + d[r][c] for c in range(3)] for r in range(3)]
    he = _m3_mul(h0, eta1)
    h2 = np.array([[h0[r][c] + (2.0 * dt) * he[r][c] for c in range(3)] for r in range(3)])
    assert np.array_equal(both[0], np.asarray(cell, float)) and np.array_equal(both[1], both[0])
    assert np.array_equal(both[2], h2)
    assert not np.array_equal(alone[2], both[2]) and np.abs(alone[2] - both[2]).max() > 1e-9


def test_run_md_sends_a_committee_with_a_barostat_to_the_device_loop(monkeypatch):
    """The stand-in engine records what run_md asks of it: md_begin with the barostat, then md_committee with the member's
    engine, and the host loop npt_moving_cell is not entered.  With constraints the run still goes to a host loop."""
    import autoforce_amd.workloads as wl
    from autoforce_amd.ase_shim import Atoms
    make = _make_engine()
    calc, g = bc.g12_calculator(make)
    cls, calls = type(calc.engine), []
    base_begin, base_state = cls.md_begin, cls.md_state

    def md_begin(self, *a, **k):
        calls.append(("md_begin", {q: k.get(q) for q in ("pfactor", "ttime", "externalstress")}))
        self._md = dict(npt=k.get("pfactor") is not None)   # (what SGPRModel.md_begin notes of a run with a barostat)
        return base_begin(self, *a, **k)

    def md_state(self, which=0, results=False):
        out = base_state(self, which, results)
        out["cell"] = self._s["cell"]
        return out

    def host_loop(*a, **k):
        raise AssertionError("the host loop npt_moving_cell was entered")

    monkeypatch.setattr(cls, "md_begin", md_begin)
    monkeypatch.setattr(cls, "md_state", md_state)
    monkeypatch.setattr(cls, "md_committee", lambda self, members, moving_cell=None: calls.append(("md_committee", list(members), moving_cell)),
                        raising=False)
    monkeypatch.setattr(cls, "md_committee_info", lambda self: (np.array([0.25, 0.75]), np.zeros(2)), raising=False)
    monkeypatch.setattr(wl, "npt_moving_cell", host_loop)
    assert calc.md_on_device_ok() is True
    numbers, pos, cell, pbc = g["numbers"], g["positions"], g["cell"], g["pbc"]
    at = Atoms(numbers, pos.copy(), cell, pbc, velocities=bc.thermal_velocities(numbers, temperature=T))
    baro = _baro()
    out = list(calc.run_md(at, 2, T, dt_fs=1.0, tdamp_fs=TDAMP, **baro))
    assert [o[0] for o in out] == [0, 1, 2]
    assert [c[0] for c in calls] == ["md_begin", "md_committee"]
    assert calls[0][1]["pfactor"] == baro["pfactor"] and calls[0][1]["ttime"] is not None
    assert calls[1][1] == [calc.model_dict["a"].engine] and calls[1][2] is True   # (the opt-in a run with a barostat needs)
    assert calc.bcm_weights == {"a": 0.25, "live": 0.75}
    # where the device loop is not available the same call is the host loop's
    monkeypatch.setattr(type(calc), "md_on_device_ok", lambda self: False)
    try:
        list(calc.run_md(at, 1, T, dt_fs=1.0, tdamp_fs=TDAMP, **baro))
    except AssertionError as e:
        assert "the host loop npt_moving_cell was entered" in str(e)
    else:
        raise AssertionError("with md_on_device_ok() False the run must go to the host loop")
