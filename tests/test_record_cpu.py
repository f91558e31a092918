"""The frame record of the device loops without a GPU: the bookkeeping helper against a brute-force walk over halt codes and
intervals, md_record_kernel's resources from the build's metadata, and the three entry points in the library, the header and
the ctypes table."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, ROOT, _metadata


def _brute(t0, done, code, every):
    """Which evaluations of a call leave a frame that stands, spelled out evaluation by evaluation."""
    out = []
    for j in range(done):
        n = t0 + j
        halted_here = code == 1 and j == done - 1      # the covloss gate: the row is there, the frame is left to the next call
        if every and n % every == 0 and not halted_here:
            out.append(n)
    return out


def test_recorded_indices_against_a_brute_force_walk():
    from autoforce_amd.model import recorded_indices
    for every in (0, 1, 2, 3, 7, 100):
        for t0 in (0, 1, 2, 5, 6, 99, 100, 101):
            for done in range(0, 17):
                for code in (0, 1, 2, 3):
                    if code == 1 and done == 0:
                        continue                        # (a gate halt always returns its row)
                    assert recorded_indices(t0, done, code, every) == _brute(t0, done, code, every), (t0, done, code, every)


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_record_kernel_has_no_scratch(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    mine = {k: v for k, v in meta.items() if "md_record_kernel" in k and "private_segment_fixed_size" in v}
    assert len(mine) == 1, sorted(meta)[:20]
    for name, md in mine.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("vgpr_count", 0) <= 32, (name, md)    # (a copy: nothing that could limit the occupancy of what runs beside it)


def test_entry_points_are_exported_declared_and_bound():
    from autoforce_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "sgpr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("sgpr_md_record", 3), ("sgpr_md_frame_count", 2), ("sgpr_md_frames", 7)):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/sgpr_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs


def test_python_surface_is_there():
    from autoforce_amd import SGPRModel
    from autoforce_amd.calculator import ActiveCalculator
    import inspect
    for name in ("md_record", "md_frame_count", "md_frames"):
        assert callable(getattr(SGPRModel, name))
    assert inspect.signature(ActiveCalculator.run_md).parameters["record"].default is True
    p = inspect.signature(ActiveCalculator.run_relax).parameters
    assert p["on_frame"].default is None and p["interval"].default == 1
    assert ActiveCalculator.RECORD_BYTES == 256 << 20


def _loop_engine():
    """The CPU oracle with a stand-in for the device loop's Python surface (md_begin / md_run / md_state / md_record /
    md_frames): symplectic Euler on the host around predict(), with sgpr_md_run's rules — a row per evaluation, halt code 1 with
    the halting row returned and the state left at that configuration, `final` moving nothing behind the last evaluation, frames
    of the accepted evaluations at the multiples of `every`.  What run_md does with that surface is what is under test."""
    import numpy as np
    from helpers import OracleModel

    class LoopEngine(OracleModel):
        peer_world = 1

        def md_begin(self, numbers, positions, cell, pbc, masses, velocities=None, dt=1.0, **kw):
            self._s = dict(numbers=np.asarray(numbers), cell=np.asarray(cell, float), pbc=pbc, m=np.asarray(masses, float)[:, None], dt=dt, t=0,
                           x=np.array(positions, float), v=np.zeros_like(positions) if velocities is None else np.array(velocities, float),
                           prev=None, every=0, frames=[], runs=0)

        def md_record(self, every, velocities=True, results=True):
            self._s["every"] = int(every)

        def md_run(self, nevals, noise=None, ediff=0.0, final=False):
            s = self._s
            s["frames"], s["runs"] = [], s["runs"] + 1
            rows, code = [], 0
            for j in range(nevals):
                out = self.predict(s["numbers"], s["x"], s["cell"], s["pbc"])
                ke = float((s["m"] * s["v"] ** 2).sum())
                row = np.zeros(16)
                row[0], row[11], row[12], row[13] = out["energy"], float(out["beta"].max()), ke, ke
                rows.append(row)
                s["last"] = out
                if ediff > 0.0 and row[11] >= ediff:
                    code = 1
                    break
                if s["every"] and s["t"] % s["every"] == 0:
                    s["frames"].append((s["t"], s["x"].copy(), s["v"].copy()))
                if final and j == nevals - 1:
                    break
                s["prev"] = (s["x"].copy(), s["v"].copy())
                s["v"] = s["v"] + s["dt"] * out["forces"] / s["m"]
                s["x"] = s["x"] + s["dt"] * s["v"]
                s["t"] += 1
            return np.array(rows).reshape(-1, 16), code

        def md_state(self, which=0, results=False):
            s = self._s
            x, v = (s["x"], s["v"]) if which == 0 else s["prev"]
            out = dict(positions=x.copy(), velocities_pre=v.copy(), velocities=v.copy(), pending=False)
            if results:
                out.update(forces=s["last"]["forces"], beta=s["last"]["beta"], energy=s["last"]["energy"], stress=s["last"]["stress"])
            return out

        def md_frame_count(self):
            return len(self._s["frames"])

        def md_frames(self, closed=True, reuse=False):
            f = self._s["frames"]
            return dict(index=np.array([a[0] for a in f]), positions=np.array([a[1] for a in f]), velocities_pre=np.array([a[2] for a in f]))

    return LoopEngine


@pytest.mark.parametrize("k", [1, 3])
def test_run_md_records_instead_of_cutting_on_a_host_stand_in(tmp_path, k):
    """run_md(sync_every=k) around a stand-in for the device loop: with record=True everything a caller observes — the yields,
    self.step and the atoms at every multiple of k, behind every update and at the end, the log — is what record=False shows,
    and the loop is entered fewer times."""
    import numpy as np
    import active_common as ac
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import PairTeacher
    from oracle import oracle as orc
    steps, res = 14, {}
    orc.set_num_threads(1)   # (a fixed summation order in the oracle: the two runs are compared bit for bit)
    for record in (False, True):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        d = tmp_path / str(record)
        d.mkdir()
        calc = ActiveCalculator(engine=_loop_engine()(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                                logfile=str(d / "active.log"), pckl=None, tape=None, **ac.KW)
        at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
        out, seen = [], {}
        for st, E, Tk, u, w in calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.0, rng=np.random.default_rng(9), chunk=8, sync_every=k,
                                           record=record):
            out.append((st, E, Tk, bool(u), calc.step if st % k == 0 else None))
            if st % k == 0 or u:
                seen[st] = (at.positions.copy(), at.get_velocities().copy())
        last = (at.positions.copy(), at.get_velocities().copy(), calc.step)
        log = [re.sub(r"^\S+ \S+ ", "", ln) for ln in open(d / "active.log").read().splitlines()]
        res[record] = (out, seen, last, log, calc.engine._s["runs"], calc.size)
    orc.set_num_threads(os.cpu_count() or 1)
    (co, cs, cl, clog, cruns, csize), (ro, rs, rl, rlog, rruns, rsize) = res[False], res[True]
    assert len(co) == steps + 1 and ro == co and rlog == clog and rsize == csize
    assert any(o[3] for o in co), "nothing halted the loop: the scenario does not exercise the gate"
    assert sorted(rs) == sorted(cs)
    for st in cs:
        assert np.array_equal(cs[st][0], rs[st][0]) and np.array_equal(cs[st][1], rs[st][1]), st
    assert np.array_equal(cl[0], rl[0]) and np.array_equal(cl[1], rl[1]) and cl[2] == rl[2]
    assert rruns < cruns, (rruns, cruns)


def test_run_relax_reports_frames_from_the_host_loop_too(tmp_path):
    """Where run_relax falls back to the host loop (an engine without the device loop), on_frame is served from its steps:
    every evaluation once, in order, the final structure last; with an interval the multiples and the final one."""
    import numpy as np
    import active_common as ac
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import OracleModel, PairTeacher
    got = {}
    for interval in (1, 4):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        calc = ActiveCalculator(engine=OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0), logfile=None, pckl=None,
                                tape=None, **ac.KW)
        at = Atoms(numbers, pos, cell, True)
        frames = []
        out = calc.run_relax(at, fmax=1e-3, steps=9, interval=interval, on_frame=lambda n, fr: frames.append((n, fr["positions"].copy(), fr["energy"])))
        got[interval] = (frames, out["evaluations"])
        assert np.array_equal(frames[-1][1], at.positions) and frames[-1][2] == float(calc.results["energy"])
    (f1, n1), (f4, n4) = got[1], got[4]
    assert n1 == n4 == 10 and [f[0] for f in f1] == list(range(10))
    assert [f[0] for f in f4] == sorted(set(range(0, 10, 4)) | {9})
