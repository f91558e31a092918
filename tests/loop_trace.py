"""Scripted stand-ins for the trace test of the host protocol around SGPRModel.md_run (test_loop_driver_cpu.py): an engine whose
md_run / md_state / md_frames / neb_state ... answer from the index of the configuration alone, a calculator whose hand-over
(calculate, _md_gate, _needs_seed, size) follows a table, and the scenarios.  Everything is recorded into one list: the calls
on the engine with their scalar arguments and which rows of deviates an md_run was handed, the yields and callbacks with
calc.step and the atoms, the log file, the returned dicts, exceptions.  The numbers are integers, flags, small binary fractions
(energy t / 8, positions t, covloss 0 or twice the gate) and single correctly rounded operations on them (a temperature
ke / (dof kB)): the trace is the same on every machine, and tests/golden/g18_loop_trace.json holds it as the commit before
autoforce_amd/device_loop.py produced it (tests/golden/gen/make_loop_trace.py)."""
import os
import re
import tempfile
from types import SimpleNamespace

import numpy as np

from autoforce_amd.ase_shim import Atoms, FixAtoms
from autoforce_amd.calculator import ActiveCalculator, Calculator
from autoforce_amd.workloads import FilterState

N, KE = 2, 0.25      # atoms; sum m v^2 of configuration t is KE (t + 1) behind its kick, KE (t + 1.5) before it


def san(x):
    """What the trace keeps of a value: scalars as they are, small arrays whole, of a large one its shape and first entry."""
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, (float, np.floating)):
        return float(x)
    if isinstance(x, (np.bool_, np.integer)):
        return x.item()
    if isinstance(x, dict):
        return {str(k): san(v) for k, v in sorted(x.items())}
    if isinstance(x, (tuple, list)):
        return [san(v) for v in x]
    a = np.asarray(x)
    return a.tolist() if a.size <= 6 else [list(a.shape), san(a.flat[0]), san(a.flat[-1])]


class Counter:
    """A stub for numpy's Generator: row k of everything it has drawn is filled with k (from 1)."""

    def __init__(self):
        self.k = 0

    def normal(self, size):
        out = np.empty(size)
        for row in out:
            self.k += 1
            row[...] = self.k
        return out


class ScriptEngine:
    """halts: configurations whose covloss is twice the gate whenever a gate is set; overflow: (t, v) — the v-th attempt to
    evaluate configuration t ends the call with code 2 and without that row; converge: the configuration that ends a relaxation
    or a band with code 3."""
    peer_world, species, cutoff = 1, (14,), 4.0

    def __init__(self, trace, halts=(), overflow=(), converge=None, m=1, quiet=False):
        self.trace, self.halts, self.overflow, self.converge = trace, set(halts), set(overflow), converge
        self.m, self.mu = m, (0 if m else None)
        self.K, self.runs = 1, 0
        self._begin()
        self.say = (lambda *a: None) if quiet else (lambda *a: trace.append(san(a)))

    # ---- beginnings
    def _begin(self):
        self.t, self.every, self.frames, self.visits = 0, 0, [], {}

    def md_begin(self, numbers, positions, cell, pbc, masses, velocities=None, **kw):
        self._begin()
        self.say("md_begin", len(numbers), positions[0, 0], velocities[0, 0], kw)

    def relax_begin(self, numbers, positions, cell, pbc, fmax, **kw):
        self._begin()
        self.say("relax_begin", len(numbers), positions[0, 0], fmax, kw)

    def neb_begin(self, numbers, images, cell, pbc, fmax, **kw):
        self._begin()
        self.K = len(images) - 2
        self.say("neb_begin", len(numbers), list(images.shape), fmax, kw)

    def relax_reset(self):
        self.say("relax_reset")

    def neb_reset(self):
        self.say("neb_reset")

    def md_record(self, every, velocities=True, results=True):
        self.every = int(every)
        self.say("md_record", every, velocities, results)

    # ---- the loop
    def md_run(self, nevals, noise=None, ediff=0.0, final=False):
        self.runs += 1
        self.say("md_run", nevals, None if noise is None else [list(noise.shape)] + [r[0, 0] for r in noise], ediff, final)
        t0, end = self.t, self.t + nevals
        stops = [(t, 0, 2) for t in {t for t, _ in self.overflow} if t0 <= t < end]
        if ediff > 0.0:
            stops += [(t, 1, 1) for t in self.halts if t0 <= t < end]
        if self.converge is not None and t0 <= self.converge < end:
            stops.append((self.converge, 2, 3))
        code, last = 0, end - 1
        for t, _, c in sorted(stops):
            if c == 2:
                self.visits[t] = self.visits.get(t, 0) + 1
                if (t, self.visits[t]) not in self.overflow:
                    continue
            code, last = c, (t - 1 if c == 2 else t)
            break
        ts = np.arange(t0, last + 1)
        sc = np.zeros((len(ts), 16))
        sc[:, 0], sc[:, 1], sc[:, 2] = ts / 8, 1 + ts % self.K, 1 + (ts + 1) % self.K
        sc[:, 12], sc[:, 13] = KE * (ts + 1), KE * (ts + 1.5)
        if code == 1:
            sc[-1, 11] = 2 * ediff
        stands = last - 1 if code == 1 else last
        self.frames = [t for t in range(t0, stands + 1) if self.every and t % self.every == 0]
        self.t = last + 1 if code == 2 or (code == 0 and not final) else last
        return sc, code

    def _results(self, t, shape=()):
        return dict(energy=np.full(shape, t / 8)[()], forces=np.full(shape + (N, 3), t / 16), stress=np.full(shape + (6,), t / 32),
                    beta=np.full(shape + (N,), t / 64))

    def md_state(self, which=0, results=False):
        self.say("md_state", which, results)
        t = self.t + which
        out = dict(positions=np.full((N, 3), float(t)), velocities_pre=np.full((N, 3), t + 0.25), velocities=np.full((N, 3), t + 0.5),
                   cell=np.diag(np.full(3, 8 + t / 8)), pending=False)
        if results:
            out.update(self._results(t))
        return out

    def md_frames(self, closed=True, reuse=False):
        self.say("md_frames", closed, reuse)
        f = np.array(self.frames, float)
        out = dict(index=np.array(self.frames, int), positions=np.ones((1, N, 3)) * f[:, None, None],
                   velocities_pre=np.ones((1, N, 3)) * (f[:, None, None] + 0.25), cell=np.eye(3) * (8 + f[:, None, None] / 8),
                   energy=f / 8, forces=np.ones((1, N, 3)) * f[:, None, None] / 16)
        return out

    def md_filter_push(self, dforces, dstress=None):
        self.say("md_filter_push", dforces, dstress)

    def md_filter_state(self):
        self.say("md_filter_state")
        return np.full((N, 3), self.t + 0.125), np.full(6, self.t + 0.0625)

    def neb_state(self, which=0, results=False):
        self.say("neb_state", which, results)
        t = self.t + which
        out = dict(positions=np.ones((self.K, N, 3)) * (t + np.arange(1, self.K + 1)[:, None, None] / 8))
        if results:
            out.update(self._results(t, (self.K,)))
        return out


class ScriptCalculator(ActiveCalculator):
    """ActiveCalculator's run_md / run_relax / run_neb around a ScriptEngine.  updates: row k — (updated, inducing LCEs gained,
    jump of the forces) — is what the k-th calculate() does; gates: _md_gate behind k calculate() calls; seed: _needs_seed
    before the first."""

    def __init__(self, engine, trace, logfile, updates=((True, 1, 0.5), (False, 0, 0.0)), gates=(0.5,), seed=False):
        Calculator.__init__(self)
        self.model = SimpleNamespace(engine=engine)
        self.process_group, self.logfile, self.stdout, self._logpref = None, logfile, False, ""
        self.step, self.test, self.meta, self._veto, self.nbeads = 0, None, None, {}, 1
        self._peer_atoms, self._sys_cache, self._calc = 0, None, object()
        self.updated, self.deltas, self._maxf, self._beta, self._cov, self._nl = False, None, None, None, None, None
        self.trace, self.updates, self.gates, self.seed, self.ncalc, self._size = trace, updates, gates, seed, 0, (1, 2)

    size = property(lambda self: self._size)

    def _needs_seed(self):
        return self.step == 0 and self.seed

    def _md_gate(self, numbers):
        return self.gates[min(self.ncalc, len(self.gates) - 1)]

    def calculate(self, atoms=None, properties=("energy",), system_changes=()):
        Calculator.calculate(self, atoms, properties, system_changes)
        upd, grow, jump = self.updates[self.ncalc % len(self.updates)]
        self.ncalc += 1
        self.trace.append(san(("calculate", self.step, snapshot(atoms))))
        self.updated = upd
        self._size = (self._size[0] + (1 if grow else 0), self._size[1] + grow)
        self.deltas = dict(energy=jump, forces=np.full((N, 3), jump), stress=np.full(6, jump / 2)) if jump else None
        self.engine.m, self.engine.mu = max(self.engine.m, 1), 0
        self.results = dict(energy=np.asarray(self.ncalc / 4), forces=np.full((N, 3), self.ncalc / 2), stress=np.zeros(6))
        self.results["free_energy"] = self.results["energy"]
        self._log_lines([(self.step, "calculate")])   # (whatever a real calculate() writes: its step index only)
        self.step += 1


class AttachingCalculator(ScriptCalculator):
    def _md_attach(self, eng):
        self.trace.append(["_md_attach"])
        return ("a", "b")

    def _md_attached_done(self, eng, keys):
        self.trace.append(san(("_md_attached_done", keys)))


def snapshot(atoms):
    v = atoms.get_velocities()
    return [atoms.positions[0, 0], None if v is None else v[0, 0], np.asarray(getattr(atoms.cell, "array", atoms.cell))[0, 0]]


def make_atoms(x=-1.0, constraint=None):
    return Atoms([14] * N, np.full((N, 3), x), 8.0 * np.eye(3), True, velocities=np.array([[0.5] * 3, [-0.5] * 3]), masses=np.ones(N),
                 constraint=constraint)


def _run(body, calc_cls=ScriptCalculator, eng=None, calc=None):
    """One scenario: body(calc, trace) inside a directory of its own; the trace with the log's lines behind it."""
    trace = []
    with tempfile.TemporaryDirectory() as d:
        log = os.path.join(d, "active.log")
        engine = ScriptEngine(trace, **(eng or {}))
        c = calc_cls(engine, trace, log, **(calc or {}))
        try:
            body(c, trace)
        except Exception as exc:  # noqa: BLE001
            trace.append(["raise", type(exc).__name__, str(exc)])
        lines = open(log).read().splitlines() if os.path.isfile(log) else []
    trace.append(["log"] + [re.sub(r"^\S+ \S+ ", "", ln) for ln in lines])
    return trace


def md_case(steps, temperature_K=300.0, holder=None, atoms=None, **kw):
    def body(calc, trace):
        at = make_atoms() if atoms is None else atoms()
        for st, E, T, upd, _ in calc.run_md(at, steps, temperature_K, **kw):
            trace.append(san(("yield", st, E, T, upd, calc.step, snapshot(at))))
        trace.append(san(("end", calc.step, snapshot(at), at.get_velocities()[1, 2])))
        if holder is not None:
            trace.append(san(("filter", holder.f, holder.s, holder.pushes)))
    return body


def relax_case(**kw):
    def body(calc, trace, kw=kw):
        at, kw = make_atoms(), dict(kw)
        if kw.pop("frames", False):
            kw["on_frame"] = lambda n, fr: trace.append(san(("on_frame", n, calc.step, fr["positions"][0, 0], fr["cell"][0][0], fr["energy"],
                                                              fr["forces"][0, 0])))
        out = calc.run_relax(at, **kw)
        trace.append(san(("return", out, calc.step, snapshot(at), calc.results, calc.get_covloss())))
    return body


def neb_case(K=3, band=True, **kw):
    def body(calc, trace, kw=kw):
        images, kw = [make_atoms(float(-i)) for i in range(K + 2)], dict(kw)
        if band:
            kw["on_band"] = lambda n, st: trace.append(san(("on_band", n, calc.step, st["positions"][0, 0, 0], st["energy"])))
        out = calc.run_neb(images, **kw)
        trace.append(san(("return", out, calc.step, [im.positions[0, 0] for im in images], calc.results)))
    return body


HALTS = {"never": (), "first_row": (8,), "first_of_run": (0,), "last_row": (7,), "consecutive": (3, 4), "final": (30,),
         "several": (7, 9, 10, 17, 30)}
MIX = (2, 8, 9, 21, 22, 30)    # the first and the last row of a batch, consecutive ones, the final evaluation, at every batch rule


def scenarios():
    """name -> a function that runs the scenario and returns its trace."""
    s = {}

    def add(name, body, **kw):
        s[name] = lambda: _run(body, **kw)
    # run_md
    for name, halts in HALTS.items():   # (chunk = 8: the batch never grows; a halt at 8 is the first row of the second batch)
        add(f"md_langevin_rng_{name}", md_case(30, friction=0.5, rng=Counter(), chunk=8), eng=dict(halts=halts))
    add("md_langevin_rng_growing_batch", md_case(70, friction=0.5, rng=Counter(), chunk=32), eng=dict(halts=(7, 8, 30, 70)))
    add("md_langevin_rng_code2", md_case(30, friction=0.5, rng=Counter(), chunk=32), eng=dict(halts=(5,), overflow=((5, 2), (12, 1), (13, 1))))
    add("md_langevin_device_rng", md_case(30, friction=0.5, seed=7), eng=dict(halts=MIX))
    add("md_nve", md_case(30, friction=0.0), eng=dict(halts=MIX))
    for rec in (False, True):
        add(f"md_sync3_record{rec}", md_case(30, friction=0.5, rng=Counter(), sync_every=3, record=rec), eng=dict(halts=MIX))
        add(f"md_npt_sync3_record{rec}", md_case(30, tdamp_fs=32.0, pfactor=2.0, externalstress=0.5, iso=True, sync_every=3, record=rec),
            eng=dict(halts=MIX))
    add("md_sync1_record", md_case(20, friction=0.5, rng=Counter(), sync_every=1), eng=dict(halts=(0, 5, 6, 20)))
    for rec_max in (1, 2):
        def lowered(calc, trace, rec_max=rec_max):
            calc.RECORD_BYTES = 48 * N * rec_max
            md_case(30, friction=0.5, rng=Counter(), sync_every=3, chunk=32)(calc, trace)
        add(f"md_sync3_record_max{rec_max}", lowered, eng=dict(halts=MIX))
    add("md_nose_hoover", md_case(30, tdamp_fs=32.0), eng=dict(halts=MIX))
    add("md_fixed_atom", md_case(12, friction=0.5, rng=Counter(), atoms=lambda: make_atoms(constraint=FixAtoms(indices=[1]))), eng=dict(halts=(5,)))
    holder = FilterState(0.5)
    add("md_filter", md_case(30, friction=0.5, rng=Counter(), ml_filter=holder, holder=holder), eng=dict(halts=MIX),
        calc=dict(updates=((True, 1, 0.5), (False, 0, 0.0), (True, 2, 0.25))))
    add("md_empty_model", md_case(30, friction=0.5, rng=Counter()), eng=dict(halts=(0, 9), m=0), calc=dict(seed=True))
    add("md_empty_model_npt_sync", md_case(12, tdamp_fs=32.0, pfactor=2.0, sync_every=3), eng=dict(halts=(3,), m=0), calc=dict(seed=True))
    add("md_attached", md_case(30, friction=0.5, rng=Counter(), sync_every=3), calc_cls=AttachingCalculator, eng=dict(halts=MIX))
    add("md_gate_from_table", md_case(30, friction=0.5, rng=Counter()), eng=dict(halts=MIX), calc=dict(gates=(0.5, 0.25, 0.125)))
    add("md_zero_steps", md_case(0, friction=0.5, rng=Counter()), eng=dict(halts=(0,)))
    add("md_barostat_needs_thermostat", md_case(5, pfactor=2.0))
    add("md_barostat_refuses_constraints", md_case(5, tdamp_fs=32.0, pfactor=2.0, atoms=lambda: make_atoms(constraint=FixAtoms(indices=[1]))))
    # run_relax
    for clear in (False, True):
        for grow in (0, 1):
            add(f"relax_clear{clear}_grow{grow}", relax_case(fmax=0.25, steps=40, clear_hist=clear, chunk=32), eng=dict(halts=(0, 7, 8, 9, 30), converge=33),
                calc=dict(updates=((bool(grow), grow, 0.0),)))
    add("relax_code3_mid_batch", relax_case(fmax=0.25, steps=100, cell=True, mask=[1, 1, 1, 0, 0, 0], dt=0.125), eng=dict(converge=11))
    add("relax_steps_exhausted", relax_case(fmax=0.25, steps=30, chunk=8), eng=dict(halts=(30,)))
    add("relax_code2", relax_case(fmax=0.25, steps=30), eng=dict(halts=(5,), overflow=((5, 2), (12, 1)), converge=20))
    add("relax_empty_model", relax_case(fmax=0.25, steps=12), eng=dict(halts=(4,), m=0), calc=dict(seed=True))
    for rec_max in (1, 2, 1 << 20):
        def framed(calc, trace, rec_max=rec_max):
            calc.RECORD_BYTES = 8 * (7 * N + 11) * rec_max
            relax_case(fmax=0.25, steps=40, cell=True, frames=True, interval=3, chunk=32)(calc, trace)
        add(f"relax_frames_max{rec_max}", framed, eng=dict(halts=(0, 8, 9, 21), converge=31))   # (31: the final structure is no multiple of 3)
    add("relax_frames_final_on_interval", relax_case(fmax=0.25, steps=40, frames=True, interval=3), eng=dict(converge=30))
    add("relax_frames_steps_exhausted", relax_case(fmax=0.25, steps=10, frames=True, interval=4), eng=dict(halts=(10,)))
    # run_neb
    for grow in (0, 1):
        add(f"neb_halts_grow{grow}", neb_case(fmax=0.25, steps=40, chunk=32, k=0.5, climb=True), eng=dict(halts=(0, 7, 8, 9, 30), converge=33),
            calc=dict(updates=((bool(grow), grow, 0.0),)))
    add("neb_code3", neb_case(fmax=0.25, steps=100), eng=dict(converge=11))
    add("neb_steps_exhausted", neb_case(fmax=0.25, steps=30, chunk=8), eng=dict(halts=(30,)))
    add("neb_code2", neb_case(fmax=0.25, steps=30), eng=dict(halts=(5,), overflow=((5, 2), (12, 1)), converge=20))
    add("neb_no_callback", neb_case(fmax=0.25, steps=12, band=False), eng=dict(halts=(4,)))
    add("neb_empty_model", neb_case(fmax=0.25, steps=12), eng=dict(halts=(4,), m=0), calc=dict(seed=True))
    add("neb_fixed_atom", lambda calc, trace: trace.append(san(("return", calc.run_neb(
        [make_atoms(float(-i), constraint=FixAtoms(indices=[1])) for i in range(4)], fmax=0.25, steps=5)))), eng=dict(converge=3))
    add("neb_no_interior_image", lambda calc, trace: calc.run_neb([make_atoms(), make_atoms()]))
    return s


def run_all():
    return {name: run() for name, run in scenarios().items()}
