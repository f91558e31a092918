"""The host side of the device loops, once: what ActiveCalculator.run_md, run_relax and run_neb do around SGPRModel.md_run.

`batches` owns the protocol — how many evaluations a call asks for, its gate, `final`, which rows stand, when calculate() takes
over and the run ends — and hands every call's rows to the mode as a Batch; `log_rows` owns which rows are logged and counted.
A mode brings what is its own: how a row reads as a log line, what it does with a batch (yields, frames, callbacks), the
deviates of a call (MD with a caller's generator), and what its hand-over consists of.  The small things the three modes share
stand below them: state -> atoms, the held-component mask, the hand-over's calculate(), the frame record's cap and fetch."""
import time
from collections import namedtuple

import numpy as np

from .model import recorded_indices


class Batch(namedtuple("Batch", "first sc code rows done final resumed prev share t_host")):
    """One md_run call.  first: trajectory index of its first evaluation; sc, code: what md_run returned; rows: the accepted
    rows of sc — all of them, less the last one behind the covloss gate (code 1), which calculate() and the next call deal
    with — as lists of Python floats; done: first + len(rows); final: the call was the run's last by count; resumed: its first
    row is the configuration calculate() has just dealt with, evaluated again; prev: the row before rows[0] (None at the
    start); share: wall seconds per row; t_host: wall seconds of the hand-over before it."""
    __slots__ = ()


def batches(calc, eng, numbers, steps, chunk, resumed=False, cap=None, deviates=None, hand_over=None):
    """Evaluations 0 ... steps of the run begun on `eng`, one Batch per md_run call, until they are done or the device reports
    convergence (code 3).
    A call asks for `batch` evaluations: min(8, chunk) at first, twice as many after every call that ran through, up to
    chunk, and min(8, chunk) again after any halt code (2, an overflow of the device's tables, only does that) — less what
    cap(n, done) takes off, and never past evaluation `steps`, which is `final`: nothing moves behind it.
    The covloss gate is calc._md_gate(numbers).  Code 1 — the last row reached it, the device stands at that configuration —
    calls hand_over(batch) once the mode is through with the batch: calculate() logs and counts it and updates the model;
    the next call is `resumed`: that one configuration again, ungated, to move on from it.  resumed=True from the start: the
    first configuration has been through calculate() already.
    deviates(n, final): the noise rows of a call (default: None)."""
    done, batch, prev, t_host, code = 0, min(8, chunk), None, 0.0, 0
    while done <= steps and code != 3:
        n = 1 if resumed else min(batch, steps + 1 - done)
        if cap is not None:
            n = cap(n, done)
        final = done + n == steps + 1
        noise = None if deviates is None else deviates(n, final)
        gate = 0.0 if resumed else calc._md_gate(numbers)
        t_run = time.time()
        sc, code = eng.md_run(n, noise, ediff=gate, final=final)
        rows = (sc[:-1] if code == 1 else sc).tolist()
        b = Batch(done, sc, code, rows, done + len(rows), final, resumed, prev, (time.time() - t_run) / max(len(rows), 1), t_host)
        if rows:
            done, prev, resumed = b.done, rows[-1], False
        yield b
        batch = min(8, chunk) if code else min(2 * batch, chunk)
        if code == 1:
            t_host = time.time()
            hand_over(b)
            resumed = True
            t_host = time.time() - t_host


def log_rows(calc, b, line):
    """The log lines of a batch, in one open: every row writes line(t, row, row before it) under the step count and advances
    it — but for the first row of a resumed batch, whose line calculate() wrote and whose step it counted.  Returns calc.step
    as it is behind every row, and leaves it at the last."""
    step, prev, lines, counts = calc.step, b.prev, [], []
    for k, r in enumerate(b.rows):
        if k or not b.resumed:
            lines.append((step, line(b.first + k, r, prev)))
            step += 1
        prev = r
        counts.append(step)
    calc._log_lines(lines)
    calc.step = step
    return counts


def hand_over(calc, atoms):
    """calculate() on a configuration the device stopped at: update_results + update + the log line, as inside an ASE loop."""
    atoms.calc = calc
    calc.results = {}
    calc.calculate(atoms)


def first_on_host(calc, atoms):
    """The first configuration through calculate() before the device loop: an empty model is seeded by it."""
    atoms.calc = calc
    atoms.get_forces()


def put_state(atoms, st, cell=False, velocities=None):
    """A state of the device loop into the atoms: the cell (where it moves), the positions, the velocities under that key."""
    if cell:
        if hasattr(atoms.cell, "array"):
            atoms.set_cell(st["cell"])
        else:
            atoms.cell = np.array(st["cell"], float)
    atoms.positions = st["positions"]
    if velocities:
        atoms.set_velocities(st[velocities])


def held(mask):
    """A held-component mask (ActiveCalculator.constraint_mask), or None where it holds nothing."""
    return None if mask is None or not mask.any() else mask


def record_cap(budget, frame_bytes, every):
    """cap(n, done) of a run that records every `every`-th configuration (SGPRModel.md_record): a call's frames stay within
    `budget` bytes."""
    rec_max = max(1, budget // frame_bytes)
    return lambda n, done: max(1, min(n, rec_max * every - done % every))


def sync_cap(every):
    """cap(n, done) of a run that is cut at the multiples of `every`: such a configuration ends its call."""
    return lambda n, done: min(n, every - done % every if done % every else 1)


def recorded_frames(eng, b, every):
    """The frames batch b left in the record, or None without asking the device where the bookkeeping says there are none."""
    return eng.md_frames(reuse=True) if recorded_indices(b.first, len(b.sc), b.code, every) else None
