"""What the GPU tests of the six in-loop accumulators of the device MD loop share (test_hip_{msd,rdf,vacf,vanhove,adf,sq}_device.py):
the model and the frames, ONE run loop (run), and the test bodies that differ between the accumulators in a noun, a function name
and an argument list only — the refusal matrix (refusals), the two-rank refusal with its one worker (two_rank_refusal), the run
that is not disturbed (moves_nothing), and the skeletons of the covloss halt (halt_counts_once), of the later run and the
handle's memory (later_run_and_memory) and of run_md on the host against the device (run_md_host_and_device).  A module describes
its accumulator once, in an Acc, and defines every test under its own name; what exists for one accumulator only stays there.
Like csrc/md_host.inc's MD_ACC the description holds the function's name, the noun and the two clauses of the messages — in the
test's own spelling, never read out of the library.  Frame and model are those of test_hip_npt_device.py (LiPS, side 8: 192 /
64 / 256 atoms, cubic 21.76 A, m = 48)."""
import ctypes as C
import functools
import importlib
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

from test_hip_npt_device import _model

T = 600.0
EVALS = 40
POSITIONS = (dict(velocities=False, results=False), {}, ("positions",))   # md_record's, md_frames' arguments; the arrays kept


@functools.lru_cache(maxsize=None)
def _shared():
    mdl, frame = _model()
    return mdl, frame


def lib():
    from autoforce_amd import _lib
    return _lib.load()


def _thermal(numbers, pos, cell, pbc):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return numbers, pos, cell, pbc, mass, vel


def _frame(kind=None):
    """The shared model's frame; "sub200": 200 of its atoms (the smallest species has fewer than 64, no segment ends on a wave);
    "chunks": 540 atoms of lips(10) — the largest species spans two chunks of 256, the second ragged; "thin": the 256 atoms of
    lips((8, 8, 4)), L_z = 10.88."""
    from autoforce_amd.workloads import lips
    if kind == "thin":
        return _thermal(*lips((8, 8, 4), seed=0))
    numbers, pos, cell, pbc = _shared()[1]
    if kind is not None:
        if kind == "chunks":
            numbers, pos, cell, pbc = lips(10, seed=0)
        keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=200 if kind == "sub200" else 540, replace=False))
        numbers, pos = numbers[keep], pos[keep]
    return _thermal(numbers, pos, cell, pbc)


def _begin(mdl, fr, nh=False, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    numbers, pos, cell, pbc, mass, vel = fr
    par = dict(dt=1.0 * FS, kT=kB * T, friction=0.0, ttime=25.0 * FS) if nh else dict(dt=1.0 * FS, kT=kB * T, friction=0.05)
    par.update(kw)
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **par)


def _noise(fr, evals=EVALS):
    return np.random.default_rng(9).normal(size=(evals, len(fr[0]), 3))


def attached(**accs):
    """run()'s (attach, read) for the accumulators `name=arguments of md_<name>`, attached in the order given, a None left out;
    read returns {name: md_<name>_table()}."""
    accs = {k: v for k, v in accs.items() if v is not None}
    return (lambda mdl: [getattr(mdl, "md_" + k)(*v) for k, v in accs.items()],
            lambda mdl: {k: getattr(mdl, f"md_{k}_table")() for k in accs})


def run(fr, attach=None, read=None, cuts=(EVALS,), nh=False, record=True, seed=None, label="", overflow=False, **begin_kw):
    """A run of sum(cuts) evaluations, one md_run per cut, on the shared model: attach(mdl) attaches what the case wants behind
    the frame record, read(mdl) reads it behind the last cut.  record: True — positions at every = 1 —, False, or (md_record's
    arguments, md_frames' arguments, the arrays to keep).  overflow: a cut may end with halt code 2 (a capacity outgrown; the rows
    before it stand) and is then repeated from where it stopped.  Returns (what read returned or None, the kept arrays over the
    run — one array, or a tuple of several — or None, scalar rows, final state)."""
    mdl = _shared()[0]
    _begin(mdl, fr, nh=nh, **({} if seed is None else dict(seed=seed)), **begin_kw)
    if record is True:
        record = POSITIONS
    if record:
        what, frames_kw, keep = record
        mdl.md_record(1, **what)
    if attach is not None:
        attach(mdl)
    noise = None if (nh or seed is not None) else _noise(fr, sum(cuts))
    rows, kept, t = [], [], 0
    for n in cuts:
        done = 0
        for _ in range(4 if overflow else 1):
            t_call = time.perf_counter()
            sc, code = mdl.md_run(n - done, None if noise is None else noise[t + done:t + n])
            print(f"md_run({n - done}) on {len(fr[0])} atoms, {label}: {f'code {code}, ' if overflow else ''}"
                  f"{1e6 * (time.perf_counter() - t_call) / max(len(sc), 1):.1f} us per evaluation")
            assert (code == 0 and len(sc) == n - done) or (overflow and code == 2), (code, len(sc), n, done)
            rows.extend(sc)
            if record and len(sc):
                f = mdl.md_frames(**frames_kw)
                assert list(f["index"]) == list(range(t + done, t + done + len(sc)))
                kept.append([f[k].copy() for k in keep])
            done += len(sc)
            if code == 0:
                break
        assert done == n, (done, n)
        t += n
    tabs = None if read is None else read(mdl)
    state = mdl.md_state()
    if not record:
        return tabs, None, np.array(rows), state
    kept = [np.concatenate(k) for k in zip(*kept)]
    return tabs, (kept[0] if len(keep) == 1 else tuple(kept)), np.array(rows), state


class Acc:
    """One accumulator, as the shared bodies need it.  name: "msd" for sgpr_md_msd, md_msd, md_msd_table and run_md(msd=);
    noun, moving_cell, polymer: as the messages spell them; raw(h, **over): the library's attach with valid default arguments;
    detach(h), read(h): the library's detach and its read with null pointers; py(mdl): the Python attach with minimal arguments;
    invalid: argument sets that are SGPR_E_INVALID — dicts for raw, or (dict, words of the message), or a callable that returns
    the list; limits(c), modes(c): the accumulator's own refusals, run on a begun run behind the bad arguments and between the
    polymer and the committee (c: the names refusals() works with); port, ports: the two-rank test's port base and how many
    ports from it on it may take; run(fr, args, **kw), twin(fr, args, kept) and same(tab, want, what): the module's _run, its
    twin's table and its comparison."""

    def __init__(self, name, limits=None, modes=None, ports=40, **fields):
        self.name, self.fn, self.ports = name, b"sgpr_md_" + name.encode(), ports
        self.limits = limits or (lambda c: None)
        self.modes = modes or (lambda c: None)
        self.__dict__.update(fields)

    def attach(self, mdl, args):
        getattr(mdl, "md_" + self.name)(*args)

    def table(self, mdl):
        return getattr(mdl, f"md_{self.name}_table")()


def refusals(acc):
    """No run, bad arguments, a run without the accumulator, the accumulator's own limits; a barostat, a relaxation, a band, a
    polymer and a committee, each in both orders with both message texts; a started run, without and with the accumulator; and
    the handle predicts the energy it predicted and runs the plain run it ran."""
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    from test_hip_neb_device import _band
    from test_hip_pimd_device import _begin as _begin_pimd, _polymer
    mdl, lib = _shared()[0], _lib.load()
    fr = _frame()
    numbers, pos, cell, pbc, mass, vel = fr
    h, fn = mdl.handle, acc.fn
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    rows = run(fr, cuts=(4,), record=False, seed=77)[2]
    UNS, INV = _lib.E_UNSUPPORTED, _lib.E_INVALID

    def raw(**over):
        return acc.raw(h, **over)

    def words(w):
        assert w in lib.sgpr_last_error(), lib.sgpr_last_error()

    def invalid():
        for bad in acc.invalid() if callable(acc.invalid) else acc.invalid:
            bad, figure = bad if isinstance(bad, tuple) else (bad, b"")
            assert raw(**bad) == INV, bad
            words(figure)

    def excluded(mode, call, because, mode_first=None, **kw):
        """The accumulator, then the mode: the mode is refused; the mode, then the accumulator: the accumulator is."""
        _begin(mdl, fr, **kw)
        assert raw() == 0 and call() == UNS
        words(b"sgpr_md_" + mode + b": the run accumulates " + acc.noun)
        if mode_first is None:
            _begin(mdl, fr, **kw)
            assert call() == 0
        else:
            mode_first()
        assert raw() == UNS
        words(fn + b": the run " + because)
    c = SimpleNamespace(mdl=mdl, lib=lib, h=h, fr=fr, raw=raw, read=lambda: acc.read(h), words=words, UNS=UNS, INV=INV)
    mdl.md_end()
    assert raw() == INV and acc.read(h) == INV                                          # no run
    _begin(mdl, fr, seed=77)
    invalid()
    assert acc.read(h) == INV                                                           # a run without the accumulator
    words(b"call sgpr_md_begin and " + fn + b" first")
    acc.limits(c)
    ext = np.array([-GPA] * 3 + [0.0] * 3)
    excluded(b"barostat", lambda: lib.sgpr_md_barostat(h, (100.0 * FS) ** 2 * 30.0 * GPA, _lib.ptr(ext), None, 1.0),
             b"has a barostat; " + acc.moving_cell, nh=True)
    excluded(b"relax", lambda: lib.sgpr_md_relax(h, 0.05, None, 0, None), b"is a relaxation")
    invalid()                                       # (each bad argument is SGPR_E_INVALID ahead of the mode refusals)
    assert raw() == UNS
    words(fn + b": the run is a relaxation")
    band = np.ascontiguousarray(_band(pos, 1))
    excluded(b"neb", lambda: lib.sgpr_md_neb(h, 1, _lib.ptr(band[1:2]), 0.05, 0.1, 0, None), b"is a nudged elastic band",
             mode_first=lambda: mdl.neb_begin(numbers, band, cell, pbc, 0.05))
    _, beads, bvel, _ = _polymer(numbers, pos, 2)
    excluded(b"pimd", lambda: lib.sgpr_md_pimd(h, 2, _lib.ptr(np.ascontiguousarray(beads)), _lib.ptr(np.ascontiguousarray(bvel)), kB * T, 0.001, 1.0),
             b"is a ring polymer (sgpr_md_pimd); its " + acc.polymer + b" not sampled",
             mode_first=lambda: _begin_pimd(mdl, numbers, beads, bvel, mass, cell, pbc, seed=7))
    acc.modes(c)
    member, _ = _model(seed=2)
    arr = (C.c_void_p * 1)(member.handle.value)
    excluded(b"committee", lambda: lib.sgpr_md_committee(h, 1, arr), b"has a committee")
    with pytest.raises(NotImplementedError, match="committee"):
        acc.py(mdl)
    mdl.md_end()
    member.close()
    # a run that has started, without the accumulator and with it; a detach is always taken, frees, and the run goes on
    for early in (False, True):
        _begin(mdl, fr, seed=77)
        assert not early or raw() == 0
        sc, code = mdl.md_run(2, None)
        assert code == 0 and raw() == INV
        words(fn + b": the run has started")
        assert acc.detach(h) == 0 and acc.read(h) == INV
    sc, code = mdl.md_run(2, None)
    assert code == 0
    # the handle works: the energy it predicted, the plain run it ran
    assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0
    assert np.array_equal(run(fr, cuts=(4,), record=False, seed=77)[2], rows)


def _two_rank_worker(rank, world, port, q, name, over):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd import _lib
    from autoforce_amd.watchdog import Watchdog
    acc = importlib.import_module(f"test_hip_{name}_device").ACC
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"{acc.noun.decode()} on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = acc.raw(mdl.handle, **over)
        msg = bytes(_lib.load().sgpr_last_error())
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1, msg))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def two_rank_refusal(acc, **over):
    """The accumulators run on one rank (test_hip_record_device.py's two-rank refusal): a run begun on two refuses the attach
    (acc.raw with `over`, which must not need the shared model: the workers have their own) and the handle goes on working."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = acc.port + (os.getpid() % acc.ports)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q, acc.name, over)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, e0, e1, msg in got:
        assert code == _lib.E_UNSUPPORTED and e0 == e1 and acc.fn + b": the run was begun on 2 ranks; " + acc.noun in msg, msg
    assert got[0][2] == got[1][2]


def moves_nothing(acc, nh, args, sampled, record=False):
    """With the accumulator `args` the scalar rows, the final state and (record) the recorded frames have the bits of the run
    without it; sampled(table): what the table must show of the 20 evaluations."""
    fr = _frame()
    _, xs0, rows0, st0 = acc.run(fr, None, cuts=(9, 11), nh=nh, record=record)
    tab, xs1, rows1, st1 = acc.run(fr, args, cuts=(9, 11), nh=nh, record=record)
    print(f"nh {nh}: count {list(tab.get('count', []))} samples {tab['samples']}, E of the last row without / with {rows0[-1, 0]!r} / {rows1[-1, 0]!r}")
    assert sampled(tab) and np.array_equal(rows0, rows1) and (not record or np.array_equal(xs0, xs1))
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st0[key], st1[key]), key


def first_halt(rows, evals):
    """The first evaluation k whose covloss (column 11) exceeds every earlier one, and an ediff between the two: the gate fires
    at k and nowhere before it."""
    b = rows[:, 11]
    ks = [k for k in range(2, evals - 2) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    print(f"halt at evaluation {k} of {evals}: covloss {b[k]:.6e} over {b[:k].max():.6e}")
    return k, 0.5 * (b[:k].max() + b[k])


def halt_counts_once(acc, args, halted, repeated=None, evals=24):
    """The gate fires at evaluation k inside a call: k has been sampled (its halt is known one evaluation late), the speculative
    evaluation k + 1 behind it must stay out, and the repeat of k — the model unchanged, resumed as device_loop.batches resumes:
    one ungated evaluation, then on — must not count again.  halted(mid, k, xs): what the table behind the halt must show;
    repeated(again, mid): the table behind the repeat against it."""
    fr = _frame()
    want, xs, rows, _ = acc.run(fr, args, cuts=(evals,), seed=77)
    k, ediff = first_halt(rows, evals)
    mdl = _shared()[0]
    _begin(mdl, fr, seed=77)
    acc.attach(mdl, args)
    sc, code = mdl.md_run(evals, None, ediff=ediff)
    assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
    mid = acc.table(mdl)
    assert mid["next_due"] == k + 1
    halted(mid, k, xs)
    sc1, code = mdl.md_run(1, None, ediff=0.0)
    again = acc.table(mdl)
    assert code == 0 and len(sc1) == 1 and again["next_due"] == k + 1
    if repeated is not None:
        repeated(again, mid)
    sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
    assert code == 0 and np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows)
    acc.same(acc.table(mdl), want, f"halt at {k}")
    acc.same(want, acc.twin(fr, args, xs), "the run that never halted")


def later_run_and_memory(acc, accumulate, detach):
    """The test_hip_md_restart.py rule on a model of the test's own: a plain run behind accumulator runs — accumulate(mdl, fr)
    — is the run on a fresh handle; the table is the run's (the read refuses the plain run); detach(mdl, fr, first) checks what a
    detach gives back and leaves the accumulator attached to a begun run, whose end gives the tables back and close() every byte."""
    from autoforce_amd import _lib
    from test_hip_teardown import _live
    fr = _frame()                     # (the shared model is alive before the first reading)
    before = _live()
    mdl, _ = _model()

    def plain():
        _begin(mdl, fr, seed=7)
        out = [mdl.md_run(n, None, final=f) for n, f in ((2, False), (4, True))]
        assert all(code == 0 for _, code in out)
        return np.concatenate([sc for sc, _ in out]), mdl.md_state(results=True)
    first = plain()
    accumulate(mdl, fr)
    again = plain()
    assert np.array_equal(first[0], again[0])
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(first[1][key]), np.asarray(again[1][key])), key
    assert acc.read(mdl.handle) == _lib.E_INVALID
    assert b"call sgpr_md_begin and " + acc.fn + b" first" in _lib.load().sgpr_last_error()
    detach(mdl, fr, first)
    mdl.md_end()                      # (the accumulator's buffers go with the run)
    mdl.close()
    assert np.array_equal(_live() - before, [0, 0])


def run_md_host_and_device(tmp_path, name, holder_of, seen=None, steps=40):
    """ActiveCalculator.run_md(<name>=holder_of(cell)) with a teacher — the gate fires, calculate() updates the model, the run
    goes on — through the host loop (the twin fed every step) and on the device (the accumulator inside the loop): the same
    trajectory (rng= given), the same updates.  seen(mode, o, atoms, cell, holder): called with everything run_md yields.
    Returns ([the host's table, the device's], the device's holder, numbers)."""
    import active_common as ac
    from autoforce_amd import SGPRModel
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.calculator import ActiveCalculator
    from helpers import PairTeacher
    tabs, upd = [], []
    for mode in ("host", "device"):
        np.random.seed(1234)
        rng0, numbers, pos, cell = ac.start(0)
        d = tmp_path / mode
        d.mkdir()
        calc = ActiveCalculator(engine=SGPRModel(3, 3, 4, 4.5, species=ac.SPECIES), calculator=PairTeacher(rc=4.0),
                                logfile=str(d / "active.log"), pckl=None, tape=None, **ac.KW)
        if mode == "host":
            calc.md_on_device_ok = lambda: False
        at = Atoms(numbers, pos, cell, True, velocities=0.02 * np.random.default_rng(3).normal(size=pos.shape))
        holder = holder_of(cell)
        out = []
        for o in calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.02, rng=np.random.default_rng(9), chunk=16, **{name: holder}):
            out.append(o)
            if seen is not None:
                seen(mode, o, at, cell, holder)
        assert len(out) == steps + 1
        upd.append([o[0] for o in out if o[3]])
        tabs.append(holder.table())
        calc.engine.close()
    print(f"updates at steps {upd}")
    assert upd[0] == upd[1] and len(upd[0]) >= 1, upd        # (the device loop halted and went on)
    return tabs, holder, numbers
