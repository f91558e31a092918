"""GPU tests of the frame record of the device loops (sgpr_md_record / sgpr_md_frame_count / sgpr_md_frames; md_record_kernel
behind a recorded evaluation): a run that is NOT cut shows every `every`-th configuration.  The yardstick is always the cut
path the project had before: a fresh run of the same inputs without recording, one md_run(1) per evaluation and
sgpr_md_state(which = -1) with the packed results behind each (which = 0 behind a `final` one) — tests/test_hip_md.py
establishes that a trajectory does not depend on how the run is cut.  A frame is a copy: every comparison is np.array_equal.
Frame and model are those of test_hip_npt_device.py (LiPS, side 8, m = 48)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_hip_npt_device import _model

pytestmark = pytest.mark.gpu

T = 600.0
EVALS, CALLS = 16, (5, 7, 4)
FMAX = 1e-9   # (nothing converges in sixteen evaluations)
KINDS = ["langevin-seeded", "langevin-host", "verlet", "nose-hoover", "npt", "fire", "fire-cell", "langevin-fixed", "fire-fixed"]


@functools.lru_cache(maxsize=None)
def _shared():
    """One model for the module (a run begins from scratch with every md_begin / relax_begin)."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS
    mdl, (numbers, pos, cell, pbc) = _model()
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return mdl, (numbers, pos, cell, pbc, mass, vel)


def _system(N=None):
    """The module's frame, or N of the atoms of a larger one (test_hip_relax_device.test_frames_off_the_kernels_grids' frames)."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import MASS, lips
    mdl, frame = _shared()
    if N is None:
        return mdl, frame
    numbers, pos, cell, pbc = lips(17 if N > 512 else 8, seed=0)
    if N == 5:
        keep = np.sort(np.argsort(np.linalg.norm(pos - pos[len(pos) // 2], axis=1))[:N])
    else:
        keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=N, replace=False))
    numbers, pos = numbers[keep], pos[keep]
    mass = np.array([MASS[int(z)] for z in numbers])
    vel = np.random.default_rng(3).normal(size=pos.shape) * np.sqrt(kB * T / mass)[:, None]
    return mdl, (numbers, pos, cell, pbc, mass, vel)


def _begin(kind, N=None, fmax=FMAX):
    """A fresh run of `kind`; returns (model, is a relaxation, has cells, rows of host deviates or None)."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    from fixed_common import mask
    mdl, (numbers, pos, cell, pbc, mass, vel) = _system(N)
    n = len(numbers)
    hold = dict(fixed=mask(n)) if kind.endswith("-fixed") else {}
    noise = None
    if kind.startswith("fire"):
        mdl.relax_begin(numbers, pos, cell, pbc, fmax, cell_relax=(kind == "fire-cell"), **hold)
        return mdl, True, True, None
    kw = dict(dt=1.0 * FS, kT=kB * T)
    if kind in ("langevin-seeded", "langevin-fixed"):
        kw.update(friction=0.05, seed=77)
    elif kind == "langevin-host":
        kw.update(friction=0.05)
        noise = np.random.default_rng(9).normal(size=(EVALS, n, 3))
    elif kind == "verlet":
        kw.update(friction=0.0)
    else:
        kw.update(friction=0.0, ttime=25.0 * FS)
        if kind == "npt":
            kw.update(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, **kw, **hold)
    return mdl, False, kind == "npt", noise


def _raw_state(mdl, which):
    """sgpr_md_state itself: positions, velocities_pre, packed."""
    from autoforce_amd import _lib
    N = mdl._md["N"]
    x, v, p = np.empty((N, 3)), np.empty((N, 3)), np.empty(4 * N + 11)
    pend = C.c_int(0)
    _lib.check(_lib.load().sgpr_md_state(mdl.handle, _lib.ptr(x), _lib.ptr(v), C.addressof(pend), _lib.ptr(p), int(which)))
    return x, v, p


@functools.lru_cache(maxsize=None)
def _cut(kind, evals=EVALS, N=None):
    """The yardstick: one md_run(1) per evaluation, the last one `final`, the state read behind each.  Computed once per kind."""
    mdl, relax, has_cells, noise = _begin(kind, N)
    out = dict(x=[], v=[], p=[], cell=[], aux=[], sc=[])
    for e in range(evals):
        final = e == evals - 1
        sc, code = mdl.md_run(1, None if noise is None else noise[e:e + 1], final=final)
        assert code == 0 and len(sc) == 1, (kind, e, code)
        x, v, p = _raw_state(mdl, 0 if final else -1)
        out["x"].append(x); out["v"].append(v); out["p"].append(p); out["sc"].append(sc[0])
        if has_cells:
            c, a = mdl.md_cells()
            out["cell"].append(c[0]); out["aux"].append(a[0])
    out = {k: np.array(v) for k, v in out.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def _recorded(kind, every, calls=CALLS, evals=EVALS, N=None, what=(True, True)):
    """The same run in `calls`, recording: the frames of every call, its scalars and its cells."""
    mdl, relax, has_cells, noise = _begin(kind, N)
    mdl.md_record(every, velocities=what[0], results=what[1])
    frames, rows, cells, t = [], [], [], 0
    for n in calls:
        final = t + n == evals
        sc, code = mdl.md_run(n, None if noise is None else noise[t:t + n], final=final)
        assert code == 0 and len(sc) == n, (kind, code, len(sc), n)
        want = [i for i in range(t, t + n) if i % every == 0]
        assert mdl.md_frame_count() == len(want)
        if want:
            fr = mdl.md_frames()
            assert list(fr["index"]) == want
            frames.append(fr)
        if has_cells:
            cells.extend(mdl.md_cells()[0])
        rows.extend(sc)
        t += n
    keys = frames[0].keys()
    return {k: np.concatenate([f[k] for f in frames]) for k in keys}, np.array(rows), np.array(cells)


def _same_frames(fr, cut, has_cells, relax):
    idx = fr["index"]
    N = fr["positions"].shape[1]
    assert np.array_equal(fr["positions"], cut["x"][idx])
    assert np.array_equal(fr["velocities_pre"], cut["v"][idx])
    packed = np.concatenate([fr["forces"].reshape(len(idx), -1), fr["beta"], fr["energy"][:, None]], axis=1)
    assert np.array_equal(packed, cut["p"][idx][:, :4 * N + 1])
    if has_cells:
        assert np.array_equal(fr["cell"], cut["cell"][idx])
        assert np.array_equal(fr["D" if relax else "eta"], cut["aux"][idx])


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_frames_equal_the_cut_run(kind, every):
    from autoforce_amd import _lib
    cut = _cut(kind)
    fr, rows, cells = _recorded(kind, every)
    mdl = _shared()[0]
    relax, has_cells = kind.startswith("fire"), kind.startswith("fire") or kind == "npt"
    assert list(fr["index"]) == list(range(0, EVALS, every))            # the multiples of `every`, once each
    _same_frames(fr, cut, has_cells, relax)
    # the packed results whole (virial and overflow word included), straight from the C entry point
    k, N = len(fr["index"]), fr["positions"].shape[1]
    # (the last call's frames only are still there)
    n_last = mdl.md_frame_count()
    p = np.empty((n_last, 4 * N + 11))
    idx = np.zeros(n_last, dtype=np.int64)
    _lib.check(_lib.load().sgpr_md_frames(mdl.handle, 0, n_last, _lib.ptr(idx), None, None, _lib.ptr(p)))
    assert np.array_equal(idx, fr["index"][k - n_last:]) and np.array_equal(p, cut["p"][idx])
    # stress: sgpr_stress_from_virial of the frame's own cell, as md_state(results=True) gives it
    stress = np.zeros(6)
    cell = np.ascontiguousarray(fr["cell"][-1] if has_cells else mdl._md["cell"])
    _lib.check(_lib.load().sgpr_stress_from_virial(_lib.ptr(np.ascontiguousarray(p[-1, 4 * N + 1:4 * N + 10])), _lib.ptr(cell), _lib.ptr(stress)))
    assert np.array_equal(fr["stress"][-1], stress)
    if kind.startswith("langevin") or kind == "verlet":
        # the closed velocity in md_state(results=True)'s expression, held components zero
        i = int(fr["index"][-1])
        v = cut["v"][i] + mdl._md["hdt"] * cut["p"][i][:3 * N].reshape(N, 3) / mdl._md["masses"][:, None] if i > 0 else cut["v"][i]
        if mdl._md.get("fixed") is not None:
            v = np.where(mdl._md["fixed"], 0.0, v)
            assert np.array_equal(fr["velocities"][:, mdl._md["fixed"]], np.zeros((k, int(mdl._md["fixed"].sum()))))
        assert np.array_equal(fr["velocities"][-1], v)
    else:
        assert "velocities" not in fr
    if has_cells:
        assert np.array_equal(cells, cut["cell"])
    assert np.array_equal(rows, cut["sc"])                              # recording moves nothing


@pytest.mark.parametrize("kind", ["langevin-seeded", "fire"])
@pytest.mark.parametrize("N", [4099, 5])
def test_frames_off_the_kernels_grids(N, kind):
    """N = 4099 and N = 5: no multiple of the copy kernel's workgroup nor of a wave, and a permutation that is not the identity."""
    mdl, _ = _system(N)
    cut = _cut(kind, 12, N)
    fr, rows, _ = _recorded(kind, 1, calls=(5, 7), evals=12, N=N)
    if N > 5:   # (the species sort moves atoms)
        assert not np.array_equal(np.argsort(mdl._md["numbers"], kind="stable"), np.arange(N))
    assert list(fr["index"]) == list(range(12))
    _same_frames(fr, cut, kind == "fire", kind == "fire")
    assert np.array_equal(rows, cut["sc"])


def test_a_covloss_halt_leaves_its_frame_to_the_next_call():
    """The gate fires inside a call at an evaluation k that would be recorded: the call's frames stop before k, the following
    one-evaluation call records k exactly once, with its own results."""
    kind = "langevin-seeded"
    cut = _cut(kind)
    b = cut["sc"][:, 11]
    ks = [k for k in range(2, EVALS - 1) if b[k] > b[:k].max()]
    assert ks, "the covloss never exceeds its earlier values on this walk"
    k = ks[0]
    every = 2 if k % 2 == 0 else (3 if k % 3 == 0 else 1)
    ediff = 0.5 * (b[:k].max() + b[k])
    mdl, *_ = _begin(kind)
    mdl.md_record(every)
    sc, code = mdl.md_run(EVALS, None, ediff=ediff)
    assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
    want = [i for i in range(k) if i % every == 0]
    assert mdl.md_frame_count() == len(want)
    fr = mdl.md_frames()
    assert list(fr["index"]) == want
    _same_frames(fr, cut, False, False)
    sc, code = mdl.md_run(1, None, ediff=0.0)
    assert code == 0 and len(sc) == 1 and mdl.md_frame_count() == 1
    fr = mdl.md_frames()
    assert list(fr["index"]) == [k]
    x, v, p = _raw_state(mdl, -1)
    N = len(x)
    assert np.array_equal(fr["positions"][0], x) and np.array_equal(fr["velocities_pre"][0], v)
    assert np.array_equal(fr["forces"][0], p[:3 * N].reshape(N, 3)) and fr["energy"][0] == p[4 * N] == sc[0, 0]
    _same_frames(fr, cut, False, False)                                   # (the model has not changed in between)


def test_a_converged_relaxation_keeps_its_last_frame():
    kind = "fire"
    cut = _cut(kind)
    g = np.sqrt(cut["sc"][:, 12])
    ks = [k for k in range(3, EVALS - 1) if g[k] < g[:k].min()]
    assert ks, "no evaluation undercuts all earlier ones on this walk"
    k = ks[0]
    fmax = 0.5 * (g[k] + g[:k].min())
    mdl, *_ = _begin(kind, fmax=fmax)
    mdl.md_record(1)
    sc, code = mdl.md_run(EVALS, None)
    assert code == 3 and len(sc) == k + 1, (code, len(sc), k)
    assert mdl.md_frame_count() == k + 1
    fr = mdl.md_frames()
    assert list(fr["index"]) == list(range(k + 1))
    assert np.array_equal(fr["positions"], cut["x"][:k + 1]) and np.array_equal(fr["energy"], cut["sc"][:k + 1, 0])
    assert np.array_equal(fr["velocities_pre"][:k], cut["v"][:k])
    x, v, p = _raw_state(mdl, 0)                                          # the final structure: nothing moved out of it
    assert np.array_equal(fr["positions"][k], x) and np.array_equal(fr["velocities_pre"][k], v)
    assert np.array_equal(fr["forces"][k].ravel(), p[:3 * len(x)])


def test_a_call_that_records_nothing_has_no_frames():
    from autoforce_amd import _lib
    kind = "langevin-seeded"
    cut = _cut(kind)
    mdl, *_ = _begin(kind)
    sc, code = mdl.md_run(1, None)
    mdl.md_record(100)
    sc, code = mdl.md_run(3, None)                                        # configurations 1, 2, 3
    assert code == 0 and mdl.md_frame_count() == 0
    with pytest.raises(_lib.SgprError) as err:
        mdl.md_frames()
    assert err.value.code == _lib.E_INVALID
    mdl.md_record(1)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and np.array_equal(sc, cut["sc"][4:6])
    fr = mdl.md_frames()
    assert list(fr["index"]) == [4, 5]
    _same_frames(fr, cut, False, False)


def test_switching_between_calls():
    from autoforce_amd import _lib
    kind = "langevin-seeded"
    cut = _cut(kind)
    mdl, *_ = _begin(kind)
    lib = _lib.load()
    N = mdl._md["N"]
    mdl.md_record(1)
    mdl.md_run(3, None)
    assert list(mdl.md_frames()["index"]) == [0, 1, 2]
    mdl.md_record(0)                                                      # off: nothing is recorded
    mdl.md_run(3, None)
    assert mdl.md_frame_count() == 0
    mdl.md_record(2, velocities=False, results=False)                     # on again, on the right indices, positions only
    sc, code = mdl.md_run(4, None)                                        # configurations 6 ... 9
    assert np.array_equal(sc, cut["sc"][6:10])
    fr = mdl.md_frames()
    assert sorted(fr) == ["index", "positions"] and list(fr["index"]) == [6, 8]
    assert np.array_equal(fr["positions"], cut["x"][[6, 8]])
    p, v = np.empty((2, 4 * N + 11)), np.empty((2, N, 3))
    assert lib.sgpr_md_frames(mdl.handle, 0, 2, None, None, None, _lib.ptr(p)) == _lib.E_INVALID
    assert lib.sgpr_md_frames(mdl.handle, 0, 2, None, None, _lib.ptr(v), None) == _lib.E_INVALID
    assert lib.sgpr_md_frames(mdl.handle, 1, 2, None, None, None, None) == _lib.E_INVALID    # beyond the record
    mdl.md_record(3, velocities=True, results=False)
    sc, code = mdl.md_run(3, None)                                        # 10, 11, 12
    fr = mdl.md_frames()
    assert list(fr["index"]) == [12] and np.array_equal(fr["velocities_pre"], cut["v"][[12]]) and "forces" not in fr


def test_errors_leave_the_handle_working():
    from autoforce_amd import _lib
    kind = "langevin-seeded"
    cut = _cut(kind)
    mdl, (numbers, pos, cell, pbc, mass, vel) = _shared()
    lib = _lib.load()
    e0 = float(mdl.predict(numbers, pos, cell, pbc)["energy"])
    mdl.md_end()
    assert lib.sgpr_md_record(mdl.handle, 1, 3) == _lib.E_INVALID         # before sgpr_md_begin
    k = C.c_int(0)
    assert lib.sgpr_md_frame_count(mdl.handle, C.addressof(k)) == _lib.E_INVALID
    assert lib.sgpr_md_frames(mdl.handle, 0, 1, None, None, None, None) == _lib.E_INVALID
    assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0
    mdl, *_ = _begin(kind)
    assert lib.sgpr_md_record(mdl.handle, -1, 3) == _lib.E_INVALID        # every < 0
    assert lib.sgpr_md_record(mdl.handle, 1, 4) == _lib.E_INVALID         # unknown bits
    assert lib.sgpr_md_record(mdl.handle, 1, 7) == _lib.E_INVALID
    sc, code = mdl.md_run(4, None)                                        # a plain run goes on, nothing recorded
    assert code == 0 and np.array_equal(sc, cut["sc"][:4]) and mdl.md_frame_count() == 0
    assert float(mdl.predict(numbers, pos, cell, pbc)["energy"]) == e0


def _two_rank_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd import _lib
    from autoforce_amd.watchdog import Watchdog
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"frame record on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _model()
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        code = _lib.load().sgpr_md_record(mdl.handle, 1, 3)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, code, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_record_and_goes_on_working():
    """Frames are recorded on one rank: sgpr_md_record says SGPR_E_UNSUPPORTED on every rank and the handles go on predicting."""
    import torch.multiprocessing as mp
    from autoforce_amd import _lib
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + (os.getpid() % 40)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, e0, e1 in got:
        assert code == _lib.E_UNSUPPORTED and e0 == e1
    assert got[0][2] == got[1][2]
