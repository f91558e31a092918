"""GPU: the Bayesian committee inside the device MD loop (sgpr_md_committee, csrc/md_bcm.inc) — the combination of every
evaluation against calculator_bcm's rule applied in numpy to the members' own predict(), the four integrators against their host
twins around the same BCMActiveCalculator, the gate on the member-wise minimum covloss, determinism, `final`, detaching, the
refusals, and BCMActiveCalculator.run_md through it.
System 1: the 40-atom g5_big40 frame (2 x 16 + 8: a partial 16-row tail) with the g12_bcm models "a" and "live".
System 2: 343 atoms (LiPS 7 x 7 x 7: 21 x 16 + 7, 256 + 87 — the one-workgroup reductions stride 256) with two models that
differ in their inducing subsets."""
import numpy as np
import pytest

import bcm_md_common as bc

pytestmark = pytest.mark.gpu

# The twin tolerance ("The committee loop"): max |dx| (Angstrom) and max |dE| / |E| between the device loop and the
# host twin around BCMActiveCalculator after 8 steps.  The rule: ten times the value measured on an MI355X, never looser than
# 1e-9 A / 1e-9 |E|.  TWIN_MEASURED holds the measured pairs: every one is 0 — on the MI355X the device loop and the host
# twin agreed bit for bit in every energy and every final coordinate (the members' evaluations are the same bits on both
# sides, and the device's log gave the weights numpy's gave).  Ten times 0 would assert bit equality with one build of
# numpy's log, so a measured 0 is asserted as 16 ulp of the largest coordinate / of |E| (FLOOR).  None = not measured: the
# bound is then the reasoned one.  The reasoning: the two sides run the same member evaluations on the same bits and differ only in the last bits of the
# weights (the device's log against numpy's: <= 2 ulp of w), so a combined force differs by a few ulp of max |F| and an energy
# by a few ulp of |E| per evaluation; a position inherits dt^2 / m times the force error (far below its own ulp) plus its own
# roundings, so after 8 steps the sides are a few ulp of the largest coordinate apart (ulp(12.6 A) = 1.8e-15 A; system 2:
# ulp(21 A) = 3.6e-15) unless a rounding flips, which the dynamics amplify by less than 1 + dt^2 k / m ~ 1.01 per step.
# REASONED = 1e-12 A and 1e-12 |E| is some 300 ulp: room for that, and a thousand times tighter than the cap.
TWIN_MEASURED = {"langevin_rows": (0.0, 0.0), "langevin_seeded": (0.0, 0.0), "verlet": (0.0, 0.0), "nose_hoover": (0.0, 0.0),
                 "verlet_sys2": (0.0, 0.0)}
REASONED = (1e-12, 1e-12)
FLOOR = (16 * 3.6e-15, 16 * 2.3e-16)


def _twin_bounds(kind):
    got = TWIN_MEASURED[kind]
    if got is None:
        return REASONED
    return tuple(min(max(10.0 * v, f), 1e-9) for v, f in zip(got, FLOOR))


def _hip_engine():
    from autoforce_amd import SGPRModel
    from helpers import load
    g = load("g5_big40")
    return SGPRModel(int(g["lmax"]), int(g["nmax"]), float(g["eta"]), float(g["rc"]), species=g["species"].tolist())


class System:
    def __init__(self, members, live, frame, vel):
        from autoforce_amd.workloads import MASS
        self.members, self.live = members, live
        self.numbers, self.pos, self.cell, self.pbc = frame
        self.N = len(self.numbers)
        self.mass = np.array([MASS[int(z)] for z in self.numbers])
        self.vel = vel

    def begin(self, committee=True, dt_fs=1.0, friction=0.0, temperature=300.0, seed=0, ttime_fs=None, **kw):
        from autoforce_amd.ase_shim import kB
        from autoforce_amd.workloads import FS
        self.live.md_begin(self.numbers, self.pos, self.cell, self.pbc, self.mass, self.vel, dt=dt_fs * FS, friction=friction,
                           kT=kB * temperature, seed=seed, ttime=None if ttime_fs is None else ttime_fs * FS, **kw)
        if committee:
            self.live.md_committee(self.members)

    def outs(self, positions):
        """Every member's own predict() at `positions`, the live model last."""
        return [m.predict(self.numbers, positions, self.cell, self.pbc, beta=True) for m in self.members + [self.live]]


@pytest.fixture(scope="module")
def sys1():
    posts, g = bc.g12_posts(_hip_engine)
    s = System([posts["a"].engine], posts["live"].engine, (g["numbers"], g["positions"], g["cell"], g["pbc"]), bc.thermal_velocities(g["numbers"]))
    s.posts = posts
    yield s
    for m in s.members + [s.live]:
        m.close()


@pytest.fixture(scope="module")
def sys2():
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, lips
    numbers, pos, cell, pbc = lips(7, seed=0)
    assert len(numbers) == 343
    species = sorted(set(int(z) for z in numbers))
    models = []
    for m, seed in ((40, 1), (48, 2)):   # (two inducing subsets, drawn from two other frames)
        mdl = SGPRModel(3, 3, 4, 6.0, species=species)
        n2, p2, c2, b2 = lips(7, seed=seed)
        mdl.set_inducing(inducing_from_frame(mdl, n2, p2, c2, b2, m, seed=seed))
        rng = np.random.default_rng(2 + seed)
        mdl.solve(rng.normal(size=(64, m)), rng.normal(size=64))
        mdl.set_weights(0.02 * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
        models.append(mdl)
    from autoforce_amd.posterior import PosteriorPotential
    s = System([models[0]], models[1], (numbers, pos, cell, pbc), bc.thermal_velocities(numbers))
    s.posts = {"a": PosteriorPotential(models[0]), "live": PosteriorPotential(models[1])}
    yield s
    for m in models:
        m.close()


def _check_combination(s, st, w, cm, row=None):
    """Packed F, E, stress, beta of a state against the rule applied to the members' predict() at its positions."""
    ref = bc.committee_rule(s.outs(st["positions"]))
    fmax = np.abs(ref["forces"]).max()
    dF = np.abs(st["forces"] - ref["forces"]).max()
    dE = abs(st["energy"] - ref["energy"])
    dS = np.abs(st["stress"] - ref["stress"]).max()
    dB = np.abs(st["beta"] - ref["beta"]).max()
    print(f"combination N={s.N}: dF {dF:.3e} (max|F| {fmax:.3e})  dE {dE:.3e} (|E| {abs(ref['energy']):.3e})  dS {dS:.3e}  dbeta {dB:.3e}  w {w}")
    assert dF <= 1e-8 * fmax
    assert dE <= 1e-8 * abs(ref["energy"])
    assert dS <= 1e-8 * np.abs(ref["stress"]).max()
    assert dB <= 2e-6
    assert np.abs(cm - ref["covmax"]).max() <= 2e-6
    assert np.abs(w - bc.weights_of(cm)).max() <= 1e-12     # the rule applied to the device's own covmax
    assert abs(w.sum() - 1.0) <= 1e-15
    if row is not None:
        assert row[0] == st["energy"] and row[11] == st["beta"].max() and row[10] == 0.0
    return ref


@pytest.mark.parametrize("which", ["sys1", "sys2"])
def test_combination_of_an_evaluation(which, request):
    s = request.getfixturevalue(which)
    s.begin()
    sc, code = s.live.md_run(1, None, final=True)
    assert code == 0 and len(sc) == 1
    st = s.live.md_state(results=True)
    w, cm = s.live.md_committee_info()
    assert np.array_equal(st["positions"], s.pos)
    ref = _check_combination(s, st, w, cm, sc[0])
    # (neither fixture produces a member with covmax >= 1 — the one a committee excludes with weight 0 —: every member weighs in)
    assert 0.0 < w[0] < 1.0 and (ref["covmax"] < 1.0).all()
    # ... and of an evaluation inside a batch, behind two velocity-Verlet moves
    s.begin()
    sc, code = s.live.md_run(3, None, final=True)
    assert code == 0 and len(sc) == 3
    st = s.live.md_state(results=True)
    assert not np.array_equal(st["positions"], s.pos)
    _check_combination(s, st, *s.live.md_committee_info(), sc[2])
    ke = float((s.mass[:, None] * st["velocities"] ** 2).sum())
    assert abs(sc[2][12] - ke) <= 1e-12 * ke


def _calculator(s):
    from autoforce_amd.calculator_bcm import BCMActiveCalculator
    return BCMActiveCalculator(covariance=s.posts["live"], kernel_model_dict={"a": s.posts["a"]}, logfile=None)


class _Rows:
    """A stand-in generator that hands out prepared rows of deviates, one per normal() call."""
    def __init__(self, rows):
        self.rows, self.k = rows, 0

    def normal(self, size=None):
        self.k += 1
        return self.rows[self.k - 1].reshape(size)


def _compare_with_twin(kind, dev_E, dev_x, twin):
    dx = max(np.abs(dev_x - twin[-1][1]).max(), 0.0)
    de = max(abs(a - b) / abs(b) for a, (b, _) in zip(dev_E, twin))
    bx, be = _twin_bounds(kind)
    print(f"twin {kind}: max|dx| {dx:.3e} A  max|dE|/|E| {de:.3e}  (asserted at {bx:.1e}, {be:.1e})")
    assert len(dev_E) == len(twin) == 9
    assert dx <= bx and de <= be


@pytest.mark.parametrize("kind", ["langevin_rows", "langevin_seeded", "verlet", "verlet_sys2"])
def test_trajectory_against_the_host_twin(kind, request):
    """8 steps against workloads.langevin_nvt around the same BCMActiveCalculator: system 1, and velocity Verlet on system 2."""
    from autoforce_amd.workloads import langevin_nvt
    s, steps = request.getfixturevalue("sys2" if kind.endswith("sys2") else "sys1"), 8
    friction = 0.0 if kind.startswith("verlet") else 0.05
    s.begin(friction=friction, seed=11 if kind == "langevin_seeded" else 0)
    if kind == "langevin_seeded":
        rows = s.live.md_deviates(0, steps)
        noise, rng = None, _Rows(rows)
    else:
        rows = np.random.default_rng(5).normal(size=(steps, s.N, 3))
        noise, rng = (None if kind.startswith("verlet") else np.concatenate([rows, np.zeros((1, s.N, 3))])), np.random.default_rng(5)
    sc, code = s.live.md_run(steps + 1, noise, final=True)
    assert code == 0 and len(sc) == steps + 1
    st = s.live.md_state(results=True)
    twin = [(E, p.copy(), v.copy()) for _, E, T, _, p, v in
            langevin_nvt(_calculator(s), s.numbers, s.pos, s.cell, s.pbc, steps, temperature=300.0, dt_fs=1.0, friction=friction, vel=s.vel, rng=rng)]
    _compare_with_twin(kind, sc[:, 0], st["positions"], [(E, p) for E, p, _ in twin])
    assert np.abs(st["velocities"] - twin[-1][2]).max() <= 1e-9 * np.abs(twin[-1][2]).max()


def test_nose_hoover_against_the_host_twin(sys1):
    from autoforce_amd.workloads import nose_hoover_nvt
    s, steps = sys1, 8
    s.begin(ttime_fs=25.0)
    sc, code = s.live.md_run(steps + 1, None, final=True)
    assert code == 0 and len(sc) == steps + 1
    st = s.live.md_state(results=True)
    twin = [(E, x.copy(), z) for _, E, T, _, x, v, z, zi in
            nose_hoover_nvt(_calculator(s), s.numbers, s.pos, s.cell, s.pbc, steps, temperature=300.0, dt_fs=1.0, tdamp_fs=25.0, vel=s.vel,
                            species=s.live.species)]
    _compare_with_twin("nose_hoover", sc[:, 0], st["positions"], [(E, x) for E, x, _ in twin])
    assert sc[0][14] == 0.0 and abs(sc[-1][14] - twin[-1][2]) <= 1e-9 * abs(twin[-1][2])


def _seeded_run(s, batches, committee=True, final=False):
    s.begin(committee=committee, friction=0.05, seed=7)
    rows = []
    for k, n in enumerate(batches):
        sc, code = s.live.md_run(n, None, final=final and k == len(batches) - 1)
        assert code == 0 and len(sc) == n
        rows.append(sc)
    st = s.live.md_state(results=final)
    return np.concatenate(rows), st


@pytest.mark.parametrize("which", ["sys1", "sys2"])
def test_batching_and_repeating_change_no_bit(which, request):
    """The device generator: 1 + 7 evaluations against 8, and the same run twice — positions, velocities, scalars."""
    s = request.getfixturevalue(which)
    a, sa = _seeded_run(s, [8])
    b, sb = _seeded_run(s, [1, 7])
    c, sc_ = _seeded_run(s, [8])
    for other, so in ((b, sb), (c, sc_)):
        assert np.array_equal(a, other)
        assert np.array_equal(sa["positions"], so["positions"]) and np.array_equal(sa["velocities_pre"], so["velocities_pre"])
    assert not np.array_equal(sa["positions"], s.pos)


def test_a_copy_of_the_live_model_as_member(sys1):
    """w is exactly [0.5, 0.5], and the forces are those of the plain single-model loop within the combination bound."""
    s = sys1
    posts, _ = bc.g12_posts(_hip_engine, keys=("live",))
    twin = posts["live"].engine
    try:
        s.begin(committee=False)
        s.live.md_committee([twin])
        sc, code = s.live.md_run(1, None, final=True)
        both = s.live.md_state(results=True)
        w, cm = s.live.md_committee_info()
        assert w.tolist() == [0.5, 0.5] and cm[0] == cm[1]
        s.begin(committee=False)
        sp, _ = s.live.md_run(1, None, final=True)
        plain = s.live.md_state(results=True)
    finally:
        s.live.md_end()
        twin.close()
    fmax = np.abs(plain["forces"]).max()
    assert np.abs(both["forces"] - plain["forces"]).max() <= 1e-8 * fmax
    assert abs(both["energy"] - plain["energy"]) <= 1e-8 * abs(plain["energy"])
    assert np.abs(both["beta"] - plain["beta"]).max() <= 2e-6


def test_the_gate_is_the_committees(sys1):
    """ediff just below the largest beta_tot of a chosen evaluation (from the members' predict()): the run halts there with code 1,
    nothing has moved, md_state returns that evaluation's committee results.  ediff between the largest beta_tot and the live
    model's own maximum: the committee runs on where the live-only loop halts."""
    s = sys1
    s.begin()
    xs, vs, bts = [], [], []
    for k in range(5):
        st = s.live.md_state()
        xs.append(st["positions"]); vs.append(st["velocities_pre"])
        bts.append(float(bc.committee_rule(s.outs(st["positions"]))["beta"].max()))
        sc, code = s.live.md_run(1, None)
        assert code == 0 and abs(sc[0][11] - bts[-1]) <= 2e-6
    # (the device's beta_tot and the one from predict() agree to the last bit here — asserted within 2e-6 above —, and the
    # largest beta_tot grows by ~2e-6 per step at 300 K: a margin of 1e-7 below the chosen evaluation, 4e-7 above the ones before)
    later = [k for k in range(1, 5) if bts[k] > max(bts[:k]) + 4e-7]
    k = later[0] if later else 0
    print(f"gate: beta_tot maxima {bts}, chosen evaluation {k}")
    s.begin()
    sc, code = s.live.md_run(6, None, ediff=bts[k] - 1e-7)
    assert code == 1 and len(sc) == k + 1 and np.abs(sc[:, 11] - bts[:k + 1]).max() <= 1e-7
    st = s.live.md_state(results=True)
    assert np.array_equal(st["positions"], xs[k]) and np.array_equal(st["velocities_pre"], vs[k])
    _check_combination(s, st, *s.live.md_committee_info(), sc[k])
    # the run goes on from there: the same configuration is evaluated again
    sc2, code = s.live.md_run(1, None, final=True)
    assert code == 0 and sc2[0][0] == sc[k][0]
    # between the committee's largest covloss and the live model's own
    outs = s.outs(s.pos)
    bt0, live0 = float(bc.committee_rule(outs)["beta"].max()), float(outs[-1]["beta"].max())
    assert live0 - bt0 > 1e-2, (bt0, live0)
    mid = 0.5 * (bt0 + live0)
    s.begin()
    sc, code = s.live.md_run(2, None, ediff=mid, final=True)
    assert code == 0 and len(sc) == 2 and sc[:, 11].max() < mid
    s.begin(committee=False)
    sc, code = s.live.md_run(2, None, ediff=mid, final=True)
    assert code == 1 and len(sc) == 1 and sc[0][11] >= mid


def test_final_moves_nothing_and_detaching_is_the_plain_loop(sys1):
    s = sys1
    rows_a, sa = _seeded_run(s, [2])                 # two moves: the state is configuration 2, not evaluated
    rows_b, sb = _seeded_run(s, [3], final=True)     # ... and evaluated, with nothing moved behind it
    assert np.array_equal(rows_a, rows_b[:2])
    assert np.array_equal(sa["positions"], sb["positions"]) and np.array_equal(sa["velocities_pre"], sb["velocities_pre"])
    _check_combination(s, sb, *s.live.md_committee_info(), rows_b[2])
    # K = 0 detaches: the run that never attached
    plain, sp = _seeded_run(s, [4], committee=False, final=True)
    s.begin(friction=0.05, seed=7)
    s.live.md_committee([])
    sc, code = s.live.md_run(4, None, final=True)
    sd = s.live.md_state(results=True)
    assert code == 0 and np.array_equal(sc, plain)
    for key in ("positions", "velocities_pre", "forces", "beta", "energy"):
        assert np.array_equal(sd[key], sp[key]), key
    with pytest.raises(Exception, match="sgpr_md_committee"):
        s.live.md_committee_info()


def _refused(code, match, call):
    from autoforce_amd._lib import SgprError
    with pytest.raises(SgprError, match=match) as e:
        call()
    assert e.value.code == code, e.value


UNSUPPORTED, INVALID = -6, -1


def test_refusals_unsupported(sys1):
    s, a, live = sys1, sys1.members[0], sys1.live
    s.begin(committee=False, ttime_fs=25.0, pfactor=1.0)
    _refused(UNSUPPORTED, "barostat", lambda: live.md_committee([a]))
    live.relax_begin(s.numbers, s.pos, s.cell, s.pbc, fmax=0.01)
    _refused(UNSUPPORTED, "relaxation", lambda: live.md_committee([a]))
    fixed = np.zeros(s.N, bool)
    fixed[:3] = True
    s.begin(committee=False, fixed=fixed)
    _refused(UNSUPPORTED, "held", lambda: live.md_committee([a]))
    s.begin(committee=False)
    live.md_record(2)
    _refused(UNSUPPORTED, "frame record", lambda: live.md_committee([a]))
    s.begin()
    _refused(UNSUPPORTED, "sgpr_md_record: the run has a committee", lambda: live.md_record(2))
    # ... and what else an attached committee rules out (the Python surface sets these inside md_begin: the C entry points)
    import ctypes as C
    from autoforce_amd import _lib
    lib, f64 = _lib.load(), lambda a: np.ascontiguousarray(a, dtype=np.float64)
    mask = np.zeros((s.N, 3), np.uint8)
    mask[0] = 1
    _refused(UNSUPPORTED, "sgpr_md_fix: the run has a committee", lambda: _lib.check(lib.sgpr_md_fix(live.handle, _lib.ptr(mask))))
    _refused(UNSUPPORTED, "sgpr_md_relax: the run has a committee", lambda: _lib.check(lib.sgpr_md_relax(live.handle, 0.01, None, 0, None)))
    s.begin(ttime_fs=25.0)
    ext = f64([-1e-4] * 3 + [0.0] * 3)
    _refused(UNSUPPORTED, "sgpr_md_barostat: the run has a committee",
             lambda: _lib.check(lib.sgpr_md_barostat(live.handle, 1.0, _lib.ptr(ext), None, 1.0)))
    _refused(INVALID, "sgpr_md_thermostat: call it before sgpr_md_committee", lambda: _lib.check(lib.sgpr_md_thermostat(live.handle, 1, 2.0, 0.02)))
    s.begin(committee=False)
    _refused(UNSUPPORTED, "16 members; at most 15", lambda: live.md_committee([a] * 16))
    live.md_committee([a])       # the handle stays usable
    live.md_end()


def test_refusal_of_a_member_on_another_device(sys1):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: a member cannot live on another one")
    from autoforce_amd import SGPRModel
    far = SGPRModel(3, 3, 4, 6.0, species=sys1.live.species, device=1)
    far.set_inducing(sys1.live.X)
    far.set_weights(sys1.live.mu, choli=sys1.live.choli)
    sys1.begin(committee=False)
    _refused(UNSUPPORTED, "lives on device 1", lambda: sys1.live.md_committee([far]))
    far.close()


def _two_rank_worker(rank, world, port, q):
    """A run begun on two ranks over the library's own exchange (test_hip_peer's set-up) asks for a committee."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd._lib import SgprError
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.watchdog import Watchdog
    from autoforce_amd.workloads import FS, MASS
    from test_hip_peer import _build
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"
    with Watchdog(f"committee on two ranks, rank {rank} of {world}", seconds=120, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, (numbers, pos, cell, pbc) = _build()
        member, _ = _build(seed=2)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * len(numbers) + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        masses = np.array([MASS[int(z)] for z in numbers])
        mdl.md_begin(numbers, pos, cell, pbc, masses, None, dt=FS, friction=0.0, kT=kB * 300.0)
        try:
            mdl.md_committee([member])
            got = (rank, 0, "accepted")
        except SgprError as e:
            got = (rank, e.code, str(e))
        mdl.md_end()
        q.put(got)
        dist.barrier()
        dist.destroy_process_group()


def test_refusal_of_a_run_begun_on_two_ranks():
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29400 + (os.getpid() % 250)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=200) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, code, msg in got:
        assert code == UNSUPPORTED and "the run was begun on 2 ranks; a committee runs on one" in msg, (rank, code, msg)


def test_refusals_invalid(sys1):
    s, a, live = sys1, sys1.members[0], sys1.live
    s.begin(committee=False)
    _refused(INVALID, "the live handle itself", lambda: live.md_committee([live]))
    _refused(INVALID, "member 1 is null", lambda: live.md_committee([a, None]))
    _refused(INVALID, "member 1 is member 0 again", lambda: live.md_committee([a, a]))
    bare = _hip_engine()
    bare.set_inducing(a.X)
    _refused(INVALID, "has no weights", lambda: live.md_committee([bare]))
    bare.set_weights(a.mu)
    _refused(INVALID, "has no choli", lambda: live.md_committee([bare]))
    bare.close()
    live.md_committee([a])
    live.md_run(1, None)
    _refused(INVALID, "the run has started", lambda: live.md_committee([a]))
    _refused(INVALID, "the run has started", lambda: live.md_committee([]))   # (a detach too: a started run keeps what it has)
    live.md_end()
    _refused(INVALID, "call sgpr_md_begin first", lambda: live.md_committee([a]))


def test_through_the_calculator(sys1):
    """BCMActiveCalculator.run_md (no teacher: it evaluates) on the device loop against the same calculator sent to the host loop."""
    from autoforce_amd.ase_shim import Atoms
    s, steps = sys1, 6
    res = {}
    for on_device in (True, False):
        calc = _calculator(s)
        if not on_device:
            calc.md_on_device_ok = lambda: False
        assert calc.md_on_device_ok() is on_device
        at = Atoms(s.numbers, s.pos.copy(), s.cell, s.pbc, velocities=s.vel.copy())
        out, seen = [], {}
        for st, E, T, u, w in calc.run_md(at, steps, 300.0, dt_fs=1.0, friction=0.05, rng=np.random.default_rng(9), sync_every=2):
            out.append((st, E, T))
            if st % 2 == 0:
                seen[st] = at.positions.copy()
        res[on_device] = (out, seen, at.positions.copy(), dict(calc.bcm_weights))
    (do, ds, dp, dw), (ho, hs, hp, hw) = res[True], res[False]
    bx, be = _twin_bounds("langevin_rows")
    assert [o[0] for o in do] == list(range(steps + 1)) == [o[0] for o in ho]
    assert max(abs(a[1] - b[1]) / abs(b[1]) for a, b in zip(do, ho)) <= be
    assert max(abs(a[2] - b[2]) for a, b in zip(do, ho)) <= 1e-9 * max(b[2] for b in ho)
    assert np.abs(dp - hp).max() <= bx
    assert sorted(ds) == sorted(hs) == [0, 2, 4, 6]
    for k in ds:
        assert np.abs(ds[k] - hs[k]).max() <= bx, k
    assert set(dw) == {"a", "live"} and abs(dw["a"] - hw["a"]) <= 1e-9 and abs(sum(dw.values()) - 1.0) <= 1e-12
