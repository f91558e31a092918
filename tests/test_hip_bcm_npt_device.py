"""GPU: the Bayesian committee under a barostat inside the device MD loop (sgpr_md_committee on a run with sgpr_md_barostat;
csrc/md_bcm.inc: md_bcm_move_kernel<true>, md_npt_kernel behind md_bcm_kernel) — the trajectory against its host twin,
workloads.npt_moving_cell around a BCMActiveCalculator over the same engines; the combination of an evaluation in a strained
cell against calculator_bcm's rule applied to the members' own predict(); the barostat integrating the committee's stress and
not the live model's; the same bits however the run is cut or halted; `iso` and a `mask`; the attach order and what stays
refused — a barostat without the run's option "md_committee_cell" among it (SGPRModel.md_committee(moving_cell=True) sets it).
System "lips343": the 343-atom LiPS 7 x 7 x 7 frame (21 x 16 + 7 rows; 256 + 87 atoms: the one-workgroup sums stride) with the
two models of test_hip_bcm_md_device.py::sys2; thermal velocities of seed 4, with which the largest covloss falls for six steps
and then rises above its start, so that a gate set from it halts the run in the middle.
System "big40": the 40-atom g5_big40 frame with the g12_bcm models "a" and "live"; its cell is cubic (12.6 A), periodic in all
three directions, and npt.make_cell_upper_triangular leaves it as it is (test_bcm_npt_cpu.py checks that without a GPU), so it
qualifies for the barostat.
Barostat and thermostat are those of test_hip_npt_device.py::_setup: pfactor = (100 fs)^2 x 30 GPa, 1 GPa external, T = 600 K,
tdamp = 25 fs."""
import numpy as np
import pytest

import bcm_md_common as bc

pytestmark = pytest.mark.gpu

T, TDAMP = 600.0, 25.0

# The twin tolerance, by the rule of test_hip_bcm_md_device.py ("The committee loop"): ten times the value measured on
# an MI355X, never tighter than 16 ulp of the largest coordinate / of |E| (FLOOR), never looser than 1e-9.  TWIN_MEASURED holds
# the measured (max |dx| in Angstrom, max |dE| / |E|, max |dh| / max |h|, max |deta| / max |eta|) per comparison; None = not
# measured: REASONED.
# The reasoning is the constant-cell one — both sides run the same member evaluations and the same integrator operations and
# differ in the last bits of the weights (the device's log against numpy's), a few ulp of a force, an energy or a stress per
# evaluation — with one more path for that error: the stress moves eta by 2 dt pfact det(h) x (a few ulp of sigma), some 1e-22
# per evaluation here, and eta moves h and the positions by dt times that: far below an ulp of either.  So, as at constant cell,
# the sides are a few ulp apart after 16 steps unless a rounding flips; 1e-12 A, 1e-12 |E| and 1e-12 max |h| is some 300 ulp.
# eta is compared relative to its largest entry over the run (it is a sum of increments of that size) at the same 1e-12; the
# final velocities, (q_(n+1) - q_(n-1)) h / 2 dt, inherit the positions' bound divided by dt.
# Measured: positions, velocities and energies agree bit for bit everywhere; cell and strain rate differ in places by less than an
# ulp of their largest entry (entries that are zero on one side and 1e-20 on the other, the last bit of an eta).  "strain": the
# cell of evaluation 2 alone; "callers": test_hip_bcm_npt_callers.py, which compares no strain rate.
TWIN_MEASURED = {"lips343": (0.0, 0.0, 8.9e-23, 3.9e-17), "big40": (0.0, 0.0, 4.4e-21, 1.2e-16), "iso": (0.0, 0.0, 0.0, 0.0),
                 "mask": (0.0, 0.0, 0.0, 1.6e-16), "strain": (0.0, 0.0, 0.0, 0.0), "callers": (0.0, 0.0, 0.0, 0.0)}
REASONED = (1e-12, 1e-12, 1e-12, 1e-12)
FLOOR = (16 * 3.6e-15, 16 * 2.3e-16, 16 * 2.3e-16, 16 * 2.3e-16)


def _twin_bounds(kind):
    got = TWIN_MEASURED[kind]
    if got is None:
        return REASONED
    return tuple(min(max(10.0 * v, f), 1e-9) for v, f in zip(got, FLOOR))


def _baro():
    from autoforce_amd.npt import GPA
    from autoforce_amd.workloads import FS
    return dict(pfactor=(100.0 * FS) ** 2 * 30.0 * GPA, externalstress=1.0 * GPA)


class System:
    def __init__(self, members, live, posts, frame, vel_seed=3):
        from autoforce_amd.workloads import MASS
        self.members, self.live, self.posts = members, live, posts
        self.numbers, self.pos, self.cell, self.pbc = frame
        self.N = len(self.numbers)
        self.mass = np.array([MASS[int(z)] for z in self.numbers])
        self.vel = bc.thermal_velocities(self.numbers, temperature=T, seed=vel_seed)

    def begin(self, committee=True, barostat=True, moving_cell=None, **kw):
        from autoforce_amd.ase_shim import kB
        from autoforce_amd.workloads import FS
        baro = _baro() if barostat else {}
        self.live.md_begin(self.numbers, self.pos, self.cell, self.pbc, self.mass, self.vel, dt=1.0 * FS, friction=0.0, kT=kB * T,
                           ttime=TDAMP * FS, **baro, **kw)
        if committee:
            # (the run's option "md_committee_cell": without it a committee and a barostat refuse each other)
            self.live.md_committee(self.members, moving_cell=barostat if moving_cell is None else moving_cell)

    def outs(self, positions, cell):
        """Every member's own predict() at `positions` in `cell`, the live model last."""
        return [m.predict(self.numbers, positions, cell, self.pbc, beta=True) for m in self.members + [self.live]]

    def calculator(self):
        from autoforce_amd.calculator_bcm import BCMActiveCalculator
        return BCMActiveCalculator(covariance=self.posts["live"], kernel_model_dict={"a": self.posts["a"]}, logfile=None)

    def twin(self, steps, **kw):
        """workloads.npt_moving_cell around the committee calculator: (E, x, v, h, eta) per evaluation."""
        from autoforce_amd.workloads import npt_moving_cell
        return [(E, x.copy(), v.copy(), h.copy(), e.copy()) for _, E, Tk, _, x, v, h, e, z, zi in
                npt_moving_cell(self.calculator(), self.numbers, self.pos, self.cell, self.pbc, steps, temperature=T, dt_fs=1.0, tdamp_fs=TDAMP,
                                vel=self.vel, species=self.live.species, **_baro(), **kw)]

    def run(self, cuts, final=True, ediff=0.0):
        """md_run call by call: rows, cells, etas of every evaluation."""
        rows, cells, etas = [], [], []
        for k, n in enumerate(cuts):
            sc, code = self.live.md_run(n, None, ediff=ediff, final=final and k == len(cuts) - 1)
            assert code == 0 and len(sc) == n
            c, e = self.live.md_cells()
            assert len(c) == n
            rows.extend(sc)
            cells.extend(c)
            etas.extend(e)
        return np.array(rows), np.array(cells), np.array(etas)


def _hip_engine():
    from autoforce_amd import SGPRModel
    from helpers import load
    g = load("g5_big40")
    return SGPRModel(int(g["lmax"]), int(g["nmax"]), float(g["eta"]), float(g["rc"]), species=g["species"].tolist())


@pytest.fixture(scope="module")
def big40():
    posts, g = bc.g12_posts(_hip_engine)
    s = System([posts["a"].engine], posts["live"].engine, posts, (g["numbers"], g["positions"], g["cell"], g["pbc"]))
    yield s
    for m in s.members + [s.live]:
        m.close()


@pytest.fixture(scope="module")
def lips343():
    from autoforce_amd import SGPRModel
    from autoforce_amd.posterior import PosteriorPotential
    from autoforce_amd.workloads import inducing_from_frame, lips
    numbers, pos, cell, pbc = lips(7, seed=0)
    assert len(numbers) == 343
    species = sorted(set(int(z) for z in numbers))
    models = []
    for m, seed in ((40, 1), (48, 2)):   # (the two inducing subsets of test_hip_bcm_md_device.py::sys2)
        mdl = SGPRModel(3, 3, 4, 6.0, species=species)
        n2, p2, c2, b2 = lips(7, seed=seed)
        mdl.set_inducing(inducing_from_frame(mdl, n2, p2, c2, b2, m, seed=seed))
        rng = np.random.default_rng(2 + seed)
        mdl.solve(rng.normal(size=(64, m)), rng.normal(size=64))
        mdl.set_weights(0.02 * rng.normal(size=m), choli=mdl.choli, vscale=mdl.make_vscale())
        models.append(mdl)
    posts = {"a": PosteriorPotential(models[0]), "live": PosteriorPotential(models[1])}
    s = System([models[0]], models[1], posts, (numbers, pos, cell, pbc), vel_seed=4)
    yield s
    for m in models:
        m.close()


def _compare_with_twin(kind, s, rows, cells, etas, st, twin):
    """Energies, cell and strain rate of every evaluation, the final positions, velocities and cell."""
    from autoforce_amd.workloads import FS
    assert len(rows) == len(twin) == len(cells)
    tE, th, te = np.array([t[0] for t in twin]), np.array([t[3] for t in twin]), np.array([t[4] for t in twin])
    de = float(np.max(np.abs(rows[:, 0] - tE) / np.abs(tE)))
    hmax, emax = float(np.abs(th).max()), float(np.abs(te).max())
    dh = float(max(np.abs(cells - th).max(), np.abs(st["cell"] - th[-1]).max()) / hmax)
    dn = float(np.abs(etas - te).max() / emax)
    dx = float(np.abs(st["positions"] - twin[-1][1]).max())
    dv = float(np.abs(st["velocities"] - twin[-1][2]).max())
    bx, be, bh, bn = _twin_bounds(kind)
    print(f"twin {kind}: max|dx| {dx:.3e} A  max|dE|/|E| {de:.3e}  max|dh|/max|h| {dh:.3e}  max|deta|/max|eta| {dn:.3e} (max|eta| {emax:.3e})  "
          f"max|dv| {dv:.3e}  (asserted at {bx:.1e}, {be:.1e}, {bh:.1e}, {bn:.1e})")
    assert de <= be and dh <= bh and dn <= bn
    assert dx <= bx and dv <= bx / FS


@pytest.mark.parametrize("which", ["lips343", "big40"])
def test_trajectory_against_the_host_twin(which, request):
    """16 steps in four calls of 3, 1, 5 and 8 evaluations against npt_moving_cell around the same committee."""
    s, steps = request.getfixturevalue(which), 16
    s.begin()
    rows, cells, etas = s.run((3, 1, 5, 8))
    st = s.live.md_state(results=True)
    twin = s.twin(steps)
    _compare_with_twin(which, s, rows, cells, etas, st, twin)
    assert np.abs(st["cell"] - s.cell).max() > 1e-6        # the cell has moved
    assert rows[0][14] == 0.0 and rows[-1][14] != 0.0      # ... and the thermostat with it


def _check_combination(s, st, w, cm, row):
    """Packed F, E, stress, beta of a state against the rule applied to the members' predict() at its positions IN ITS CELL."""
    ref = bc.committee_rule(s.outs(st["positions"], st["cell"]))
    fmax = np.abs(ref["forces"]).max()
    dF = np.abs(st["forces"] - ref["forces"]).max()
    dE = abs(st["energy"] - ref["energy"])
    dS = np.abs(st["stress"] - ref["stress"]).max()
    dB = np.abs(st["beta"] - ref["beta"]).max()
    print(f"combination N={s.N}: dF {dF:.3e} (max|F| {fmax:.3e})  dE {dE:.3e} (|E| {abs(ref['energy']):.3e})  dS {dS:.3e} "
          f"(max|S| {np.abs(ref['stress']).max():.3e})  dbeta {dB:.3e}  w {w}")
    assert dF <= 1e-8 * fmax
    assert dE <= 1e-8 * abs(ref["energy"])
    assert dS <= 1e-8 * np.abs(ref["stress"]).max()
    assert dB <= 2e-6
    assert np.abs(cm - ref["covmax"]).max() <= 2e-6
    assert np.abs(w - bc.weights_of(cm)).max() <= 1e-12     # the rule applied to the device's own covmax
    assert row[0] == st["energy"] and row[11] == st["beta"].max() and row[10] == 0.0
    return ref


@pytest.mark.parametrize("which", ["lips343", "big40"])
def test_combination_under_strain_and_whose_stress_moves_the_cell(which, request):
    s = request.getfixturevalue(which)
    s.begin()
    rows, cells, etas = s.run((4,))                         # three moves, the fourth configuration evaluated
    st = s.live.md_state(results=True)
    assert not np.array_equal(st["cell"], s.cell) and np.array_equal(st["cell"], cells[3])
    assert not np.array_equal(st["positions"], s.pos)
    ref = _check_combination(s, st, *s.live.md_committee_info(), rows[3])
    assert 0.0 < ref["w"][0] < 1.0
    # the barostat integrates the committee's stress: h_2 = h_0 + 2 dt h_1 eta_1, eta_1 from the stress of evaluation 0
    s.begin(committee=False)
    _, alone, _ = s.run((4,))
    assert np.array_equal(alone[:2], cells[:2]) and not np.array_equal(alone[2], cells[2])
    twin = s.twin(3)
    bx, be, bh, bn = _twin_bounds("strain")
    dh = np.abs(cells[2] - twin[2][3]).max() / np.abs(twin[2][3]).max()
    sep = np.abs(alone[2] - cells[2]).max() / np.abs(cells[2]).max()
    print(f"cell of evaluation 2, N={s.N}: committee against the twin {dh:.3e} (asserted at {bh:.1e}), against the live model alone {sep:.3e}")
    assert dh <= bh and sep > 100.0 * bh


@pytest.mark.parametrize("which", ["lips343", "big40"])
def test_cutting_and_halting_change_no_bit(which, request):
    s, n = request.getfixturevalue(which), 16
    s.begin()
    a = s.run((n,))
    sa = s.live.md_state(results=True)
    s.begin()
    b = s.run((1, 4, 11))
    sb = s.live.md_state(results=True)
    keys = ("positions", "velocities", "velocities_pre", "cell", "eta", "forces", "beta", "energy", "stress")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for key in keys:
        assert np.array_equal(sa[key], sb[key]), key
    # a halt in the middle: the first evaluation whose largest covloss exceeds every one before it
    bt = a[0][:, 11]
    later = [k for k in range(2, n - 2) if bt[k] > bt[:k].max()]
    assert later, bt
    k = later[len(later) // 2]
    ediff = 0.5 * (bt[:k].max() + bt[k])
    print(f"halt N={s.N}: covloss maxima {bt}, chosen evaluation {k}, ediff {ediff}")
    s.begin()
    s.run((k,), final=False)   # (the configuration the halt must leave: a run cut there)
    want = s.live.md_state()
    s.begin()
    sc, code = s.live.md_run(n, None, ediff=ediff, final=True)
    assert code == 1 and len(sc) == k + 1 and np.array_equal(sc, a[0][:k + 1])
    c, e = s.live.md_cells()
    assert np.array_equal(c, a[1][:k + 1]) and np.array_equal(e, a[2][:k + 1])
    got = s.live.md_state(results=True)
    for key in ("positions", "velocities_pre", "cell", "eta"):
        assert np.array_equal(got[key], want[key]), key
    assert got["energy"] == a[0][k][0]
    _check_combination(s, got, *s.live.md_committee_info(), sc[k])
    # ... and on from there: the halted configuration again, then the rest of the run
    sc2, code = s.live.md_run(n - k, None, ediff=0.0, final=True)
    assert code == 0 and np.array_equal(sc2, a[0][k:])
    c2, e2 = s.live.md_cells()
    assert np.array_equal(c2, a[1][k:]) and np.array_equal(e2, a[2][k:])
    sc_ = s.live.md_state(results=True)
    for key in keys:
        assert np.array_equal(sa[key], sc_[key]), key


@pytest.mark.parametrize("kind", ["iso", "mask"])
def test_iso_and_mask_against_the_host_twin(kind, request):
    """8 steps with iso=True (big40) and with a mask on the diagonal (lips343)."""
    s, steps = request.getfixturevalue("big40" if kind == "iso" else "lips343"), 8
    kw = dict(iso=True) if kind == "iso" else dict(mask=(1, 1, 0))
    s.begin(**kw)
    rows, cells, etas = s.run((2, steps - 1))
    st = s.live.md_state(results=True)
    _compare_with_twin(kind, s, rows, cells, etas, st, s.twin(steps, **kw))
    c = st["cell"]
    assert c[0, 0] != s.cell[0, 0]
    if kind == "iso":
        np.testing.assert_allclose(c / c[2, 2], s.cell / s.cell[2, 2], rtol=0, atol=1e-12)
    else:
        assert c[2, 2] == s.cell[2, 2] and c[1, 1] != s.cell[1, 1]


def _refused(code, match, call):
    from autoforce_amd._lib import SgprError
    with pytest.raises(SgprError, match=match) as e:
        call()
    assert e.value.code == code, e.value


UNSUPPORTED, INVALID = -6, -1


def test_attach_order_detach_and_refusals(big40):
    from autoforce_amd import _lib
    from autoforce_amd.npt import zero_mean_momentum
    s, a, live = big40, big40.members[0], big40.live
    lib = _lib.load()
    baro = _baro()
    ext = np.ascontiguousarray([-baro["externalstress"]] * 3 + [0.0] * 3, dtype=np.float64)

    def barostat():
        return lib.sgpr_md_barostat(live.handle, float(baro["pfactor"]), _lib.ptr(ext), None, 1.0)

    # barostat then committee (the Python surface), committee then barostat (the C entry points): the same bits
    s.begin()
    first = s.run((6,))
    sf = live.md_state(results=True)
    vel, s.vel = s.vel, zero_mean_momentum(s.vel, s.mass)   # (what md_begin(pfactor=) uploads)
    try:
        s.begin(barostat=False, moving_cell=True)
    finally:
        s.vel = vel
    _lib.check(barostat())
    live._md["npt"] = True      # (what md_begin(pfactor=) notes for md_cells / md_state)
    second = s.run((6,))
    ss = live.md_state(results=True)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    for key in ("positions", "velocities", "cell", "eta", "forces", "energy"):
        assert np.array_equal(sf[key], ss[key]), key
    # a started run takes neither
    assert barostat() == _lib.E_INVALID
    _refused(INVALID, "sgpr_md_committee: the run has started", lambda: live.md_committee([a]))
    _refused(INVALID, "md_committee_cell: the run has started", lambda: live.md_committee([a], moving_cell=True))
    # without the run's option each still refuses the other, and md_begin switches the option off again
    s.begin(committee=False)
    _refused(UNSUPPORTED, "sgpr_md_committee: the run has a barostat.*md_committee_cell", lambda: live.md_committee([a]))
    s.begin(barostat=False, moving_cell=False)
    assert barostat() == _lib.E_UNSUPPORTED
    live.md_end()
    _refused(INVALID, "md_committee_cell belongs to a run", lambda: _lib.check(lib.sgpr_set_option(live.handle, b"md_committee_cell", 1)))
    # detaching leaves the plain moving-cell run
    s.begin(committee=False)
    plain = s.run((6,))
    sp = live.md_state(results=True)
    s.begin()
    live.md_committee([])
    gone = s.run((6,))
    sg = live.md_state(results=True)
    for x, y in zip(plain, gone):
        assert np.array_equal(x, y)
    for key in ("positions", "velocities", "cell", "eta", "forces", "energy"):
        assert np.array_equal(sp[key], sg[key]), key
    assert not np.array_equal(plain[1][2], first[1][2])
    # what stays refused beside the barostat: argument checks, nothing is enqueued
    s.begin(committee=False, ml_filter=0.5)
    _refused(UNSUPPORTED, "sgpr_md_committee: the run has a filter", lambda: live.md_committee([a], moving_cell=True))
    fixed = np.zeros(s.N, bool)
    fixed[:3] = True
    with pytest.raises(NotImplementedError, match="held components"):
        s.begin(committee=False, fixed=fixed)
    s.begin(committee=False)
    live.md_record(2)
    _refused(UNSUPPORTED, "sgpr_md_committee: a frame record is armed", lambda: live.md_committee([a], moving_cell=True))
    s.begin()
    _refused(UNSUPPORTED, "sgpr_md_record: the run has a committee", lambda: live.md_record(2))
    with pytest.raises(NotImplementedError, match="sgpr_md_meta: the run has a barostat"):
        live.md_meta([("distance", 0, 1)], 0.1, 0.01)
    s.begin(committee=False)
    _refused(UNSUPPORTED, "16 members; at most 15", lambda: live.md_committee([a] * 16, moving_cell=True))
    live.md_committee([a], moving_cell=True)       # the handle stays usable
    sc, code = live.md_run(2, None, final=True)
    assert code == 0 and len(sc) == 2
    live.md_end()
