"""The filter of model-update jumps (`ml_filter=`) in the host twins of the device loops — workloads.langevin_nvt,
nose_hoover_nvt and npt_moving_cell: the reference's FilterDeltas (calculator/active.py:47-76) written by evaluation index,
    A_f <- (A_f + deltas["forces"]) s,  F_seen = F - clip(A_f, -1, 1);   A_s <- (A_s + deltas["stress"]) s,  stress - A_s
once per configuration, the rule sgpr_md_filter states.  A stub calculator (a pair potential plus offsets that jump at chosen
configurations, where it publishes `deltas`; one jump is +10 eV/A on some components and -10 on others, so both clamps act)
stands for a model that updates; the same stub with FilterDeltas' arithmetic already applied inside its getters is what every
twin with ml_filter= must equal bit for bit."""
import os

import numpy as np
import pytest

from autoforce_amd.ase_shim import Atoms
from autoforce_amd.npt import GPA, NPT, FilterDeltas
from autoforce_amd.workloads import FS, langevin_nvt, nose_hoover_nvt, npt_moving_cell
from fixed_common import mask as _mask, toy as _toy
from helpers import PairTeacher
from test_npt_twin_cpu import PFACTOR, _system

STEPS, SHRINK = 30, 0.8
PBC = [True] * 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_twins_unmasked.npz")


def _jumps(N, seed=2):
    """Configuration -> (dF, dS): order 0.3 eV/A with +-10 on a few components at 5; two in a row at 11, 12; stress 1e-3."""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (5, 11, 12, 20):
        dF = 0.3 * rng.normal(size=(N, 3))
        if n == 5:
            dF[1, 0] = dF[4, 2] = dF[7, 1] = 10.0
            dF[2, 1] = dF[9, 0] = -10.0
        out[n] = (dF, 1e-3 * rng.normal(size=6))
    return out


class Jumping:
    """base + offsets that jump at the configurations of `jumps` (counted by distinct positions / cells asked for); `deltas` as
    ActiveCalculator publishes them: the jump where one happened, None elsewhere.  prefilter = s: the getters return what
    FilterDeltas(shrink=s) would make of them, and no deltas are published."""
    implemented_properties = ["energy", "forces", "stress", "free_energy"]

    def __init__(self, base, jumps, N, prefilter=None):
        self.base, self.jumps, self.prefilter = base, jumps, prefilter
        self.n, self._key, self.deltas, self.results = -1, None, None, {}
        self.off_f, self.off_s = np.zeros((N, 3)), np.zeros(6)
        self.acc_f, self.acc_s = np.zeros((N, 3)), np.zeros(6)
        self.raw_forces = None

    def get_property(self, name, atoms=None):
        key = None if atoms is None else (atoms.positions.tobytes(), np.asarray(atoms.cell).tobytes())
        if atoms is not None and key != self._key:
            self._key = key
            self.n += 1
            r = {q: np.array(self.base.get_property(q, atoms)) for q in ("energy", "forces", "stress")}
            d = None
            if self.n in self.jumps:
                dF, dS = self.jumps[self.n]
                self.off_f, self.off_s = self.off_f + dF, self.off_s + dS
                d = dict(energy=0.0, forces=dF, stress=dS)
            F, S = r["forces"] + self.off_f, r["stress"] + self.off_s
            self.raw_forces = F
            if self.prefilter is not None:
                self.acc_f = ((self.acc_f + d["forces"]) if d else self.acc_f) * self.prefilter
                self.acc_s = ((self.acc_s + d["stress"]) if d else self.acc_s) * self.prefilter
                F, S = F - np.clip(self.acc_f, -1.0, 1.0), S - self.acc_s
                d = None
            self.deltas = d
            self.results = dict(energy=float(r["energy"]), free_energy=float(r["energy"]), forces=F, stress=S)
        return self.results[name]


def _pair(N, **kw):
    return Jumping(PairTeacher(rc=4.0), _jumps(N), N, **kw)


def _run(twin, calc, kw, **extra):
    numbers, pos, cell, mass, v = _system()
    return [tuple(np.copy(c) if isinstance(c, np.ndarray) else c for c in row)
            for row in twin(calc, numbers, pos, cell, PBC, STEPS, 300.0, 1.0, vel=v, **kw, **extra)]


TWINS = [(langevin_nvt, dict(friction=0.05, seed=3)), (langevin_nvt, dict(friction=0.0, seed=3)), (nose_hoover_nvt, dict(tdamp_fs=25.0)),
         (npt_moving_cell, dict(tdamp_fs=25.0, pfactor=PFACTOR, externalstress=1.0 * GPA)),
         (npt_moving_cell, dict(tdamp_fs=25.0, pfactor=PFACTOR, externalstress=1.0 * GPA, iso=True))]
IDS = ["langevin", "verlet", "nose-hoover", "npt", "npt-iso"]


def _same(a, b, skip=(3,)):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for k, (ca, cb) in enumerate(zip(ra, rb)):
            if k not in skip:   # (3: wall seconds)
                assert np.array_equal(np.asarray(ca), np.asarray(cb)), k


@pytest.mark.parametrize("twin,kw", TWINS, ids=IDS)
def test_twin_with_a_filter_equals_the_twin_around_prefiltered_getters(twin, kw):
    N = 27
    raw = _pair(N)
    got = _run(twin, raw, kw, ml_filter=SHRINK)
    pre = _pair(N, prefilter=SHRINK)
    ref = _run(twin, pre, kw)
    _same([r[:-1] for r in got], ref)
    # the accumulators: as the LAST configuration found them, i.e. one shrink short of the prefiltered calculator's
    f, s = got[-1][-1]
    assert np.array_equal(f * SHRINK, pre.acc_f) and np.abs(f).max() > 0
    if twin is npt_moving_cell:
        assert np.array_equal(s * SHRINK, pre.acc_s) and np.abs(s).max() > 0
    else:
        assert not s.any()   # (nobody asks for a stress at constant cell)
    # both clamps acted, and the filter changed the walk
    f6 = got[6][-1][0]
    assert f6.max() > 1.0 and f6.min() < -1.0
    plain = _run(twin, _pair(N), kw)
    assert np.array_equal(plain[5][4], got[5][4]) and not np.array_equal(plain[8][4], got[8][4])


@pytest.mark.parametrize("iso", [False, True], ids=["full", "iso"])
def test_moving_cell_twin_with_a_filter_against_npt_around_filterdeltas(iso):
    numbers, pos, cell, mass, v = _system()
    N = len(numbers)
    at = Atoms(numbers, pos, cell, True, velocities=v, masses=mass)
    at.calc = _pair(N)
    wrapped = FilterDeltas(at, shrink=SHRINK)
    dyn = NPT(wrapped, 1.0 * FS, 300.0, ttime=25.0 * FS, externalstress=1.0 * GPA, pfactor=PFACTOR)
    if iso:
        dyn.set_fraction_traceless(0.0)
    twin = npt_moving_cell(_pair(N), numbers, pos, cell, PBC, STEPS, 300.0, 1.0, 25.0, vel=v, iso=iso, externalstress=1.0 * GPA, pfactor=PFACTOR,
                           ml_filter=SHRINK)
    n = 0
    for (k, E, T, _), (kt, Et, Tt, _, xt, vt, ht, et, zeta, zint, acc) in zip(dyn.run(STEPS), twin):
        assert k == kt
        # (the tolerances of test_npt_twin_cpu.py: twin against NPT)
        np.testing.assert_allclose(at.positions, xt, rtol=0, atol=1e-10)
        np.testing.assert_allclose(np.asarray(at.cell), ht, rtol=0, atol=1e-10)
        np.testing.assert_allclose(dyn.eta, et, rtol=0, atol=1e-10)
        assert abs(E - Et) < 1e-9 and abs(dyn.zeta - zeta) < 1e-12 and abs(dyn.zeta_integrated - zint) < 1e-12
        if k:
            np.testing.assert_allclose(at.get_velocities(), vt, rtol=0, atol=1e-10)
        n += 1
    assert n == STEPS + 1
    # FilterDeltas has shrunk for the last configuration's forces already; its stress call comes with the next step
    np.testing.assert_allclose(acc[0] * SHRINK, wrapped.f, rtol=0, atol=1e-12)
    np.testing.assert_allclose(acc[1], wrapped.s, rtol=0, atol=1e-15)
    assert np.abs(wrapped.f).max() > 0 and np.abs(wrapped.s).max() > 0


def test_without_a_filter_the_twins_keep_their_bits():
    """ml_filter=None against the walks recorded before fixed= existed (fixed_common.walks' calls), and for the moving cell
    against the call without the keyword."""
    gold = np.load(GOLDEN)
    numbers, pos, cell, v, calc = _toy()
    rows = [(E, T, p.copy(), w.copy()) for _, E, T, _, p, w in
            langevin_nvt(calc, numbers, pos, cell, PBC, 25, 300.0, 1.0, 0.05, seed=3, vel=v, ml_filter=None, filter_init=None)]
    assert np.array_equal([r[0] for r in rows], gold["lv_E"]) and np.array_equal([r[1] for r in rows], gold["lv_T"])
    assert np.array_equal(rows[-1][2], gold["lv_x"]) and np.array_equal(rows[-1][3], gold["lv_v"])
    rows = [(E, T, p.copy(), w.copy(), z, zi) for _, E, T, _, p, w, z, zi in
            nose_hoover_nvt(calc, numbers, pos, cell, PBC, 25, 300.0, 1.0, 20.0, vel=v, ml_filter=None, filter_init=None)]
    assert np.array_equal([r[0] for r in rows], gold["nh_E"]) and np.array_equal([r[4] for r in rows], gold["nh_zeta"])
    assert np.array_equal(rows[-1][2], gold["nh_x"]) and np.array_equal(rows[-1][3], gold["nh_v"])
    kw = TWINS[3][1]
    _same(_run(npt_moving_cell, PairTeacher(rc=4.0), kw), _run(npt_moving_cell, PairTeacher(rc=4.0), kw, ml_filter=None, filter_init=None))


@pytest.mark.parametrize("twin,kw", TWINS[:3], ids=IDS[:3])
def test_a_held_component_sees_zero_whatever_the_accumulator_holds(twin, kw):
    numbers, pos, cell, mass, v = _system()
    N = len(numbers)
    fx = _mask(N)
    big = np.full((N, 3), 7.0)   # (clamped to 1 eV/A on every component, held ones included)
    got = _run(twin, _pair(N), kw, ml_filter=SHRINK, fixed=fx, filter_init=(big, None))
    ref = _run(twin, _pair(N, prefilter=SHRINK), kw, fixed=fx)
    free = _run(twin, _pair(N), kw, ml_filter=SHRINK, filter_init=(big, None))
    for row, rf in zip(got, free):
        x, w = row[4], row[5]
        assert np.array_equal(x[fx], pos[fx])   # the bits they started with
        assert np.array_equal(w[fx], np.zeros(fx.sum())) and not np.signbit(w[fx]).any()
        assert np.abs(row[-1][0][fx]).min() > 0     # ... while their accumulators are anything but zero
    assert not np.array_equal(free[3][4][fx], pos[fx])
    # and with zero accumulators at the start: the masked twin around the prefiltered getters, bit for bit
    got0 = _run(twin, _pair(N), kw, ml_filter=SHRINK, fixed=fx)
    _same([r[:-1] for r in got0], ref)


@pytest.mark.parametrize("cut", [12, 9], ids=["cut-at-a-jump", "cut-between-jumps"])
def test_filter_init_continues_a_run(cut):
    """Two halves — the second begun from the first's last positions, velocities and accumulators, with the deviate stream and
    the calculator going on — are the one run, bit for bit; also where the cut configuration is one that jumped."""
    numbers, pos, cell, mass, v = _system()
    N = len(numbers)
    kw = dict(friction=0.05)
    one = [(p.copy(), w.copy(), a) for *_, p, w, a in
           langevin_nvt(_pair(N), numbers, pos, cell, PBC, STEPS, 300.0, 1.0, vel=v, rng=np.random.default_rng(3), ml_filter=SHRINK, **kw)]
    calc, rng = _pair(N), np.random.default_rng(3)
    first = [(p.copy(), w.copy(), a) for *_, p, w, a in
             langevin_nvt(calc, numbers, pos, cell, PBC, cut, 300.0, 1.0, vel=v, rng=rng, ml_filter=SHRINK, **kw)]
    p, w, a = first[-1]
    second = [(p_.copy(), w_.copy(), a_) for *_, p_, w_, a_ in
              langevin_nvt(calc, numbers, p, cell, PBC, STEPS - cut, 300.0, 1.0, vel=w, rng=rng, ml_filter=SHRINK, filter_init=a, **kw)]
    both = first + second[1:]
    assert len(both) == len(one)
    for (pa, wa, aa), (pb, wb, ab) in zip(one, both):
        assert np.array_equal(pa, pb) and np.array_equal(wa, wb) and np.array_equal(aa[0], ab[0]) and np.array_equal(aa[1], ab[1])
    assert np.array_equal(second[0][0], first[-1][0]) and np.array_equal(second[0][1], first[-1][1])


def test_shrink_must_lie_between_zero_and_one():
    numbers, pos, cell, mass, v = _system()
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            next(langevin_nvt(_pair(27), numbers, pos, cell, PBC, 2, 300.0, 1.0, vel=v, ml_filter=bad))
