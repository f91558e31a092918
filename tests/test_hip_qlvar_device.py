"""GPU tests of the Steinhardt Q_l colvar inside the device MD loop (kind 2 of md_meta.inc: md_meta_ql_kernel,
md_meta_merged_ql_kernel; sgpr_md_meta_ql) against the host twin workloads.meta_bias / workloads.langevin_nvt(meta=) around the
same library, on the golden frames with their own fitted models (rc = 6) and the cases of tests/golden/g17_qlvar.npz.

  Every comparison with the twin asserts test_hip_meta_device's precondition: no CV component within 1e-6 sigma of a bin or block
edge.
  A single evaluation with preloaded hills on every case: forces, energy and stress of md_state minus the same run without a bias,
and the hill row, against meta_bias to 1e-12 of the largest bias force (that file's bound for the other kinds: the device forms
the pair sums in the twin's order, so only sqrt, the divisions and exp could differ).  Covered by the cases: two dimensions,
46 selected neighbours with repeated images of one atom and the index atom's own images (sheared: they stand on the z axis), a
66-entry list in a triclinic cell, the index atom last in caller order, species selection, an open direction with neighbours near
the z axis, a cluster, and an empty environment evaluated twice (Fself does not accumulate).
  A 64-step Langevin trajectory on si32 (soft model, Q4 + Q6, well-tempered) against workloads.langevin_nvt(meta=): the largest
deviation of positions and velocities measured on the first run was 2.14e-16 relative (a velocity; every position and every
hill row had the twin's bits); the bound is 100 times that.
  Bit for bit — positions, velocities, every hill row —: one call, calls of 7, halted by the covloss gate and evaluated again,
repeated; also with merge=16.  With fixed=, ml_filter= and md_record together.  The refusals.  A spec without a qlvar gives the
same bits before and after a qlvar run on the same handle."""
import numpy as np
import pytest

from helpers import load
from test_hip_fixed_device import _Rows
from test_hip_meta_device import DT_FS, MARGIN, SOFT, STEPS, T, _begin, _cut_run, _single, _vel, models  # noqa: F401  (models: a fixture)
from test_hip_npt_device import _PredictCalc

pytestmark = pytest.mark.gpu

RC = 6.0
TRAJ_MEASURED = 2.14e-16     # the largest relative deviation of positions and velocities on the first run
TRAJ_RTOL = 100 * TRAJ_MEASURED
assert TRAJ_RTOL <= 1e-8

# name -> (frame, index (None: first of species i), i, j, cutoff, l): the cases of g17_qlvar.npz
CASES = {
    "si32_a0": ("g5_si32", 0, 14, 14, 4.0, (4, 6)),
    "si32_a5_images": ("g5_si32", 5, 14, 14, 6.0, (4,)),
    "tric24_a0": ("g5_tric24", 0, None, 16, 6.0, (4, 6)),
    "tric24_last": ("g5_tric24", 23, None, 3, 6.0, (6,)),
    "mixed64_zr_c4": ("g5_mixed64", None, 40, 8, 4.0, (4, 6)),
    "mixed64_zr_c6": ("g5_mixed64", None, 40, 8, 6.0, (4, 6)),
    "slab18_nearz": ("g5_slab18_nearz", 0, None, 29, 6.0, (4, 6)),
    "cluster16_a0": ("g5_cluster16", 0, None, 10, 6.0, (6,)),
}


def _bias(mdl, cvs, sigma, w, numbers, pos, cell, pbc, hills, tem=None, merge=None):
    from autoforce_amd.workloads import meta_bias
    return meta_bias(cvs, sigma, w, numbers, pos, cell, hills, tem=tem, species=mdl.species, merge=merge, pbc=pbc, rc=RC)


def _margin(cv, sigma, dims):
    """meta_bias's margin over the dimensions `dims`: the distance, in units of sigma, from a bin edge k sigma or a block edge k 5 sigma"""
    u = (np.asarray(cv) / np.broadcast_to(np.asarray(sigma, float), np.shape(cv)))[dims]
    return float(min(np.min(np.minimum(u - np.floor(u), np.ceil(u) - u)), 5.0 * np.min(np.minimum(u / 5 - np.floor(u / 5), np.ceil(u / 5) - u / 5))))


def _check_single(mdl, numbers, pos, cell, pbc, cvs, sigma, w, tem, H, seed=1, label="", exact=()):
    """exact: dimensions whose CV is 0.0 by construction on both sides (an empty environment) — ON a bin edge, and no last bit can
    move it: the margin precondition is asserted over the others"""
    cv0 = _bias(mdl, cvs, sigma, w, numbers, pos, cell, pbc, None)["cv"]
    hills = cv0 + 1.2 * np.asarray(sigma) * np.random.default_rng(seed).normal(size=(H, len(cv0)))
    want = _bias(mdl, cvs, sigma, w, numbers, pos, cell, pbc, hills, tem=tem)
    if exact:
        assert all(want["cv"][d] == 0.0 for d in exact)
        assert _margin(want["cv"], sigma, [d for d in range(len(cv0)) if d not in exact]) > MARGIN
    else:
        assert want["margin"] > MARGIN, want["margin"]
    row0, plain = _single(mdl, numbers, pos, cell, pbc)
    row, st = _single(mdl, numbers, pos, cell, pbc, cvs, sigma=sigma, w=w, tem=tem, hills=hills, capacity=H + 4)
    fb = np.abs(want["forces"]).max()
    tol = 1e-12 * fb
    dF, dE, dS = st["forces"] - plain["forces"], st["energy"] - plain["energy"], st["stress"] - plain["stress"]
    cvd, Vd = mdl.md_meta_hills(H, 1)
    figs = dict(F=np.abs(dF - want["forces"]).max(), E=abs(dE - want["energy"]), S=np.abs(dS - want["stress"]).max(),
                cv=np.abs(cvd[0] - want["cv"]).max(), V=abs(Vd[0] - want["energy"]))
    print(f"qlvar single {label} H={H}: cv {want['cv']} max|F_bias| {fb:.3e} V {want['energy']:.3e} gaps " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    return st, want, figs, tol, (row[0] - row0[0], dE), hills


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_evaluation_on_the_cases_of_the_fixture(models, name):
    frame, index, zi, zj, cutoff, ls = CASES[name]
    mdl, numbers, pos, cell, pbc = models(frame)
    index = int(np.where(numbers == zi)[0][0]) if index is None else index
    g17 = load("g17_qlvar")
    assert index == int(g17[f"{name}_index"]) and list(ls) == list(g17[f"{name}_l"])
    cvs = [("qlvar", index, zj, cutoff, ls)]
    tem = 900.0 if name in ("si32_a0", "mixed64_zr_c6") else None
    st, want, figs, tol, (drow, dE), _ = _check_single(mdl, numbers, pos, cell, pbc, cvs, 0.02, 0.05, tem, 257, seed=3, label=name)
    np.testing.assert_allclose(want["cv"], g17[f"{name}_Q"], rtol=1e-12)          # the twin's Q is the reference's
    assert np.abs(want["forces"]).max() > 0.01 and want["energy"] > 0              # the bias is not a rounding error of the model's forces
    assert figs["F"] <= tol and figs["E"] <= tol and figs["S"] <= tol, figs
    assert figs["cv"] <= 1e-13 * np.abs(want["cv"]).max() and figs["V"] <= tol
    assert drow == dE                                                              # the scalar row carries the biased energy too
    assert mdl.md_meta_info() == dict(D=len(ls), below=257, held=258, capacity=261)


def test_qlvar_beside_a_distance_and_a_second_qlvar(models):
    """Three components, D = 4: the rows of the two qlvars stand one behind the other in the kernel's LDS."""
    mdl, numbers, pos, cell, pbc = models("g5_mixed64")
    zr, o = int(np.where(numbers == 40)[0][0]), int(np.where(numbers == 8)[0][0])
    cvs = [("qlvar", zr, 8, 4.0, (4, 6)), ("distance", 0, len(numbers) - 1), ("qlvar", o, 8, 5.0, (6,))]
    st, want, figs, tol, _, _ = _check_single(mdl, numbers, pos, cell, pbc, cvs, [0.02, 0.02, 0.1, 0.02], 0.3, None, 300, seed=5, label="mixed64 ql + d + ql")
    assert np.abs(want["forces"]).max() > 0.01 and want["cv"][3] > 0.05
    assert figs["F"] <= tol and figs["E"] <= tol and figs["S"] <= tol and figs["V"] <= tol, figs
    assert figs["cv"] <= 1e-13 * np.abs(want["cv"]).max()


def test_an_empty_environment_is_zero_and_does_not_accumulate(models):
    """g5_cluster16 atom 14 has no neighbour inside the cutoff: Q = 0, no force from it; beside it a qlvar that does pull, and the
    same configuration evaluated twice gives the same bits."""
    mdl, numbers, pos, cell, pbc = models("g5_cluster16")
    assert np.diff(load("g5_cluster16")["nl_ptr"])[14] == 0
    cvs = [("qlvar", 14, 10, 6.0, (6,)), ("qlvar", 0, 10, 6.0, (6,))]
    st, want, figs, tol, _, hills = _check_single(mdl, numbers, pos, cell, pbc, cvs, 0.02, 0.05, None, 200, seed=4, label="cluster16 empty + a0", exact=(0,))
    assert want["cv"][0] == 0.0 and np.abs(want["forces"]).max() > 0.01
    assert figs["F"] <= tol and figs["E"] <= tol and figs["S"] <= tol and figs["V"] <= tol and figs["cv"] <= 1e-13, figs
    sc, code = mdl.md_run(1, final=True)                  # the same configuration again (a `final` call moved nothing)
    st2 = mdl.md_state(results=True)
    assert code == 0 and np.array_equal(st2["forces"], st["forces"]) and st2["energy"] == st["energy"] and np.array_equal(st2["stress"], st["stress"])
    assert mdl.md_meta_hills(200, 1)[0][0, 0] == 0.0
    # the empty one alone: the bias is there (a hill at Q = 0.01) and pulls on nobody
    row0, plain = _single(mdl, numbers, pos, cell, pbc)
    row, only = _single(mdl, numbers, pos, cell, pbc, cvs[:1], sigma=0.02, w=0.05, hills=np.array([[0.01]]), capacity=4)
    assert np.array_equal(only["forces"], plain["forces"]) and only["energy"] > plain["energy"]


def _twin_meta(mdl, var, sigma, w, tem):
    from autoforce_amd.meta import Meta
    m = Meta(var, sigma=sigma, w=w, tem=tem, hist=None)
    m.species, m.rc = list(mdl.species), RC
    return m


def _langevin_twin(mdl, numbers, pos, cell, pbc, vel, xi, meta, **kw):
    from autoforce_amd.workloads import langevin_nvt
    margin, out = np.inf, []
    for row in langevin_nvt(_PredictCalc(mdl), numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=DT_FS, friction=0.05, vel=vel, rng=_Rows(xi), meta=meta, **kw):
        out.append((row[1], row[4].copy(), row[5].copy()))
        margin = min(margin, meta.margin)
    return out, margin


QL_SI = [("qlvar", 0, 14, 4.0, (4, 6))]
QL_META = dict(sigma=0.004, w=0.02, tem=900.0)


def test_trajectory_against_the_twin(models):
    from autoforce_amd.meta import Qlvar
    mdl, numbers, pos, cell, pbc = models("g5_si32", SOFT)
    N = len(numbers)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    meta = _twin_meta(mdl, Qlvar(14, 14, index=0, cutoff=4.0, l=[4, 6]), **QL_META)
    assert meta.device_spec() == QL_SI
    host, margin = _langevin_twin(mdl, numbers, pos, cell, pbc, vel, xi, meta)
    assert margin > MARGIN, margin
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05)
    mdl.md_meta(QL_SI, capacity=STEPS + 2, **QL_META)
    sc, code = mdl.md_run(STEPS + 1, xi, final=True)
    assert code == 0 and len(sc) == STEPS + 1
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    cvd, Vd = mdl.md_meta_hills()
    dcv = np.abs(cvd - np.array(meta.hills)).max()
    print(f"qlvar trajectory: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e} dcv {dcv:.2e} max V {Vd.max():.3e} Q range {cvd.min(0)} {cvd.max(0)}")
    assert len(cvd) == STEPS + 1 and Vd.max() > 1e-3      # the walk revisits its hills: the bias acts
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL, (dx, dv)
    assert dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max()) and dcv <= TRAJ_RTOL


@pytest.mark.parametrize("merge", [None, 16], ids=["rows", "merge16"])
def test_cuts_and_halts_leave_the_same_bits(models, merge):
    mdl, numbers, pos, cell, pbc = models("g5_si32", SOFT)
    N = len(numbers)
    meta = dict(QL_META, **({} if merge is None else dict(merge=merge)))
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    one = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, meta)
    gate = float(np.sort(one[0][:, 11])[-3])                # the three largest covlosses of the run reach it
    runs = [one, _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, meta, cuts=7), _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, meta, ediff=gate),
            _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, meta), _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, meta, cuts=7, ediff=gate)]
    assert runs[2][4] >= 2 and runs[4][4] >= 2 and runs[0][4] == 0
    for r in runs[1:]:
        assert np.array_equal(r[0][:, :12], one[0][:, :12])
        assert np.array_equal(r[1], one[1]) and np.array_equal(r[2], one[2])
        assert np.array_equal(r[3][0], one[3][0]) and np.array_equal(r[3][1], one[3][1])
    assert len(one[3][0]) == STEPS + 1 and one[3][1].max() > 1e-3
    if merge:
        centres, counts, rows = mdl.md_meta_table()
        assert rows == (STEPS + 1) // merge * merge and counts.sum() == rows and centres.shape[1] == 2


def test_with_held_components_the_filter_and_the_record_together(models):
    from autoforce_amd.meta import Qlvar
    mdl, numbers, pos, cell, pbc = models("g5_si32", SOFT)
    N = len(numbers)
    fx = np.zeros((N, 3), bool)
    fx[0] = True                                           # the index atom of the qlvar
    fx[1, 2] = True
    kw = dict(fixed=fx, ml_filter=0.8, filter_init=(0.4 * np.random.default_rng(21).normal(size=(N, 3)), None))
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    meta = _twin_meta(mdl, Qlvar(14, 14, index=0, cutoff=4.0, l=[4, 6]), **QL_META)
    host, margin = _langevin_twin(mdl, numbers, pos, cell, pbc, vel, xi, meta, **kw)
    assert margin > MARGIN
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05, **kw)
    mdl.md_meta(QL_SI, capacity=STEPS + 2, **QL_META)
    mdl.md_record(8, velocities=True, results=True)
    sc, code = mdl.md_run(STEPS + 1, xi, final=True)
    assert code == 0
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    print(f"qlvar composed: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e}")
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL and dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max())
    assert np.array_equal(st["positions"][fx], pos[fx]) and not st["velocities"][fx].any()
    # what the run reports is the model's results plus the bias of the hills below the configuration — on the held atoms too
    hills = mdl.md_meta_hills(0, STEPS + 1)[0]
    fr = mdl.md_frames()
    assert list(fr["index"]) == list(range(0, STEPS + 1, 8)) and np.array_equal(fr["energy"], sc[fr["index"], 0])
    for k in (4, 8):
        n = int(fr["index"][k])
        plain = mdl.predict(numbers, fr["positions"][k], cell, pbc)
        want = _bias(mdl, QL_SI, QL_META["sigma"], QL_META["w"], numbers, fr["positions"][k], cell, pbc, hills[:n], tem=QL_META["tem"])
        fb, fm = np.abs(want["forces"]).max(), np.abs(plain["forces"]).max()
        assert fb > 1e-3 and np.abs(want["forces"][0]).max() > 1e-4
        assert np.abs(fr["forces"][k] - plain["forces"] - want["forces"]).max() <= 1e-12 * max(fb, fm)
        assert np.abs(fr["stress"][k] - plain["stress"] - want["stress"]).max() <= 1e-12 * max(np.abs(plain["stress"]).max(), np.abs(want["stress"]).max())
    assert np.array_equal(fr["forces"][8], st["forces"]) and np.array_equal(fr["stress"][8], st["stress"])


def test_a_spec_without_a_qlvar_keeps_its_bits_around_a_qlvar_run(models):
    mdl, numbers, pos, cell, pbc = models("g5_si32", SOFT)
    N = len(numbers)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    d = [("distance", 0, 5)]
    dm = dict(sigma=0.02, w=0.3, tem=900.0)
    before = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, d, dm)
    ql = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, QL_SI, QL_META)
    after = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, d, dm)
    mixed = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, d + QL_SI, dict(sigma=[0.02, 0.004, 0.004], w=0.3, tem=900.0))
    for k in range(3):
        assert np.array_equal(before[k] if k else before[0][:, :12], after[k] if k else after[0][:, :12])
    assert np.array_equal(before[3][0], after[3][0]) and np.array_equal(before[3][1], after[3][1])
    assert not np.array_equal(ql[1], before[1]) and mixed[3][0].shape == (STEPS + 1, 3)
    assert np.array_equal(mixed[3][0][0, :1], before[3][0][0])      # the distance of configuration 0 is the distance


def test_refusals(models):
    from autoforce_amd import SgprError, _lib
    mdl, numbers, pos, cell, pbc = models("g5_si32")
    lib = _lib.load()
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers))

    def invalid(fn, word):
        with pytest.raises(SgprError) as e:
            fn()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 6.5, (6,))], 0.02, 0.1), "cutoff <= rc")           # the list ends at rc = 6
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 0.0, (6,))], 0.02, 0.1), "cutoff")
    invalid(lambda: mdl.md_meta([("qlvar", len(numbers), 14, 4.0, (6,))], 0.02, 0.1), "atom")
    invalid(lambda: mdl.md_meta([("qlvar", 0, 8, 4.0, (6,))], 0.02, 0.1), "species")                 # no oxygen here
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 4.0, (13,))], 0.02, 0.1), "l = 13")
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 4.0, (-1,))], 0.02, 0.1), "l = -1")
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 4.0, ())], 0.02, 0.1), "values of l")
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 4.0, (2, 4, 6, 8)), ("qlvar", 1, 14, 4.0, (2, 4, 6))], 0.02, 0.1), "dimensions")   # D = 7
    invalid(lambda: mdl.md_meta([("qlvar", 0, 14, 4.0, (6,))], 0.02, 0.1, hills=np.array([[np.nan]])), "not a number")
    # a kind-2 component whose parameters nobody staged — and what was staged for a call that failed is gone with it
    spec = _lib.i32(np.array([2, 0, 14], np.int32))
    sg = _lib.f64(np.array([0.02]))
    args = (mdl.handle, 1, _lib.ptr(spec), _lib.ptr(sg), 0.1, 0.0, 1, 8, 0, None, None)
    assert lib.sgpr_md_meta(*args) == -1 and "sgpr_md_meta_ql" in lib.sgpr_last_error().decode()
    ls = _lib.i32(np.array([6], np.int32))
    assert lib.sgpr_md_meta_ql(mdl.handle, 0, 4.0, 1, _lib.ptr(ls)) == 0
    assert lib.sgpr_md_meta(mdl.handle, 1, _lib.ptr(_lib.i32(np.array([2, 99, 14], np.int32))), _lib.ptr(sg), 0.1, 0.0, 1, 8, 0, None, None) == -1
    assert lib.sgpr_md_meta(*args) == -1 and "sgpr_md_meta_ql" in lib.sgpr_last_error().decode()
    assert lib.sgpr_md_meta_ql(mdl.handle, 4, 4.0, 1, _lib.ptr(ls)) == -1 and lib.sgpr_md_meta_ql(mdl.handle, 0, 4.0, 7, _lib.ptr(ls)) == -1
    # staged and attached: the run runs, D is what the stage said
    assert lib.sgpr_md_meta_ql(mdl.handle, 0, 4.0, 1, _lib.ptr(ls)) == 0 and lib.sgpr_md_meta(*args) == 0
    sc, code = mdl.md_run(3)
    assert code == 0 and mdl.md_meta_info()["D"] == 1 and mdl.md_meta_info()["below"] == 3
    # what the device bias does not serve still names the host path
    from autoforce_amd.workloads import FS
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers), ttime=20.0 * FS, pfactor=1e3)
    with pytest.raises(NotImplementedError, match="host loop"):
        mdl.md_meta([("qlvar", 0, 14, 4.0, (6,))], 0.02, 0.1)
