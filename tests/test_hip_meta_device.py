"""GPU tests of metadynamics inside the device MD loop (sgpr_md_meta, md_meta_kernel; the reference's calculator/meta.py by
evaluation index) against the host twin workloads.meta_bias / workloads.*(meta=) around the same library, on the small golden
frames with their own fitted models.

  Every comparison with the twin asserts its precondition: over the run no CV component comes within 1e-6 sigma of a bin edge
k sigma or a block edge k 5 sigma (the twin reports the smallest margin) — there a last-bit difference moves a hill by a whole
bin and proves nothing.
  A single evaluation (configuration 0, preloaded hills, md_run(1, final=True)): forces, energy and stress of md_state minus the
same run without a bias, and the hill row, against meta_bias to 1e-12 of the largest bias force — sums of a few hundred terms
each within a few ulp.  Hill counts at the edges of the kernel's strided sum (256 threads, 1024 hills per trip), a dense posvar
on 36 atoms (no multiple of 16) and on 64, a distance between the first and the last atom in caller order (different species:
both ends of the permutation), and a CV atom without a neighbour inside the cutoff evaluated twice (Fself does not accumulate).
  Trajectories of 64 steps, D = 4, plain and well-tempered, against workloads.langevin_nvt / nose_hoover_nvt(meta=): the
largest deviation of positions and velocities measured on the first run was 1.53e-16 relative (a velocity of the Langevin
run; every position had the twin's bits); the bound is 100 times that.
  Bit for bit: the same run as one call, as calls of 7, and halted by the covloss gate with the halted configuration evaluated
again, and all of it repeated — positions, velocities and every hill row.
  With held components, the update-jump filter and the frame record, each alone and together; the capacity; the refusals, a run
begun on two ranks included."""
import numpy as np
import pytest

from helpers import load
from test_hip_fixed_device import _Rows
from test_hip_npt_device import _PredictCalc

pytestmark = pytest.mark.gpu

T, STEPS, DT_FS = 600.0, 64, 0.5
SOFT = 0.05   # the trajectories run on the golden models with their weights scaled down: forces of order 0.1 eV/A keep the walk near its hills
MARGIN = 1e-6
TRAJ_RTOL = 1.53e-14    # 100 x the largest deviation measured on the first run (1.53e-16), never looser than 1e-8
assert TRAJ_RTOL <= 1e-8


def D4(numbers):
    """Catvar(Posvar(1, select=Z), distance(first, last))"""
    return [("posvar", 1, int(numbers[1])), ("distance", 0, len(numbers) - 1)]


def _model(frame, scale=1.0):
    from autoforce_amd import Local, SGPRModel
    g = load(frame)
    mdl = SGPRModel(int(g["lmax"]), int(g["nmax"]), float(g["eta"]), float(g["rc"]), species=g["species"].tolist())
    ptr = g["ind_ptr"]
    mdl.set_inducing([Local(int(z), g["ind_nbr_z"][ptr[q]:ptr[q + 1]], g["ind_nbr_r"][ptr[q]:ptr[q + 1]]) for q, z in enumerate(g["ind_z"])])
    mdl.set_weights(scale * g["mu"], choli=g["choli"])
    return mdl, g["numbers"], g["positions"], g["cell"], g["pbc"]


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(frame, scale=1.0):
        if (frame, scale) not in cache:
            cache[frame, scale] = _model(frame, scale)
        return cache[frame, scale]
    yield get
    for m in cache.values():
        m[0].close()


def _masses(numbers):
    from autoforce_amd.workloads import MASS
    extra = {10: 20.18, 18: 39.948, 29: 63.546, 47: 107.868}
    return np.array([MASS.get(int(z), extra.get(int(z), 1.0)) for z in numbers])


def _begin(mdl, numbers, pos, cell, pbc, vel=None, friction=0.0, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl.md_begin(numbers, pos, cell, pbc, _masses(numbers), vel, dt=DT_FS * FS, friction=friction, kT=kB * T, **kw)


def _single(mdl, numbers, pos, cell, pbc, cvs=None, **meta):
    _begin(mdl, numbers, pos, cell, pbc)
    if cvs:
        mdl.md_meta(cvs, **meta)
    sc, code = mdl.md_run(1, final=True)
    assert code == 0 and len(sc) == 1
    return sc[0], mdl.md_state(results=True)


def _check_single(mdl, numbers, pos, cell, pbc, cvs, sigma, w, tem, H, seed=1, label=""):
    from autoforce_amd.workloads import meta_bias
    cv0 = meta_bias(cvs, sigma, w, numbers, pos, cell, None, species=mdl.species)["cv"]
    hills = cv0 + 1.2 * np.asarray(sigma) * np.random.default_rng(seed).normal(size=(H, len(cv0)))
    want = meta_bias(cvs, sigma, w, numbers, pos, cell, hills, tem=tem, species=mdl.species)
    assert want["margin"] > MARGIN, want["margin"]
    row0, plain = _single(mdl, numbers, pos, cell, pbc)
    row, st = _single(mdl, numbers, pos, cell, pbc, cvs, sigma=sigma, w=w, tem=tem, hills=hills, capacity=H + 4)
    fb = np.abs(want["forces"]).max()
    tol = 1e-12 * fb
    dF, dE, dS = st["forces"] - plain["forces"], st["energy"] - plain["energy"], st["stress"] - plain["stress"]
    cvd, Vd = mdl.md_meta_hills(H, 1)
    figs = dict(F=np.abs(dF - want["forces"]).max(), E=abs(dE - want["energy"]), S=np.abs(dS - want["stress"]).max(),
                cv=np.abs(cvd[0] - want["cv"]).max(), V=abs(Vd[0] - want["energy"]))
    print(f"meta single {label} H={H}: max|F_bias| {fb:.3e} V {want['energy']:.3e} gaps " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    if H:
        assert fb > 0.01 and want["energy"] > 0          # the bias is not a rounding error of the model's forces (well-tempered: of order kT / sigma at most)
    assert figs["F"] <= tol and figs["E"] <= tol and figs["S"] <= tol, figs
    assert figs["cv"] <= 1e-13 * np.abs(want["cv"]).max() and figs["V"] <= tol
    assert row[0] - row0[0] == dE                         # the scalar row carries the biased energy too
    assert mdl.md_meta_info() == dict(D=len(cv0), below=H, held=H + 1, capacity=H + 4)
    return st


@pytest.mark.parametrize("H", [0, 1, 255, 256, 257, 1024, 1025])
def test_single_evaluation_at_the_hill_counts_where_the_strided_sum_turns(models, H):
    mdl, numbers, pos, cell, pbc = models("g5_mixed64")
    assert numbers[0] != numbers[-1]                       # first and last atom in caller order, of different species
    _check_single(mdl, numbers, pos, cell, pbc, [("distance", 0, len(numbers) - 1)], 0.1, 1.5, None, H, label="distance mixed64")


@pytest.mark.parametrize("frame", ["g5_bigtric36", "g5_mixed64", "g5_si32"])
@pytest.mark.parametrize("tem", [None, 900.0], ids=["plain", "wt"])
def test_single_evaluation_dense_posvar_and_catvar(models, frame, tem):
    mdl, numbers, pos, cell, pbc = models(frame)
    _check_single(mdl, numbers, pos, cell, pbc, [("posvar", 3, None)], [0.1, 0.15, 0.2], 25.0, tem, 300, seed=2, label=f"posvar dense {frame}")
    _check_single(mdl, numbers, pos, cell, pbc, D4(numbers), 0.2, 90.0, tem, 257, seed=3, label=f"D4 {frame}")


def test_an_atom_without_neighbours_does_not_accumulate_the_bias(models):
    """g5_cluster16: atoms 14 and 15 have no neighbour inside the cutoff.  The reverse pass stores their Fself (zeros) every
    step: the bias evaluated twice at the same configuration gives the same bits, and it is the whole force on such an atom."""
    from autoforce_amd.workloads import meta_bias
    mdl, numbers, pos, cell, pbc = models("g5_cluster16")
    g = load("g5_cluster16")
    assert np.diff(g["nl_ptr"])[14] == 0
    cvs = [("distance", 0, 14), ("posvar", 15, None)]
    st = _check_single(mdl, numbers, pos, cell, pbc, cvs, 0.15, 40.0, None, 200, seed=4, label="cluster16 lonely atoms")
    sc, code = mdl.md_run(1, final=True)                  # the same configuration again (a `final` call moved nothing)
    st2 = mdl.md_state(results=True)
    assert code == 0 and np.array_equal(st2["forces"], st["forces"]) and st2["energy"] == st["energy"]
    hills = mdl.md_meta_hills(0, 200)[0]
    want = meta_bias(cvs, 0.15, 40.0, numbers, pos, cell, hills, species=mdl.species)
    assert np.abs(st["forces"][14] - want["forces"][14]).max() <= 1e-12 * np.abs(want["forces"]).max()
    assert np.abs(want["forces"][14]).max() > 0


def _twin(mdl, numbers, pos, cell, pbc, vel, how, meta, xi=None, **kw):
    from autoforce_amd.workloads import langevin_nvt, nose_hoover_nvt
    calc = _PredictCalc(mdl)
    if how == "nose-hoover":
        loop = nose_hoover_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=DT_FS, tdamp_fs=20.0, vel=vel, species=mdl.species, meta=meta, **kw)
    else:
        loop = langevin_nvt(calc, numbers, pos, cell, pbc, STEPS, temperature=T, dt_fs=DT_FS, friction=0.05 if how == "langevin" else 0.0, vel=vel,
                            rng=_Rows(xi), meta=meta, **kw)
    margin, out = np.inf, []
    for row in loop:
        out.append((row[1], row[4].copy(), row[5].copy()))
        margin = min(margin, meta.margin)
    return out, margin


def _vel(numbers, seed=3):
    from autoforce_amd.ase_shim import kB
    return np.random.default_rng(seed).normal(size=(len(numbers), 3)) * np.sqrt(kB * T / _masses(numbers))[:, None]


def _twin_meta(mdl, numbers, sigma, w, tem, pace=1):
    """The Meta of D4(numbers), its posvar's mean summed in the order of the model's species table."""
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    m = Meta(Catvar(Posvar(1, select=int(numbers[1])), Distance(0, len(numbers) - 1)), sigma=sigma, w=w, tem=tem, pace=pace, hist=None)
    assert m.device_spec() == D4(numbers)
    m.species = list(mdl.species)
    return m


@pytest.mark.parametrize("tem", [None, 900.0], ids=["plain", "wt"])
@pytest.mark.parametrize("how", ["langevin", "verlet", "nose-hoover"])
def test_trajectory_against_the_twin(models, how, tem):
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36", SOFT)
    N = len(numbers)
    cvs, sigma, w = D4(numbers), 0.05, 0.3
    vel = _vel(numbers)
    xi = np.random.default_rng(9).normal(size=(STEPS + 1, N, 3)) if how == "langevin" else np.zeros((STEPS + 1, N, 3))
    host, margin = _twin(mdl, numbers, pos, cell, pbc, vel, how, _twin_meta(mdl, numbers, sigma, w, tem), xi=xi)
    assert margin > MARGIN, margin
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05 if how == "langevin" else 0.0, ttime=20.0 * FS if how == "nose-hoover" else None)
    mdl.md_meta(cvs, sigma, w, tem=tem, capacity=STEPS + 2)
    sc, code = mdl.md_run(STEPS + 1, xi if how == "langevin" else None, final=True)
    assert code == 0 and len(sc) == STEPS + 1
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    cvd, Vd = mdl.md_meta_hills()
    print(f"meta trajectory {how} tem={tem}: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e} max V {Vd.max():.3e}")
    assert len(cvd) == STEPS + 1 and Vd.max() > 1e-3      # the walk revisits its hills: the bias acts
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL, (dx, dv)
    assert dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max())


def _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta, cuts=None, ediff=0.0, capacity=STEPS + 2, **begin):
    """The run of STEPS + 1 evaluations in calls of `cuts` (None: one call), halted by the gate where ediff says so — the halted
    configuration is evaluated again by a call of one (the model is what it was) — until every configuration is through."""
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05, **begin)
    mdl.md_meta(cvs, capacity=capacity, **meta)
    done, halts, rows = 0, 0, []
    total = STEPS + 1
    again = False
    while done < total:
        n = 1 if again else min(cuts or total, total - done)
        sc, code = mdl.md_run(n, xi[done:done + n], ediff=0.0 if again else ediff, final=(done + n == total))
        assert code in (0, 1)
        acc = len(sc) - 1 if code == 1 else len(sc)
        rows.extend(sc[:acc])
        done += acc
        again = code == 1
        halts += code == 1
    st = mdl.md_state(results=True)
    return np.array(rows), st["positions"], st["velocities"], mdl.md_meta_hills(), halts


def test_cuts_and_halts_leave_the_same_bits(models):
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36", SOFT)
    N = len(numbers)
    cvs, meta = D4(numbers), dict(sigma=0.05, w=0.3, tem=900.0)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    one = _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta)
    cov = one[0][:, 11]
    gate = float(np.sort(cov)[-3])                         # the three largest covlosses of the run reach it
    runs = [one, _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta, cuts=7), _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta, ediff=gate),
            _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta), _cut_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta, cuts=7, ediff=gate)]
    assert runs[2][4] >= 2 and runs[4][4] >= 2 and runs[0][4] == 0
    for r in runs[1:]:
        assert np.array_equal(r[0][:, :12], one[0][:, :12])
        assert np.array_equal(r[1], one[1]) and np.array_equal(r[2], one[2])
        assert np.array_equal(r[3][0], one[3][0]) and np.array_equal(r[3][1], one[3][1])
    assert len(one[3][0]) == STEPS + 1 and one[3][1].max() > 1e-3


def test_pace_deposits_every_third_configuration(models):
    mdl, numbers, pos, cell, pbc = models("g5_si32")
    from autoforce_amd.workloads import meta_bias
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers))
    mdl.md_meta([("distance", 0, 5)], 0.02, 3.0, pace=3, capacity=8)
    sc, code = mdl.md_run(7)                               # configurations 0 ... 6: deposits at 0, 3, 6
    assert code == 0 and mdl.md_meta_info()["below"] == 3
    cvd, Vd = mdl.md_meta_hills()
    assert len(cvd) == 3 and Vd[0] == 0.0
    x3 = mdl.md_state(which=-1)["positions"]               # configuration 6
    assert abs(meta_bias([("distance", 0, 5)], 0.02, 3.0, numbers, x3, cell, None)["cv"][0] - cvd[2, 0]) <= 1e-14 * cvd[2, 0]


@pytest.mark.parametrize("kind", ["fixed", "filter", "record", "all"])
def test_with_held_components_the_filter_and_the_record(models, kind):
    """Each on its own and all three together, on the golden model as it is, against the twin with the same keywords.  fixed= on
    atoms of the CV: the coordinates keep their bits and the force reported on them includes the bias; ml_filter= with accumulators
    that are not zero; md_record: the frames carry the biased energy, forces and stress."""
    import autoforce_amd.workloads as wl
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36")
    N = len(numbers)
    cvs, sigma, w = D4(numbers), 0.05, 0.3
    fx = np.zeros((N, 3), bool)
    fx[1] = True                                           # the index atom of the posvar
    fx[N - 1, 2] = True                                    # a component of the distance's far end
    f0 = 0.4 * np.random.default_rng(21).normal(size=(N, 3))
    kw = {}
    if kind in ("fixed", "all"):
        kw.update(fixed=fx)
    if kind in ("filter", "all"):
        kw.update(ml_filter=0.8, filter_init=(f0, None))
    rec = kind in ("record", "all")
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    host, margin = _twin(mdl, numbers, pos, cell, pbc, vel, "langevin", _twin_meta(mdl, numbers, sigma, w, None), xi=xi, **kw)
    assert margin > MARGIN
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05, **kw)
    mdl.md_meta(cvs, sigma, w, capacity=STEPS + 2)
    if rec:
        mdl.md_record(8, velocities=True, results=True)
    sc, code = mdl.md_run(STEPS + 1, xi, final=True)
    assert code == 0
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    print(f"meta composed {kind}: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e}")
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL and dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max())
    if "fixed" in kw:
        assert np.array_equal(st["positions"][fx], pos[fx]) and not st["velocities"][fx].any()
    # what the run reports at a configuration is the model's results plus the bias of the hills below it — on the held atoms too
    hills = mdl.md_meta_hills(0, STEPS + 1)[0]

    def biased(x, n):
        plain = mdl.predict(numbers, x, cell, pbc)
        b = wl.meta_bias(cvs, sigma, w, numbers, x, cell, hills[:n], species=mdl.species)
        return plain, b
    plain, want = biased(st["positions"], STEPS)
    fb, fm = np.abs(want["forces"]).max(), np.abs(plain["forces"]).max()
    assert fb > 1e-3 and np.abs(want["forces"][1]).max() > 1e-4
    assert np.abs(st["forces"] - plain["forces"] - want["forces"]).max() <= 1e-12 * max(fb, fm)
    if rec:
        fr = mdl.md_frames()
        assert list(fr["index"]) == list(range(0, STEPS + 1, 8))
        assert np.array_equal(fr["energy"], sc[fr["index"], 0])
        np.testing.assert_allclose(fr["energy"], [host[i][0] for i in fr["index"]], rtol=TRAJ_RTOL, atol=TRAJ_RTOL)
        for k in (4, 8):                                    # configurations 32 and 64: forces and stress of the frame
            n = int(fr["index"][k])
            plain, want = biased(fr["positions"][k], n)
            assert np.abs(fr["forces"][k] - plain["forces"] - want["forces"]).max() <= 1e-12 * max(fb, fm)
            assert np.abs(fr["stress"][k] - plain["stress"] - want["stress"]).max() <= 1e-12 * max(np.abs(plain["stress"]).max(), np.abs(want["stress"]).max())
            assert abs(fr["energy"][k] - plain["energy"] - want["energy"]) <= 1e-12 * max(1.0, abs(plain["energy"]))
        assert np.array_equal(fr["forces"][8], st["forces"]) and np.array_equal(fr["stress"][8], st["stress"])


def test_capacity_is_checked_before_anything_is_enqueued_and_the_run_goes_on_with_more_room(models):
    from autoforce_amd import SgprError
    mdl, numbers, pos, cell, pbc = models("g5_si32")
    N = len(numbers)
    cvs, meta = [("distance", 0, 5), ("posvar", 2, None)], dict(sigma=0.02, w=2.0)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(40, N, 3))
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05)
    mdl.md_meta(cvs, capacity=64, **meta)
    mdl.md_run(16, xi[:16])
    sc_ref, _ = mdl.md_run(24, xi[16:40], final=True)
    ref = mdl.md_state(results=True)
    ref_hills = mdl.md_meta_hills()
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05)
    mdl.md_meta(cvs, capacity=20, **meta)
    mdl.md_run(16, xi[:16])
    before = (mdl.md_state(), mdl.md_meta_info())
    with pytest.raises(SgprError) as e:
        mdl.md_run(24, xi[16:40], final=True)
    assert e.value.code == -1 and "capacity" in str(e.value)
    after = (mdl.md_state(), mdl.md_meta_info())
    assert after[1] == before[1] and all(np.array_equal(after[0][k], before[0][k]) for k in ("positions", "velocities_pre"))
    cvh, Vh = mdl.md_meta_hills(0, before[1]["below"])
    mdl.md_meta(cvs, capacity=64, hills=(cvh, Vh), **meta)
    info = mdl.md_meta_info()                              # (attached anew: the rows given stand, nothing else until the run goes on)
    assert info["below"] == info["held"] == len(cvh) and info["capacity"] == 64
    sc, code = mdl.md_run(24, xi[16:40], final=True)
    st = mdl.md_state(results=True)
    assert code == 0 and np.array_equal(sc[:, :12], sc_ref[:, :12])
    assert np.array_equal(st["positions"], ref["positions"]) and np.array_equal(st["velocities"], ref["velocities"])
    got = mdl.md_meta_hills()
    assert np.array_equal(got[0], ref_hills[0]) and np.array_equal(got[1], ref_hills[1])


def test_what_the_device_bias_does_not_serve_is_refused_with_the_host_path_named(models):
    from autoforce_amd import SgprError
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc = models("g5_si32")
    other = models("g5_bigtric36")[0]
    cvs = [("distance", 0, 5)]

    def refused(fn):
        with pytest.raises((NotImplementedError, SgprError)) as e:
            fn()
        assert isinstance(e.value, NotImplementedError) or e.value.code == -6, e.value
        assert "host loop" in str(e.value) and "calculate()" in str(e.value), str(e.value)

    # a barostat
    assert np.array_equal(cell, np.triu(cell))
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers), ttime=20.0 * FS, pfactor=1e3)
    refused(lambda: mdl.md_meta(cvs, 0.1, 0.1))
    # a relaxation
    mdl.relax_begin(numbers, pos, cell, pbc, 0.05)
    refused(lambda: mdl.md_meta(cvs, 0.1, 0.1))
    # a band
    mdl.neb_begin(numbers, np.array([pos, pos + 0.01, pos + 0.02]), cell, pbc, 0.05)
    refused(lambda: mdl.md_meta(cvs, 0.1, 0.1))
    # a committee, from either side
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers))
    mdl.md_meta(cvs, 0.1, 0.1)
    refused(lambda: mdl.md_committee([other]))
    # the scatter form of the step: refused by md_run before anything is enqueued, the state as it was; back in the gather form the run runs
    from autoforce_amd import _lib
    _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"reverse_scatter", 1))
    before = mdl.md_state()
    refused(lambda: mdl.md_run(3))
    assert all(np.array_equal(mdl.md_state()[k], before[k]) for k in ("positions", "velocities_pre"))
    _lib.check(_lib.load().sgpr_set_option(mdl.handle, b"reverse_scatter", 0))
    sc, code = mdl.md_run(3)
    assert code == 0 and len(sc) == 3 and mdl.md_meta_info()["below"] == 3
    # bad arguments are errors of their own
    for bad in (dict(cvs=[("distance", 0, 0)]), dict(cvs=[("distance", 0, len(numbers))]), dict(cvs=[("posvar", 0, 99)]),
                dict(cvs=[("posvar", 0, None)] * 3), dict(cvs=cvs, pace=0), dict(cvs=cvs, sigma=0.0)):
        kw = dict(sigma=0.1, w=0.1)
        kw.update(bad)
        with pytest.raises(SgprError) as e:
            mdl.md_meta(**kw)
        assert e.value.code == -1, bad
    # ... and a run without a bias is the run it was: detached, the rows are those of a run that never had one
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers))
    a, _ = mdl.md_run(5)
    _begin(mdl, numbers, pos, cell, pbc, _vel(numbers))
    mdl.md_meta(cvs, 0.1, 0.1)
    mdl.md_meta(None, 0.1, 0.1)
    b, _ = mdl.md_run(5)
    assert np.array_equal(a, b)
    with pytest.raises(SgprError):
        mdl.md_meta_info()


def _two_rank_worker(rank, world, port, q):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch.distributed as dist
    from autoforce_amd import SgprError
    from autoforce_amd.watchdog import Watchdog
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SGPR_PEER_TIMEOUT_MS"] = "20000"   # (the processes share the one GPU of the test box)
    with Watchdog(f"metadynamics on two ranks, rank {rank} of {world}", seconds=240, rank=rank):
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mdl, numbers, pos, cell, pbc = _model("g5_si32")
        N = len(numbers)
        blobs = [None] * world
        dist.all_gather_object(blobs, mdl.peer_export(rank, world, 7 * N + 11))
        mdl.peer_attach(blobs)
        dist.barrier()
        e0 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        mdl.md_begin(numbers, pos, cell, pbc, np.ones(N), None, dt=1.0, friction=0.0, kT=0.0)
        said = ""
        try:
            mdl.md_meta([("distance", 0, 5)], 0.1, 0.1)
        except (NotImplementedError, SgprError) as e:
            said = type(e).__name__ + ": " + str(e)
        e1 = float(mdl.predict(numbers, pos, cell, pbc, rank=rank, world=world)["energy"])
        q.put((rank, said, e0, e1))
        dist.barrier()
        mdl.peer_destroy()
        dist.destroy_process_group()


def test_a_run_begun_on_two_ranks_refuses_the_bias_and_goes_on_working():
    """The bias runs on one rank: md_meta says so on every rank of a run begun on two, naming the host path, and the handles go
    on predicting."""
    import os
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29870 + (os.getpid() % 40)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, said, e0, e1 in got:
        assert said.startswith("NotImplementedError") and "2 ranks" in said and "host loop around calculate()" in said, said
        assert e0 == e1
    assert got[0][2] == got[1][2]
