"""GPU tests of the merged form of the device bias (sgpr_md_meta_merge, md_meta_merge_kernel, md_meta_merged_kernel) against the
host twin workloads.meta_bias(merge=) / meta_table / workloads.*(meta=Meta(..., merge=)) around the same library, through the
helpers of tests/test_hip_meta_device.py, on the small golden frames with their own models.

  A single evaluation with preloaded hills, CH = 8: hill counts that make the tail empty and CH - 1 long and, with every hill in
a bin of its own, take the table across 256 and 1024 entries, where the strided sum turns; a second draw confined to about five
bins (counts above one).  Forces, energy, stress and the hill row against the twin at _check_single's tolerances (1e-12 of the
largest bias force, 1e-13 on the CV), the margin precondition asserted; md_meta_table() against meta_table exactly, the entry
order included.
  Merging inside the loop: 64-step trajectories against the twin within TRAJ_RTOL, the table at the end, the merges counted.
  Bit for bit: one call, calls of 7, halts of the covloss gate — at a chunk crossing and at the configuration in front of one,
where the speculative step behind the halted configuration has merged a chunk the halted one must not see —, the run attached
again from md_meta_hills, all of it repeated.
  Unmerged unchanged; the surface's refusals."""
import numpy as np
import pytest

from test_hip_meta_device import (D4, MARGIN, STEPS, TRAJ_RTOL, SOFT, _begin, _single, _twin, _twin_meta, _vel, models)  # noqa: F401

pytestmark = pytest.mark.gpu

CH = 8
HS = [0, 7, 8, 9, 16, 263, 264, 265, 1032, 1033]

CASES = {
    "distance": ("g5_mixed64", lambda numbers: [("distance", 0, len(numbers) - 1)], 0.1, 1.5),
    "posvar": ("g5_si32", lambda numbers: [("posvar", 3, None)], [0.1, 0.15, 0.2], 25.0),
    "D4": ("g5_bigtric36", D4, 0.2, 90.0),
}


def _draw(cv0, sigma, H, how, seed=1):
    """own: every hill in a bin of its own, side by side along the first dimension from one bin below the CV upwards (one-sided: the
    bias force is no rounding error of the model's); few: all within about five bins, one-sided too"""
    sg = np.broadcast_to(np.asarray(sigma, float), cv0.shape)
    off = np.zeros((H, len(cv0)))
    if how == "own":
        off[:, 0] = (np.arange(H) - 1) * sg[0]
    else:
        off[:, 0] = sg[0] * np.random.default_rng(seed).uniform(-0.5, 4.5, size=H)
    return cv0 + off


def _table_equals(mdl, hills, sigma, ch, D):
    from autoforce_amd.workloads import meta_table
    sg = np.broadcast_to(np.asarray(sigma, float), (D,))
    tc, _, cnt, B = meta_table(np.asarray(hills).reshape(-1, D), sg, ch)
    centres, counts, rows = mdl.md_meta_table()
    assert rows == B, (rows, B)
    assert centres.shape == tc.shape and np.array_equal(centres, tc) and np.array_equal(counts, cnt)   # (the entry order included)
    return len(cnt), (cnt.max() if len(cnt) else 0.0)


def _check_single_merged(mdl, frame, plain_cache, numbers, pos, cell, pbc, cvs, sigma, w, tem, hills, ch, label=""):
    from autoforce_amd.workloads import meta_bias
    H = len(hills)
    want = meta_bias(cvs, sigma, w, numbers, pos, cell, hills, tem=tem, species=mdl.species, merge=ch)
    assert want["margin"] > MARGIN, want["margin"]
    if frame not in plain_cache:
        plain_cache[frame] = _single(mdl, numbers, pos, cell, pbc)
    row0, plain = plain_cache[frame]
    row, st = _single(mdl, numbers, pos, cell, pbc, cvs, sigma=sigma, w=w, tem=tem, hills=hills if H else None, capacity=H + 4, merge=ch)
    fb = np.abs(want["forces"]).max()
    tol = 1e-12 * fb
    dF, dE, dS = st["forces"] - plain["forces"], st["energy"] - plain["energy"], st["stress"] - plain["stress"]
    cvd, Vd = mdl.md_meta_hills(H, 1)
    figs = dict(F=np.abs(dF - want["forces"]).max(), E=abs(dE - want["energy"]), S=np.abs(dS - want["stress"]).max(),
                cv=np.abs(cvd[0] - want["cv"]).max(), V=abs(Vd[0] - want["energy"]))
    T, cmax = _table_equals(mdl, hills, sigma, ch, len(want["cv"]))
    print(f"meta merged single {label} H={H} CH={ch}: entries {T} largest count {cmax:.0f} max|F_bias| {fb:.3e} V {want['energy']:.3e} gaps "
          + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    if H:
        assert fb > 0.01 and want["energy"] > 0            # (as _check_single: the bias is not a rounding error of the model's forces)
    assert figs["F"] <= tol and figs["E"] <= tol and figs["S"] <= tol, figs
    assert figs["cv"] <= 1e-13 * np.abs(want["cv"]).max() and figs["V"] <= tol
    assert row[0] - row0[0] == dE
    assert mdl.md_meta_info() == dict(D=len(want["cv"]), below=H, held=H + 1, capacity=H + 4)
    return T, cmax


@pytest.fixture(scope="module")
def plain_cache():
    return {}


@pytest.mark.parametrize("how", ["own", "few"])
@pytest.mark.parametrize("tem", [None, 900.0], ids=["plain", "wt"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_single_evaluation_with_preloaded_hills(models, plain_cache, case, tem, how):
    from autoforce_amd.workloads import meta_bias
    frame, spec, sigma, w = CASES[case]
    mdl, numbers, pos, cell, pbc = models(frame)
    cvs = spec(numbers)
    cv0 = meta_bias(cvs, sigma, w, numbers, pos, cell, None, species=mdl.species)["cv"]
    for H in HS:
        T, cmax = _check_single_merged(mdl, frame, plain_cache, numbers, pos, cell, pbc, cvs, sigma, w, tem, _draw(cv0, sigma, H, how), CH,
                                       label=f"{case} {frame} {how}")
        B = (H // CH) * CH
        if how == "own":
            assert T == B                                   # 264 and 1032 entries: across 256 and 1024
        elif B >= 16:
            assert T <= 7 and cmax > 1


@pytest.mark.parametrize("ch,H", [(1, 300), (257, 600)])
def test_single_evaluation_with_other_chunk_lengths(models, plain_cache, ch, H):
    """CH = 1: no tail, every row merged on its own launch; CH = 257: a chunk longer than the merge kernel's 256 rows at a time."""
    from autoforce_amd.workloads import meta_bias
    frame, spec, sigma, w = CASES["D4"]
    mdl, numbers, pos, cell, pbc = models(frame)
    cvs = spec(numbers)
    cv0 = meta_bias(cvs, sigma, w, numbers, pos, cell, None, species=mdl.species)["cv"]
    hills = cv0 + 1.2 * sigma * np.random.default_rng(3).normal(size=(H, len(cv0)))
    T, cmax = _check_single_merged(mdl, frame, plain_cache, numbers, pos, cell, pbc, cvs, sigma, w, None, hills, ch, label=f"D4 CH={ch}")
    assert T > 50


def _pre(mdl, numbers, pos, cell, cvs, sigma, n=13):
    from autoforce_amd.workloads import meta_bias
    cv0 = meta_bias(cvs, sigma, 1.0, numbers, pos, cell, None, species=mdl.species)["cv"]
    return cv0 + sigma * np.random.default_rng(17).normal(size=(n, len(cv0)))


@pytest.mark.parametrize("pre", [0, 13], ids=["empty", "preloaded13"])
@pytest.mark.parametrize("how,tem", [("langevin", None), ("langevin", 900.0), ("nose-hoover", 900.0)])
def test_trajectory_with_merging_inside_the_loop_against_the_twin(models, how, tem, pre):
    from autoforce_amd.workloads import FS
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36", SOFT)
    N = len(numbers)
    cvs, sigma, w = D4(numbers), 0.05, 0.3
    vel = _vel(numbers)
    xi = np.random.default_rng(9).normal(size=(STEPS + 1, N, 3)) if how == "langevin" else np.zeros((STEPS + 1, N, 3))
    hills0 = _pre(mdl, numbers, pos, cell, cvs, sigma, pre) if pre else None
    meta = _twin_meta(mdl, numbers, sigma, w, tem)
    meta.merge = CH
    if pre:
        meta.hills = [h.copy() for h in hills0]
    host, margin = _twin(mdl, numbers, pos, cell, pbc, vel, how, meta, xi=xi)
    assert margin > MARGIN, margin
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05 if how == "langevin" else 0.0, ttime=20.0 * FS if how == "nose-hoover" else None)
    mdl.md_meta(cvs, sigma, w, tem=tem, hills=hills0, capacity=pre + STEPS + 2, merge=CH)
    assert mdl.md_meta_table()[2] == (pre // CH) * CH      # the uploaded chunks are merged at the attach
    sc, code = mdl.md_run(STEPS + 1, xi if how == "langevin" else None, final=True)
    assert code == 0 and len(sc) == STEPS + 1
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    cvd, Vd = mdl.md_meta_hills()
    info = mdl.md_meta_info()
    print(f"meta merged trajectory {how} tem={tem} pre={pre}: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e} max V {Vd[pre:].max():.3e}")
    assert len(cvd) == pre + STEPS + 1 and Vd[pre:].max() > 1e-3 and info["below"] == pre + STEPS
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL, (dx, dv)
    assert dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max())
    # the table at the end is the twin's, from the twin's own hills; eight chunks were merged inside the loop
    T, cmax = _table_equals(mdl, np.array(meta.hills)[:info["below"]], sigma, CH, 4)
    rows = mdl.md_meta_table()[2]
    assert rows == ((pre + STEPS) // CH) * CH and rows // CH - pre // CH == 8
    assert cmax > 1 and mdl.md_meta_info() == info and sorted(info) == ["D", "below", "capacity", "held"]


def _merged_run(mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta, cuts=None, ediff=0.0, reattach=None, known=None, **begin):
    """test_hip_meta_device._cut_run for a merged run, with the places of the halts and the table returned too; reattach = n: behind the
    first call that has passed configuration n the bias is attached again from md_meta_hills (the restart path), merge included;
    known: the hill rows of the same run — at every halt the table the caller sees is the twin's table of the rows below the halted
    configuration (in front of a crossing the device holds one chunk more by then)."""
    from autoforce_amd.workloads import meta_table
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05, **begin)
    mdl.md_meta(cvs, capacity=STEPS + 2, **meta)
    done, halts, rows, total, again = 0, [], [], STEPS + 1, False
    while done < total:
        n = 1 if again else min(cuts or total, total - done)
        sc, code = mdl.md_run(n, xi[done:done + n], ediff=0.0 if again else ediff, final=(done + n == total))
        assert code in (0, 1)
        acc = len(sc) - 1 if code == 1 else len(sc)
        rows.extend(sc[:acc])
        done += acc
        again = code == 1
        if code == 1:
            halts.append(done)
            if known is not None:
                tc, _, cnt, B = meta_table(known[:done], np.full(known.shape[1], meta["sigma"]), meta["merge"])
                got = mdl.md_meta_table()
                assert got[2] == B and np.array_equal(got[0], tc) and np.array_equal(got[1], cnt), (done, got[2], B)
        if reattach is not None and done >= reattach and done < total:
            below = mdl.md_meta_info()["below"]
            table = mdl.md_meta_table()
            mdl.md_meta(cvs, capacity=STEPS + 2, hills=mdl.md_meta_hills(0, below), **meta)
            again_table = mdl.md_meta_table()                 # merged at the attach through the same kernel: the table the loop had built
            assert all(np.array_equal(a, b) for a, b in zip(table, again_table)) and table[2] == (below // meta["merge"]) * meta["merge"]
            reattach = None
    st = mdl.md_state(results=True)
    return dict(rows=np.array(rows)[:, :12], x=st["positions"], v=st["velocities"], hills=mdl.md_meta_hills(), table=mdl.md_meta_table(), halts=halts)


def _same(a, b):
    return (np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["x"], b["x"]) and np.array_equal(a["v"], b["v"])
            and np.array_equal(a["hills"][0], b["hills"][0]) and np.array_equal(a["hills"][1], b["hills"][1])
            and a["table"][2] == b["table"][2] and np.array_equal(a["table"][0], b["table"][0]) and np.array_equal(a["table"][1], b["table"][1]))


def test_cuts_halts_and_a_restart_leave_the_same_bits(models):
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36", SOFT)
    N = len(numbers)
    cvs, meta = D4(numbers), dict(sigma=0.05, w=0.3, tem=900.0, merge=CH)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    args = (mdl, numbers, pos, cell, pbc, vel, xi, cvs, meta)
    one = _merged_run(*args)
    cov = one["rows"][:, 11]
    # the gate of the existing cut test — the three largest covlosses reach it —, lowered where needed so that a halt falls on a
    # chunk crossing (configuration 8 k: its own launch merges a chunk) and on a configuration in front of one (8 k - 1: the
    # speculative step behind it merges a chunk the halted configuration must not see when it is evaluated again)
    gate = float(min(np.sort(cov)[-3], cov[8:STEPS:8].max(), cov[7:STEPS:8].max()))
    runs = [_merged_run(*args, cuts=7), _merged_run(*args, ediff=gate, known=one["hills"][0]), _merged_run(*args), _merged_run(*args, cuts=7, ediff=gate),
            _merged_run(*args, reattach=30, cuts=19), _merged_run(*args, reattach=13, ediff=gate)]
    assert not one["halts"] and len(runs[1]["halts"]) >= 2
    for r in (runs[1], runs[5]):
        assert any(k % 8 == 0 for k in r["halts"]) and any(k % 8 == 7 for k in r["halts"]), r["halts"]
    for r in runs:
        assert _same(r, one), r["halts"]
    assert one["table"][2] == STEPS and one["table"][1].sum() == STEPS and len(one["hills"][0]) == STEPS + 1 and one["hills"][1].max() > 1e-3


def test_held_components_the_filter_and_the_record_together_with_merging(models):
    import autoforce_amd.workloads as wl
    mdl, numbers, pos, cell, pbc = models("g5_bigtric36")
    N = len(numbers)
    cvs, sigma, w = D4(numbers), 0.05, 0.3
    fx = np.zeros((N, 3), bool)
    fx[1] = True
    fx[N - 1, 2] = True
    f0 = 0.4 * np.random.default_rng(21).normal(size=(N, 3))
    kw = dict(fixed=fx, ml_filter=0.8, filter_init=(f0, None))
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(STEPS + 1, N, 3))
    meta = _twin_meta(mdl, numbers, sigma, w, None)
    meta.merge = CH
    host, margin = _twin(mdl, numbers, pos, cell, pbc, vel, "langevin", meta, xi=xi, **kw)
    assert margin > MARGIN
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05, **kw)
    mdl.md_meta(cvs, sigma, w, capacity=STEPS + 2, merge=CH)
    mdl.md_record(8, velocities=True, results=True)
    sc, code = mdl.md_run(STEPS + 1, xi, final=True)
    assert code == 0
    st = mdl.md_state(results=True)
    dx = np.abs(st["positions"] - host[-1][1]).max() / np.abs(host[-1][1]).max()
    dv = np.abs(st["velocities"] - host[-1][2]).max() / np.abs(host[-1][2]).max()
    dE = np.abs(sc[:, 0] - np.array([h[0] for h in host])).max()
    print(f"meta merged composed: margin {margin:.2e} dx {dx:.2e} dv {dv:.2e} dE {dE:.2e}")
    assert dx <= TRAJ_RTOL and dv <= TRAJ_RTOL and dE <= TRAJ_RTOL * max(1.0, np.abs(sc[:, 0]).max())
    assert np.array_equal(st["positions"][fx], pos[fx]) and not st["velocities"][fx].any()
    hills = mdl.md_meta_hills(0, STEPS + 1)[0]

    def biased(x, n):
        return mdl.predict(numbers, x, cell, pbc), wl.meta_bias(cvs, sigma, w, numbers, x, cell, hills[:n], species=mdl.species, merge=CH)
    plain, want = biased(st["positions"], STEPS)
    fb, fm = np.abs(want["forces"]).max(), np.abs(plain["forces"]).max()
    assert fb > 1e-3 and np.abs(st["forces"] - plain["forces"] - want["forces"]).max() <= 1e-12 * max(fb, fm)
    fr = mdl.md_frames()
    assert list(fr["index"]) == list(range(0, STEPS + 1, 8)) and np.array_equal(fr["energy"], sc[fr["index"], 0])
    np.testing.assert_allclose(fr["energy"], [host[i][0] for i in fr["index"]], rtol=TRAJ_RTOL, atol=TRAJ_RTOL)
    for k in (4, 8):
        n = int(fr["index"][k])
        plain, want = biased(fr["positions"][k], n)
        assert np.abs(fr["forces"][k] - plain["forces"] - want["forces"]).max() <= 1e-12 * max(fb, fm)
        assert abs(fr["energy"][k] - plain["energy"] - want["energy"]) <= 1e-12 * max(1.0, abs(plain["energy"]))
    _table_equals(mdl, hills[:STEPS], sigma, CH, 4)


def test_unmerged_runs_keep_their_bits_and_the_surface_refuses_what_it_must(models):
    from autoforce_amd import SgprError, _lib
    mdl, numbers, pos, cell, pbc = models("g5_si32")
    N = len(numbers)
    lib = _lib.load()
    cvs, meta = [("distance", 0, 5), ("posvar", 2, None)], dict(sigma=0.02, w=2.0)
    vel, xi = _vel(numbers), np.random.default_rng(9).normal(size=(24, N, 3))

    def run(attach):
        _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05)
        attach()
        sc, code = mdl.md_run(24, xi, final=True)
        st = mdl.md_state(results=True)
        return sc[:, :12], st["positions"], st["velocities"], mdl.md_meta_hills()

    def same(a, b):
        return all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])
    base = run(lambda: mdl.md_meta(cvs, capacity=32, **meta))
    none = run(lambda: mdl.md_meta(cvs, capacity=32, merge=None, **meta))
    assert same(base, none)

    def off_again():
        mdl.md_meta(cvs, capacity=32, merge=4, **meta)
        _lib.check(lib.sgpr_md_meta_merge(mdl.handle, 0))
    assert same(base, run(off_again))
    with pytest.raises(SgprError):
        mdl.md_meta_table()                                 # (no table without merging)
    merged = run(lambda: mdl.md_meta(cvs, capacity=32, merge=4, **meta))
    assert mdl.md_meta_info() == dict(D=4, below=23, held=24, capacity=32) and mdl.md_meta_table()[2] == 20
    assert np.allclose(merged[1], base[1], rtol=0, atol=1e-9)   # (the same terms in another order: the same run to rounding, not promised bit for bit)
    # after the first md_run since the attach, before sgpr_md_meta, and a negative chunk: SGPR_E_INVALID
    assert lib.sgpr_md_meta_merge(mdl.handle, 4) == -1
    _begin(mdl, numbers, pos, cell, pbc, vel, friction=0.05)
    assert lib.sgpr_md_meta_merge(mdl.handle, 4) == -1
    mdl.md_meta(cvs, capacity=32, **meta)
    assert lib.sgpr_md_meta_merge(mdl.handle, -1) == -1
    assert lib.sgpr_md_meta_merge(mdl.handle, 4) == 0 and lib.sgpr_md_meta_merge(mdl.handle, 0) == 0
    with pytest.raises(ValueError):
        mdl.md_meta(cvs, capacity=32, merge=0, **meta)
