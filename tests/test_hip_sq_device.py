"""GPU tests of the structure-factor accumulator of the device MD loop (sgpr_md_sq / sgpr_md_sq_read; md_sq_part_kernel in both
forms, md_sq_fold_kernel and md_sq_done_kernel behind a sampled evaluation) against its host twin and definition workloads.SqRing.
The device's sincospi is not numpy's sin and cos, so the two are held to the a-priori bound of md_sq.inc, restated here,
    |d rho_z(q)| <= B_z = 128 hmax (1 + smax) n_z 2^-52,   |d f[k, j, a, b]| <= count[k] (n_a B_b + n_b B_a + count[k] n_a n_b 2^-52)
(the sum of rho over the samples: samples B_z), integers exactly, and two device runs bit for bit.  The twin is fed the positions
of the SAME run's frame record at every = 1.  One call and a cut run, other settings and sets of wave vectors, held atoms,
Nose-Hoover, device deviates, frames whose species segments end off a chunk and off a wave, a covloss halt in the middle with and
without a model update, runs beside the record, the filter, a bias and the other five accumulators, every refusal in both
directions, and ActiveCalculator.run_md(sq=) on the device against the host loop.  Frame, model, run loop and the bodies the six
accumulators share: accumulator_device.py."""
import numpy as np
import pytest

import accumulator_device as A
from accumulator_device import EVALS, T, _begin, _frame, _shared

pytestmark = pytest.mark.gpu

KEYS = ("f", "mean", "count")
WORST = dict(f=0.0, mean=0.0)   # the largest deviation over bound this module has seen (printed by every comparison)


def _hkl(kind="mixed", cell=None):
    """Sets of wave vectors: "mixed" — the first shells of the half-sphere, triples with negative indices and with a zero in
    each axis, and indices up to 16 (the wide form's last power); "narrow": the same with indices up to 32; an integer: that many
    vectors of the half-sphere."""
    from autoforce_amd.transport import q_vectors
    cell = _frame()[2] if cell is None else cell
    if isinstance(kind, int):
        qmax = 0.9
        while True:
            hkl = q_vectors(cell, qmax)
            if len(hkl) >= kind:
                return hkl[:kind]
            qmax *= 1.3
    top = 16 if kind == "mixed" else 32
    own = [(-1, 2, 0), (0, 1, -3), (-5, 0, 7), (0, 0, 2), (0, 3, 0), (4, 0, 0), (top, 0, 0), (0, -top, 0), (0, 0, top), (-top, top, -top),
           (top - 1, -3, 5), (1, 1, 1), (-2, -3, -4)]
    return np.concatenate([q_vectors(cell, 1.2), np.array(own)])


def _run(fr, sq, beside=None, **kw):
    """accumulator_device.run with the accumulator `sq` = (every, hkl, lags, origin_every) or None; beside(mdl) attaches what runs
    beside it, ahead of it, and returns a reader of its tables.  Returns (table or None, recorded positions or None, scalar rows,
    final state, what the reader read)."""
    reader = []

    def attach(mdl):
        if beside is not None:
            reader.append(beside(mdl))
        if sq is not None:
            mdl.md_sq(*sq)

    def read(mdl):
        return (None if sq is None else mdl.md_sq_table()), (reader[0]() if reader else None)
    (tab, other), xs, rows, state = A.run(fr, attach, read, label=f"sq {None if sq is None else (sq[0], len(sq[1])) + tuple(sq[2:])}", **kw)
    return tab, xs, rows, state, other


def _twin(fr, sq, xs):
    from autoforce_amd.workloads import SqRing
    tw = SqRing(sq[0], sq[1], sq[2], sq[3], fr[0], _shared()[0].species, fr[2], fr[3])
    for x in xs:
        tw.add(x)
    return tw.table(), tw.smax


def _bounds(hmax, smax, nz, count):
    n, c = np.asarray(nz, float), np.asarray(count, float)[:, None, None]
    B = 128.0 * hmax * (1.0 + smax) * n * 2.0 ** -52
    return B, c * (n[:, None] * B[None, :] + n[None, :] * B[:, None] + c * n[:, None] * n[None, :] * 2.0 ** -52)


def _within(tab, want, smax, what=""):
    """The device's table against the twin's: integers and settings exactly, f and mean within the bound."""
    hmax = int(np.abs(want["hkl"]).max())
    B, F = _bounds(hmax, smax, want["n"], want["count"])
    df = np.abs(tab["f"] - want["f"]).max(axis=1)
    dm = np.abs(tab["mean"] - want["mean"]).max(axis=0)
    rf = float(np.max(df[F > 0] / F[F > 0])) if np.any(F > 0) else 0.0
    rm = float(np.max(dm[B > 0] / (want["samples"] * B[B > 0]))) if want["samples"] else 0.0
    WORST["f"], WORST["mean"] = max(WORST["f"], rf), max(WORST["mean"], rm)
    print(f"{what}: count {list(tab['count'][:6])} samples {tab['samples']} next_due {tab['next_due']} hmax {hmax} smax {smax:.3f}: "
          f"max |df| {df.max():.3e} = {rf:.3e} of its bound, max |dmean| {dm.max():.3e} = {rm:.3e} of its bound (module's worst {WORST})")
    for k in ("count", "lags", "hkl", "species", "n"):
        assert np.array_equal(tab[k], want[k]), (what, k)
    assert tab["samples"] == want["samples"] and tab["next_due"] == want["next_due"], (what, tab["samples"], tab["next_due"])
    assert np.allclose(tab["q"], want["q"], rtol=1e-12, atol=0)
    assert np.all(df <= F), (what, df, F)
    assert np.all(dm <= want["samples"] * B), (what, dm, want["samples"] * B)


def _bits(a, b, what=""):
    for k in KEYS + ("lags", "hkl", "species", "n"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["samples"] == b["samples"] and a["next_due"] == b["next_due"], what


def test_one_call_and_a_cut_run_have_the_same_bits_and_lie_within_the_bound_of_the_twin():
    fr = _frame()
    sq = (1, _hkl(), 8, 1)
    tab, xs, rows, _, _ = _run(fr, sq)
    want, smax = _twin(fr, sq, xs)
    assert list(want["count"]) == [40, 39, 38, 37, 36, 35, 34, 33] and want["samples"] == 40 and want["next_due"] == 40
    assert np.abs(want["f"][0][:, [0, 1, 2], [0, 1, 2]]).min() > 0.0 and tab["f"].shape == (8, len(sq[1]), 3, 3)
    _within(tab, want, smax, "one call")
    tab2, xs2, rows2, _, _ = _run(fr, sq, cuts=(7, 1, 12, 20))
    assert np.array_equal(xs2, xs) and np.array_equal(rows2, rows)
    _bits(tab2, tab, "cut 7 + 1 + 12 + 20")
    _within(tab2, want, smax, "cut 7 + 1 + 12 + 20")


VARIANTS = dict(every3=dict(sq=(3, "mixed", 5, 1)), origin3=dict(sq=(1, "mixed", 7, 3)), lags1=dict(sq=(1, "mixed", 1, 1)),
                lags13=dict(sq=(1, "mixed", 13, 1)), lags64=dict(sq=(1, "mixed", 64, 1)), nq1=dict(sq=(1, 1, 4, 1)),
                nq257=dict(sq=(1, 257, 3, 1)), narrow=dict(sq=(1, "narrow", 4, 2)), held=dict(sq=(1, "mixed", 4, 1)),
                nose_hoover=dict(sq=(2, "mixed", 4, 1), nh=True), deviates=dict(sq=(1, "mixed", 4, 1), seed=41))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_lie_within_the_bound_of_the_twin(variant):
    from fixed_common import mask
    fr = _frame()
    v = dict(VARIANTS[variant])
    every, kind, lags, origin_every = v.pop("sq")
    sq = (every, _hkl(kind), lags, origin_every)
    if variant == "held":
        v["fixed"] = mask(len(fr[0]))
    tab, xs, _, _, _ = _run(fr, sq, **v)
    want, smax = _twin(fr, sq, xs)
    samples = -(-EVALS // every)
    assert want["samples"] == samples and list(want["count"]) == [
        sum(1 for s in range(samples) if s >= k and (s - k) % origin_every == 0) for k in range(lags)]
    if variant == "lags64":
        assert np.all(want["count"][40:] == 0) and np.all(tab["f"][40:] == 0.0)
    if kind in ("mixed", "narrow"):   # (negative indices, a zero in each axis, the form's last power)
        assert np.any(sq[1] < 0) and all(np.any(sq[1][:, a] == 0) for a in range(3)) and np.abs(sq[1]).max() == (16 if kind == "mixed" else 32)
    if variant == "nq257":
        assert len(sq[1]) == 257
    _within(tab, want, smax, variant)


def _off_grid(kind):
    """accumulator_device's "sub200" and "chunks", and "absent": sub200 without the atoms of its smallest species."""
    if kind != "absent":
        return _frame(kind)
    numbers, pos, cell, pbc, mass, vel = _frame("sub200")
    zs, cnt = np.unique(numbers, return_counts=True)
    keep = numbers != zs[np.argmin(cnt)]
    return numbers[keep], pos[keep], cell, pbc, mass[keep], vel[keep]


@pytest.mark.parametrize("form", ["mixed", "narrow"])
@pytest.mark.parametrize("kind", ["sub200", "chunks", "absent"])
def test_segments_off_a_chunk_and_a_species_without_atoms(kind, form):
    fr = _off_grid(kind)
    width = 64 if form == "mixed" else 32
    n = np.array([int(np.sum(fr[0] == z)) for z in _shared()[0].species])
    if kind == "sub200":
        assert 0 < n.min() < width and np.all(n % width != 0) and np.all(np.cumsum(n) % width != 0) and np.all(np.cumsum(n) % 64 != 0)
    elif kind == "chunks":
        assert n.max() > 4 * width and np.any(n % width != 0)
    else:
        assert n.min() == 0 and np.sum(n > 0) == 2
    sq = (1, _hkl(form, fr[2]), 5, 2)
    tab, xs, _, _, _ = _run(fr, sq, cuts=(5, 11))
    want, smax = _twin(fr, sq, xs)
    assert np.array_equal(want["n"], n)
    _within(tab, want, smax, f"{kind}, {form}")
    if kind == "absent":
        z = int(np.argmin(n))
        assert np.all(tab["f"][:, :, z, :] == 0.0) and np.all(tab["f"][:, :, :, z] == 0.0) and np.all(tab["mean"][:, z] == 0.0)


def test_a_covloss_halt_counts_the_configuration_once():
    """The gate fires at evaluation k inside a call: k has been sampled at its first evaluation (positions do not depend on the
    model), the speculative evaluation k + 1 behind it stays out, and the repeat of k — with the model unchanged or updated
    between the calls — counts nothing: the table is the one of the positions that stand."""
    fr, evals = _frame(), 24
    sq = (1, _hkl(), 6, 1)
    want, xs, rows, _, _ = _run(fr, sq, cuts=(evals,), seed=77)
    k, ediff = A.first_halt(rows, evals)
    mdl = _shared()[0]
    mu0, vs0 = np.array(mdl.mu, float), dict(mdl._vscale)   # (the update changes the weights alone and puts them back)
    for update in (False, True):
        _begin(mdl, fr, seed=77)
        mdl.md_record(1, velocities=False, results=False)
        mdl.md_sq(*sq)
        got = []
        try:
            sc, code = mdl.md_run(evals, None, ediff=ediff)
            assert code == 1 and len(sc) == k + 1, (code, len(sc), k)
            got.append(mdl.md_frames(closed=False)["positions"].copy())
            mid = mdl.md_sq_table()
            assert (mid["next_due"], mid["samples"], mid["count"][0], mid["count"][1]) == (k + 1, k + 1, k + 1, k)
            if update:
                mdl.set_weights(1.5 * mu0, choli=mdl.choli, vscale=vs0)
            sc1, code = mdl.md_run(1, None, ediff=0.0)
            assert code == 0 and len(sc1) == 1
            got.append(mdl.md_frames(closed=False)["positions"].copy())
            _bits(mdl.md_sq_table(), mid, "the repeat counts nothing")
            sc2, code = mdl.md_run(evals - k - 1, None, ediff=0.0)
            assert code == 0
            got.append(mdl.md_frames(closed=False)["positions"].copy())
            tab = mdl.md_sq_table()
            pos = np.concatenate(got)
            assert len(pos) == evals and np.array_equal(pos[:k + 1], xs[:k + 1])
            twin, smax = _twin(fr, sq, pos)
            _within(tab, twin, smax, f"halt at {k}, the model {'updated' if update else 'unchanged'}")
            if update:
                assert not np.array_equal(pos[k + 1:], xs[k + 1:]) and not np.array_equal(tab["f"], want["f"])
            else:
                assert np.array_equal(np.concatenate([sc[:k], sc1, sc2]), rows)
                _bits(tab, want, "the run that never halted")
        finally:
            if update:
                mdl.set_weights(mu0, choli=mdl.choli, vscale=vs0)
    _, _, rows_after, _, _ = _run(fr, None, cuts=(evals,), seed=77, record=False)   # (the module's model is the one it was)
    assert np.array_equal(rows_after, rows)


def _same_tables(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], dict):
            _same_tables(a[k], b[k], f"{what}.{k}")
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


BESIDE = dict(
    record=dict(record=True),
    ml_filter=dict(kw=dict(ml_filter=0.5), attach=lambda m: (lambda: dict(filter=dict(zip("fs", m.md_filter_state()))))),
    md_meta=dict(attach=lambda m: (m.md_meta([("distance", 0, 5)], 0.02, 0.5, capacity=64), lambda: dict(hills=dict(zip(("cv", "V"), m.md_meta_hills()))))[1]),
    md_msd=dict(attach=lambda m: (m.md_msd(2, 3, True), m.md_msd_table)[1]),
    md_rdf=dict(attach=lambda m: (m.md_rdf(4, 6.0, 60, 0.0), m.md_rdf_table)[1]),
    md_vacf=dict(attach=lambda m: (m.md_vacf(1, 5, 2, True), m.md_vacf_table)[1]),
    md_vanhove=dict(attach=lambda m: (m.md_vanhove(2, 3, 3.0, 30, 2, 2, 6.0, 20), m.md_vanhove_table)[1]),
    md_adf=dict(attach=lambda m: (m.md_adf(3, 36, 3.0), m.md_adf_table)[1]))


@pytest.mark.parametrize("other", list(BESIDE))
def test_beside_the_record_the_filter_a_bias_and_the_other_accumulators_nobody_notices(other):
    """With and without md_sq the other's tables, the scalar rows and the final state have the same bits; with and without the
    other md_sq's own table has the same bits."""
    fr, b = _frame(), BESIDE[other]
    sq = (2, _hkl(), 4, 1)
    moves = other in ("ml_filter", "md_meta")   # (a filter and a bias are other integrators: the record tells where the atoms went)
    kw = dict(cuts=(9, 11), seed=5, record=b.get("record", moves), **b.get("kw", {}))
    both, xs, rows, st, o = _run(fr, sq, beside=b.get("attach"), **kw)
    _, xs_o, rows_o, st_o, oo = _run(fr, None, beside=b.get("attach"), **kw)
    assert both["samples"] == 10 and both["next_due"] == 20
    assert np.array_equal(rows, rows_o)
    for key in ("positions", "velocities_pre"):
        assert np.array_equal(st[key], st_o[key]), key
    if o is not None:
        _same_tables(o, oo, other)
    if xs is not None:
        assert np.array_equal(xs, xs_o)
    if moves:
        want, smax = _twin(fr, sq, xs)
        _within(both, want, smax, f"beside {other}")
        again, _, _, _, _ = _run(fr, sq, beside=b.get("attach"), **kw)
        _bits(again, both, f"beside {other}, again")
    else:
        alone, _, rows_a, _, _ = _run(fr, sq, cuts=(9, 11), seed=5, record=False)
        assert np.array_equal(rows, rows_a)
        _bits(both, alone, f"beside {other}")


def test_a_detach_frees_and_a_fresh_attach_starts_from_zeros():
    from test_hip_teardown import _live
    mdl, fr = _shared()[0], _frame()
    sq = (1, _hkl(), 6, 1)
    _begin(mdl, fr, seed=7)
    mdl.md_sq(0)
    plain = _live()
    mdl.md_sq(*sq)
    held = _live()
    assert held[0] > plain[0] and held[1] > plain[1]
    mdl.md_sq(0)
    assert np.array_equal(_live(), plain)
    with pytest.raises(RuntimeError, match="no accumulator"):
        mdl.md_sq_table()
    mdl.md_sq(*sq)
    assert np.array_equal(_live(), held)
    zero = mdl.md_sq_table()
    assert zero["samples"] == 0 and zero["next_due"] == 0 and not np.any(zero["count"]) and not np.any(zero["f"]) and not np.any(zero["mean"])
    sc, code = mdl.md_run(6, None)
    assert code == 0 and mdl.md_sq_table()["count"][0] == 6
    mdl.md_sq(0)
    _begin(mdl, fr, seed=7)
    mdl.md_record(1, velocities=False, results=False)
    mdl.md_sq(*sq)
    sc, code = mdl.md_run(10, None)
    assert code == 0
    want, smax = _twin(fr, sq, mdl.md_frames()["positions"])
    _within(mdl.md_sq_table(), want, smax, "a fresh attach behind a detach")
    mdl.md_end()


GOOD = np.ascontiguousarray([[1, 0, 0], [0, -2, 3]], dtype=np.int32)


def _raw(h, every=1, hkl=GOOD, lags=4, origin_every=1, nq=None):
    from autoforce_amd._lib import ptr
    return A.lib().sgpr_md_sq(h, every, len(hkl) if nq is None else nq, None if hkl is None else ptr(np.ascontiguousarray(hkl, dtype=np.int32)),
                              lags, origin_every)


def _limits(c):
    """A wave vector with a component along a direction that is not periodic; a table over the byte limit."""
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    numbers, pos, cell, pbc, mass, vel = c.fr
    c.mdl.md_begin(numbers, pos, cell, (True, True, False), mass, vel, dt=1.0 * FS, kT=kB * T, friction=0.05)
    assert c.raw(hkl=[[1, 0, 1]]) == c.INV
    c.words(b"not periodic")
    assert c.raw(hkl=[[1, -1, 0]]) == 0
    _begin(c.mdl, c.fr, seed=77)
    assert c.raw(hkl=np.ones((8192, 3), dtype=np.int32), lags=8192) == c.UNS
    c.words(b"at most 1073741824")


ACC = A.Acc(name="sq", noun=b"structure factors", moving_cell=b"the wave vectors are the reciprocal lattice of a constant cell", polymer=b"beads are",
            raw=_raw, detach=lambda h: A.lib().sgpr_md_sq(h, 0, 0, None, 0, 0), read=lambda h: A.lib().sgpr_md_sq_read(h, None, None, None, None),
            py=lambda mdl: mdl.md_sq(1, GOOD), limits=_limits,
            invalid=[dict(every=-1), dict(nq=0), dict(hkl=np.ones((8193, 3), dtype=np.int32)), dict(hkl=None, nq=2), dict(hkl=[[1, 0, 0], [0, 0, 0]]),
                     dict(hkl=[[33, 0, 0]]), dict(hkl=[[0, -33, 1]]), dict(lags=0), dict(lags=8193), dict(origin_every=0)],
            port=29920)


def test_refusals_in_both_directions_leave_the_handle_working():
    A.refusals(ACC)


def test_a_run_begun_on_two_ranks_refuses_the_accumulator_and_goes_on_working():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("two ranks need two devices")
    A.two_rank_refusal(ACC)


def test_run_md_fills_tables_on_the_device_and_through_the_host_loop_that_agree_within_the_bound(tmp_path):
    """accumulator_device.run_md_host_and_device with run_md(sq=holder), the host loop's SqRing fed every step's positions: the
    same integers and tables within the bound."""
    from autoforce_amd.transport import Sq, intermediate_scattering, q_vectors, structure_factor
    smax = [0.0]

    def seen(mode, o, at, cell, holder):
        if mode == "host" and o[0] % holder.every == 0:   # (the host loop sets atoms.positions before every yield: the sample the twin was fed)
            smax[0] = max(smax[0], float(np.abs(np.asarray(at.positions) @ np.linalg.inv(np.asarray(cell, float).reshape(3, 3))).max()))
    tabs, holder, numbers = A.run_md_host_and_device(tmp_path, "sq", lambda cell: Sq(2, q_vectors(cell, 2.0), lags=5, origin_every=2), seen)
    print(f"counts {list(tabs[0]['count'])}, nq {len(tabs[0]['hkl'])}")
    assert list(tabs[0]["count"]) == [11, 10, 10, 9, 9] and tabs[0]["samples"] == 21
    _within(tabs[1], tabs[0], smax[0], "run_md on the device against the host loop")
    q, S = structure_factor(holder)
    present = np.flatnonzero(np.asarray(holder.n) > 0)
    assert np.all(np.isfinite(S[:, present][:, :, present])) and np.all(S[:, present, present] > 0.0)
    assert np.all(np.isfinite(intermediate_scattering(holder)[2][:, :, present][:, :, :, present]))
