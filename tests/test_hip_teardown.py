"""GPU tests of ownership and teardown: every device buffer of a handle is a DevBuf that frees itself, sgpr_destroy names
none of them, and sgpr_live_device_memory counts what is alive.  Every test works with DIFFERENCES of
autoforce_amd.live_device_memory(), taken before its first handle is created (other modules' fixtures may hold handles in
this process): after close() the difference in bytes and in buffers is exactly (0, 0) — for every run mode that allocates
buffers of its own, for the paths that hand a buffer from one owner to another, and for a handle destroyed in the middle
of a run.  Frame and model are test_hip_npt_device._model()'s (512-atom lips(8), 48 inducing points)."""
import gc

import numpy as np
import pytest

from test_hip_npt_device import _begin as _begin_npt, _model, _setup

pytestmark = pytest.mark.gpu

T = 600.0


def _live():
    """(bytes, buffers) now.  Handles that earlier tests dropped without close() are destroyed first, so that none of them
    goes away between two readings."""
    from autoforce_amd import live_device_memory
    gc.collect()
    return np.array(live_device_memory(), dtype=np.int64)


def _begin(mdl, numbers, pos, cell, pbc, mass, vel, friction=0.0, **kw):
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    mdl.md_begin(numbers, pos, cell, pbc, mass, vel, dt=1.0 * FS, friction=friction, kT=kB * T, **kw)


def _run(mdl, n=4, final=True):
    sc, code = mdl.md_run(n, None, final=final)
    assert code == 0 and len(sc) == n and np.all(np.isfinite(sc))
    return sc


# ---------------------------------------------------------------------------------------------- every feature gives everything back
def _predict(mdl, s):
    assert np.isfinite(mdl.predict(s[1], s[2], s[3], s[4])["energy"])


def _langevin(mdl, s):
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    _run(mdl)


def _nose_hoover(mdl, s):
    from autoforce_amd.workloads import FS
    _begin(mdl, *s[1:7], ttime=25.0 * FS)
    _run(mdl)


def _barostat(mdl, s):
    _begin_npt(mdl, *s[1:8])
    _run(mdl)
    assert len(mdl.md_cells()[0]) == 4


def _relax(mdl, s, **kw):
    mdl.relax_begin(s[1], s[2], s[3], s[4], 1e-9, **kw)
    _run(mdl, final=False)


def _relax_cell(mdl, s):
    _relax(mdl, s, cell_relax=True)


def _filter(mdl, s):
    _begin(mdl, *s[1:7], ml_filter=0.8)
    _run(mdl, 3, final=False)
    mdl.md_filter_push(0.1 * np.random.default_rng(5).normal(size=s[2].shape), None)
    _run(mdl, 2)


def _fixed(mdl, s):
    _begin(mdl, *s[1:7], fixed=np.arange(len(s[1])) % 7 == 0)
    _run(mdl)


def _record(mdl, s):
    _begin(mdl, *s[1:7])
    mdl.md_record(2, velocities=True, results=True)
    _run(mdl, 6)
    assert len(mdl.md_frames()["index"]) == 3


def _meta(mdl, s):
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    mdl.md_meta([("distance", 0, 5)], 0.1, 0.1, capacity=64, merge=4)
    _run(mdl, 10)
    rows = mdl.md_meta_table()[2]
    assert rows == (mdl.md_meta_info()["below"] // 4) * 4 > 0     # whole chunks of four rows were merged inside the loop


def _committee(mdl, s):
    member, _ = _model(seed=2)
    _begin(mdl, *s[1:7])
    mdl.md_committee([member])
    _run(mdl)
    mdl.md_end()
    member.close()


def _neb(mdl, s):
    from test_hip_neb_device import _band
    mdl.neb_begin(s[1], _band(s[2], 3), s[3], s[4], 0.05)
    _run(mdl, 3, final=False)


def _pimd(mdl, s):
    from test_hip_pimd_device import _begin as _begin_pimd, _polymer
    numbers, beads, vel, mass = _polymer(s[1], s[2], 3)
    _begin_pimd(mdl, numbers, beads, vel, mass, s[3], s[4], seed=7)
    _run(mdl, 3, final=False)


def _data(mdl, s):
    """The resident matrix and the kept first-stage factorisation: a refit, an appended and a popped column (QrKeep::ops), a
    frame pushed on top of a kept factor and popped again (r1_cache), a re-solve."""
    from autoforce_amd.workloads import inducing_from_frame, lips
    extra = inducing_from_frame(mdl, *lips(8, seed=3), 50, seed=9)[:2]
    for f in range(2):
        mdl.data_push(*lips(8, seed=100 + f))
    rng = np.random.default_rng(4)
    Y = rng.normal(size=mdl.data_info()[1])
    mdl.data_solve(Y)
    assert mdl.solve_info().startswith("stage1=full factorisation;")
    mdl.add_inducing(extra[0])
    mdl.data_solve(Y)
    assert "through the kept reflectors" in mdl.solve_info()
    mdl.remove_inducing(-1)
    mdl.data_solve(Y)
    mdl.data_push(*lips(8, seed=102))
    mdl.data_solve(np.concatenate([Y, rng.normal(size=mdl.data_info()[1] - len(Y))]))
    mdl.data_pop(-1)
    mdl.data_solve(Y)
    assert np.all(np.isfinite(mdl.resolve(0.02)))


def _inducing(mdl, s):
    """The design-matrix pair: a selection gathers into the second buffer and swaps."""
    from autoforce_amd.workloads import inducing_from_frame, lips
    extra = inducing_from_frame(mdl, *lips(8, seed=3), 50, seed=9)[:2]
    mdl.data_push(*lips(8, seed=100))
    for x in extra:
        mdl.add_inducing(x)
    mdl.remove_inducing(0)
    mdl.select_inducing(list(range(0, mdl.m, 2))[::-1])
    mdl.select_inducing(list(range(mdl.m))[::-1])
    assert mdl.data_get().shape == (mdl.data_info()[1], mdl.m)


FEATURES = dict(predict=_predict, langevin=_langevin, nose_hoover=_nose_hoover, barostat=_barostat, relax=_relax, relax_cell=_relax_cell,
                ml_filter=_filter, fixed=_fixed, record=_record, meta_merge=_meta, committee=_committee, neb=_neb, pimd=_pimd, data=_data,
                inducing=_inducing)


@pytest.mark.parametrize("feature", list(FEATURES))
def test_every_feature_gives_everything_back(feature):
    before = _live()
    s = _setup()
    mdl = s[0]
    FEATURES[feature](mdl, s)
    held = _live() - before
    mdl.close()
    after = _live() - before
    print(f"{feature}: held {held[0]} bytes in {held[1]} buffers; after close {tuple(after)}")
    assert held[0] > 0 and held[1] > 0
    assert tuple(after) == (0, 0)


# ---------------------------------------------------------------------------------------------- hand-overs
# The update path's members of a handle (api.hip, struct sgpr_model), which the refits, edits and trials below may allocate:
# sc_dense_part, sc_mae_v, sc_mae_rows, sc_ea_y, sc_ea_rows (5); d_qr_A, d_qr_work (2); sc_s2A ... sc_bwork (17); sc_s2so ...
# sc_chol_info (8); sc_sel_A, sc_sel_work (2); sc_ai_ptr, sc_erow (2); sc_ise (1); r1_cache[4].r1 (4); qr_keep[4] with erows,
# store, Rc, yt, yraw, ysnap, vec each (28); s2k.VT, s2k.R1 (2); sc_s2W, sc_s2flag, sc_potrf (3); d_L, d_R1, d_edit_tmp (3) —
# and one Op::pstore per column selection folded into a kept factorisation.
UPDATE_PATH_MEMBERS = 5 + 2 + 17 + 8 + 2 + 2 + 1 + 4 + 28 + 2 + 3 + 3


def test_hand_overs_neither_leak_nor_double_free():
    from autoforce_amd import SGPRModel
    from autoforce_amd.workloads import inducing_from_frame, lips
    before = _live()
    mdl, (numbers, pos, cell, pbc) = _model()
    pool = inducing_from_frame(mdl, *lips(8, seed=3), 60, seed=9)
    count = lambda: int((_live() - before)[1])

    # sgpr_set_inducing replaces its nine buffers by moves (d_ind_slot, d_ind_nn, d_qoff, d_Pm, d_PmT, d_pm_norm, d_M, d_mu,
    # d_choli), one for one; the K_mm tile table is a member that only grows: nothing new
    mdl.set_inducing(pool[:40])
    c0 = count()
    mdl.set_inducing(pool[:44])
    mdl.set_inducing(pool[4:40])
    c1 = count()
    print("buffers: after set_inducing", c0, "after two more", c1)
    assert c1 - c0 <= 0

    # design_reserve (data.inc): a frame is 1 + 3 * 512 + 6 = 1543 rows; the first push reserves (1543 * 3 / 2 + 63) / 64 * 64 =
    # 2368 rows, the second needs 3086 and grows to 4672, the fourth (6172) grows again.  A growth moves the new buffer into
    # d_design and only RELEASES d_design_alt; the frames have one size, so the rows scratch of the first push serves the rest
    mdl.data_push(*lips(8, seed=100))
    c2 = count()
    for f in range(1, 4):
        mdl.data_push(*lips(8, seed=100 + f))
    c3 = count()
    print("buffers: after the first push", c2, "after three more (two growths)", c3)
    assert mdl.data_info() == (4, 4 * 1543) and c3 - c2 <= 0
    rng = np.random.default_rng(4)
    Y = rng.normal(size=4 * 1543)
    mdl.data_solve(Y)
    assert mdl.solve_info().startswith("stage1=full factorisation;")
    c4 = count()
    assert c4 - c3 <= UPDATE_PATH_MEMBERS

    # sgpr_select_inducing: sc_sel_map, d_edit_tmp (gather_into), d_design_alt and sc_sel_idx (design_select, then the swap),
    # and for the kept factorisation (qr_keep_select) sc_sel_A, sc_sel_work, sc_dense_part and the selection's own Op::pstore
    mdl.select_inducing(list(range(0, 36, 1))[::-1][:32])
    c5 = count()
    print("buffers: after the refit", c4, "after the selection", c5)
    assert c5 - c4 <= 8
    mdl.data_solve(Y)
    assert "selected through the kept reflectors" in mdl.solve_info()

    # trials: every accepted column is one more Op behind the selection's (which owns a buffer) in QrKeep::ops — six of them
    # take the vector through its capacities 1, 2, 4, 8.  The first trial allocates what a trial needs (sgpr_add_inducing's
    # scratch, the second stage's kept factor); the five behind it run the same code on the same members, a flat Op owns no
    # buffer (its reflector lies in the slot's `store`, sized for QR_APPEND_MAX of them at the factorisation) and a member that
    # must grow is replaced one for one: not one buffer more
    trial = []
    for k in range(6):
        mdl.add_inducing(pool[44 + k])
        mdl.data_solve(Y)
        assert "appended / popped through the kept reflectors" in mdl.solve_info()
        trial.append(count())
    print("buffers: after each accepted column", trial)
    assert max(trial[1:]) - trial[0] <= 0
    # a rejected column is popped again: the same members once more
    mdl.add_inducing(pool[50])
    mdl.data_solve(Y)
    mdl.remove_inducing(-1)
    mdl.data_solve(Y)
    c6 = count()
    assert c6 - trial[0] <= 0
    # a frame pushed on top of the kept factor and popped (qr_row_append: sc_ra_y, sc_ra_t, d_R1 the first time; the matrix
    # has room for 9280 rows since the fourth push, and popping the last frame moves nothing) — the second such trial adds nothing
    pushed = []
    for f in range(2):
        mdl.data_push(*lips(8, seed=104 + f))
        mdl.data_solve(np.concatenate([Y, rng.normal(size=1543)]))
        assert "rows of the new frame appended" in mdl.solve_info()
        mdl.data_pop(-1)
        mu = mdl.data_solve(Y)
        pushed.append(count())
    print("buffers: after the rejected column", c6, "after each pushed and popped frame", pushed)
    assert pushed[1] - pushed[0] <= 0
    assert pushed[1] - c3 <= UPDATE_PATH_MEMBERS + 1 + 4      # ... the selection's pstore, and the selection's four above

    # the final model against a fresh handle with the same inducing set and weights, bit for bit
    choli, vscale = mdl.choli, mdl.make_vscale()
    mdl.set_weights(mu, choli=choli, vscale=vscale)
    a = mdl.predict(numbers, pos, cell, pbc)
    fresh = SGPRModel(3, 3, 4, 6.0, species=mdl.species)
    fresh.set_inducing(list(mdl.X))
    fresh.set_weights(mu, choli=choli, vscale=vscale)
    b = fresh.predict(numbers, pos, cell, pbc)
    for key in ("energy", "forces", "stress", "beta"):
        assert np.array_equal(a[key], b[key]), key
    fresh.close()
    mdl.close()
    assert tuple(_live() - before) == (0, 0)


# ---------------------------------------------------------------------------------------------- destroy in the middle of a run
def test_destroy_in_the_middle_of_a_run():
    before = _live()
    s = _setup()
    mdl, (numbers, pos, cell, pbc) = s[0], s[1:5]
    e0 = mdl.predict(numbers, pos, cell, pbc)
    # a covloss halt (column 11 of the rows is the largest covloss), the speculative evaluation behind it discarded, no sgpr_md_end
    _begin(mdl, *s[1:7])
    b = _run(mdl, 30, final=False)[:, 11]
    later = np.nonzero(b > b[:3].max())[0]
    assert len(later), "the covloss never exceeds its starting value on this walk"
    k = int(later[0])
    _begin(mdl, *s[1:7])
    sc, code = mdl.md_run(30, None, ediff=0.5 * (b[:k].max() + b[k]))
    assert code == 1 and len(sc) == k + 1
    mdl.close()
    assert tuple(_live() - before) == (0, 0)
    # ... and with a bias attached, its hills still held
    s = _setup()
    mdl = s[0]
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    mdl.md_meta([("distance", 0, 5)], 0.1, 0.1, capacity=64, merge=4)
    _run(mdl, 10, final=False)
    assert mdl.md_meta_info()["below"] >= 9 and mdl.md_meta_table()[2] >= 4
    mdl.close()
    assert tuple(_live() - before) == (0, 0)
    # a new handle evaluates as the first one did
    mdl, _ = _model()
    e1 = mdl.predict(numbers, pos, cell, pbc)
    for key in ("energy", "forces", "stress", "beta"):
        assert np.array_equal(e0[key], e1[key]), key
    mdl.close()
    assert tuple(_live() - before) == (0, 0)
