"""GPU tests of what sgpr_md_begin owes to the handle's past: nothing but the seed.  The run state of the device loop is a value
(MdRun, api.hip) that sgpr_md_begin replaces whole — a run begun behind ANY mode of the loop is the run begun on a fresh
handle, bit for bit, and the modes' inspection calls refuse it; a sgpr_md_begin that fails leaves the handle with no run at
all; and the seed, the one setting with a contract across sgpr_md_begin (sgpr_md_seed needs no run), survives it.  Frame,
model and mode runners are test_hip_npt_device._setup()'s and test_hip_teardown.FEATURES' (512-atom lips(8), 48 inducing
points); the reference run R — seeded Langevin, six evaluations cut (2, 4) — is computed once on the handle every case shares."""
import ctypes as C

import numpy as np
import pytest

from test_hip_npt_device import _setup
from test_hip_teardown import FEATURES, _begin

pytestmark = pytest.mark.gpu

MODES = ["nose_hoover", "barostat", "relax", "relax_cell", "ml_filter", "fixed", "record", "meta_merge", "committee", "neb"]


def _R(mdl, s):
    """The reference run: rows of its six evaluations, and the state it ends in."""
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    rows = []
    for n, final in ((2, False), (4, True)):
        sc, code = mdl.md_run(n, None, final=final)
        assert code == 0 and len(sc) == n
        rows.append(sc)
    return np.concatenate(rows), mdl.md_state(results=True)


def _same(a, b):
    assert np.array_equal(a[0], b[0]), "scalar rows"
    for key in ("positions", "velocities_pre", "velocities", "forces", "beta", "energy", "stress"):
        assert np.array_equal(np.asarray(a[1][key]), np.asarray(b[1][key])), key


def _lib_begin(mdl, s, mass):
    """sgpr_md_begin itself (the wrapper's md_begin seeds again behind it): its return code."""
    from autoforce_amd import _lib
    from autoforce_amd.ase_shim import kB
    from autoforce_amd.workloads import FS
    from test_hip_teardown import T
    numbers, pos, cell, pbc, _, vel = s[1:7]
    N = len(numbers)
    return _lib.load().sgpr_md_begin(mdl._h, N, _lib.ptr(_lib.i32(numbers)), _lib.ptr(_lib.f64(pos).reshape(N, 3)),
                                     _lib.ptr(_lib.f64(np.asarray(cell, float).reshape(3, 3))),
                                     _lib.ptr(_lib.i32(np.asarray(pbc, bool).astype(np.int32))), _lib.ptr(_lib.f64(mass)),
                                     _lib.ptr(_lib.f64(vel).reshape(N, 3)), 1.0 * FS, 0.05, kB * T)


@pytest.fixture(scope="module")
def shared():
    s = _setup()
    first = _R(s[0], s)
    yield s, first
    s[0].close()


@pytest.mark.parametrize("mode", MODES)
def test_a_new_run_owes_nothing_to_the_last_one(shared, mode):
    from autoforce_amd import _lib
    s, first = shared
    mdl = s[0]
    FEATURES[mode](mdl, s)
    again = _R(mdl, s)
    print(f"behind {mode}: rows equal {np.array_equal(first[0], again[0])}, largest |dE| {np.abs(first[0][:, 0] - again[0][:, 0]).max():.3e}")
    _same(first, again)
    # the last mode's inspection calls refuse the plain run
    for call, what in ((lambda: mdl.md_cells(0, 1), "sgpr_md_barostat"), (mdl.md_filter_state, "sgpr_md_filter"),
                       (mdl.md_meta_info, "sgpr_md_meta"), (mdl.md_committee_info, "sgpr_md_committee")):
        with pytest.raises(_lib.SgprError, match=f"call sgpr_md_begin and {what}"):
            call()
    out = np.zeros(32)   # (the wrapper's neb_info answers from its own record: the entry point itself)
    assert _lib.load().sgpr_md_neb_info(mdl._h, 0, 1, _lib.ptr(out)) == -1
    assert b"call sgpr_md_begin and sgpr_md_neb first" in _lib.load().sgpr_last_error()
    assert mdl.md_frame_count() == 0


def test_a_failed_begin_leaves_no_run(shared):
    from autoforce_amd import _lib
    s, first = shared
    mdl = s[0]
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    sc, code = mdl.md_run(2, None)
    assert code == 0 and len(sc) == 2
    mass = np.array(s[5], float)
    mass[len(mass) // 2] = 0.0     # (rejected on the host, behind the bind and the allocation: nothing reaches the device loop)
    assert _lib_begin(mdl, s, mass) == -1
    assert b"is not positive" in _lib.load().sgpr_last_error()
    with pytest.raises(_lib.SgprError, match="sgpr_md_run: call sgpr_md_begin first"):
        mdl.md_run(2, None)
    _same(first, _R(mdl, s))


def test_the_seed_survives_a_begin(shared):
    from autoforce_amd import _lib
    s, first = shared
    mdl = s[0]
    _begin(mdl, *s[1:7], friction=0.05, seed=3)     # (the wrapper's own record of a run of this frame; the handle's seed is now 3)
    other, code = mdl.md_run(4, None)
    assert code == 0 and not np.array_equal(other, first[0][:4])
    mdl.md_end()
    assert _lib.load().sgpr_md_seed(mdl._h, 7) == 0
    assert _lib_begin(mdl, s, s[5]) == 0
    rows, code = mdl.md_run(4, None)
    assert code == 0 and len(rows) == 4
    # the first call of R is two evaluations and moves on behind both; this one is four: the same trajectory, row for row
    _begin(mdl, *s[1:7], friction=0.05, seed=7)
    want, code = mdl.md_run(4, None)
    assert code == 0 and np.array_equal(rows, want)
