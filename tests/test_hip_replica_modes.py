"""GPU test of what a band and a polymer share on one handle (MdState::rep, md_replica_run): the rings of positions and packed
results and the device record of a call belong to whichever of the two the run is.  A band of K = 3, a polymer of P = 5 and a
band of K = 2 run one after the other on ONE handle; each must give the bits of the same run on a fresh handle — a row width, a
replica count or a ring capacity left over from the mode before would show in the scalars, the record or the state —, and the
readers of the other mode refuse.  Frame (200 of its atoms), model and helpers are those of test_hip_neb_device.py and
test_hip_pimd_device.py."""
import numpy as np
import pytest

from test_hip_neb_device import FMAX, _band
from test_hip_npt_device import _model
from test_hip_pimd_device import _begin as _begin_pimd, _polymer

pytestmark = pytest.mark.gpu

EVALS = 4


def _band_run(mdl, numbers, pos, cell, pbc, keep, K):
    mdl.neb_begin(numbers[keep], _band(pos, K, keep=keep), cell, pbc, FMAX)
    return _collect(mdl, mdl.neb_info, mdl.neb_state)


def _polymer_run(mdl, numbers, pos, cell, pbc, keep, P):
    numbers, beads, vel, mass = _polymer(numbers, pos, P, keep=keep)
    _begin_pimd(mdl, numbers, beads, vel, mass, cell, pbc, seed=5)   # (the deviates are drawn on the device)
    return _collect(mdl, mdl.pimd_info, mdl.pimd_state)


def _collect(mdl, info, state):
    """The scalar rows, the record, the current configuration and the one the call evaluated last with its results."""
    sc, code = mdl.md_run(EVALS, None)
    assert code == 0 and len(sc) == EVALS and np.all(np.isfinite(sc))
    E, cov = info()
    assert len(E) == EVALS
    out = dict(scalars=sc, E=E, covmax=cov)
    out.update({"now." + k: v for k, v in state().items()})
    out.update({"last." + k: v for k, v in state(which=-1, results=True).items()})
    return out


def test_a_band_a_polymer_and_a_band_on_one_handle_are_the_runs_of_fresh_handles():
    from autoforce_amd import _lib
    from autoforce_amd._lib import ptr
    mdl, (numbers, pos, cell, pbc) = _model()
    keep = np.sort(np.random.default_rng(11).choice(len(numbers), size=200, replace=False))
    runs = [(_band_run, 3), (_polymer_run, 5), (_band_run, 2)]
    got = []
    for k, (run, R) in enumerate(runs):
        got.append(run(mdl, numbers, pos, cell, pbc, keep, R))
        if k == 1:   # the run is a polymer: the band's reader refuses
            assert _lib.load().sgpr_md_neb_state(mdl.handle, None, None, None, 0) == _lib.E_INVALID
        if k == 2:   # the run is a band again: the polymer's reader refuses
            assert _lib.load().sgpr_md_pimd_info(mdl.handle, 0, 1, ptr(np.zeros((1, 64)))) == _lib.E_INVALID
    mdl.close()
    for (run, R), a in zip(runs, got):
        fresh, _ = _model()
        b = run(fresh, numbers, pos, cell, pbc, keep, R)
        fresh.close()
        assert a["E"].shape == (EVALS, R) and a["now.positions"].shape == (R, 200, 3) and a["last.energy"].shape == (R,)
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), (run.__name__, R, key)
