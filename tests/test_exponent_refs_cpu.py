"""The two host references of the similarity kernel against each other at every exponent the GPU tests use
(exponent_common.ETAS), so that a failure of test_hip_exponent.py points at the device: step_ref.knm (long double, with
its a-priori bound) and the oracle's kernel_matrix (double; a multiply loop for integers up to 64, pow() otherwise), on the
inducing sets of three edge frames of test_hip_step_edges and on four LCEs with pairwise orthogonal descriptors.

The orthogonal pairs must be exactly 0 at every exponent, also below 1 where the derivative is unbounded there; no other
same-species dot product of the edge frames may be zero or negative (a negative one has no real power for a non-integer
exponent, and the GPU tests rely on there being none)."""
import numpy as np
import pytest

import step_ref as ref
from exponent_common import ETAS, ORTHO_PAIRS, ORTHO_SPECIES, RC, oracle_inducing, orthogonal_lces
from test_hip_step_edges import EDGES, inducing, slots_of

SETS = ("s5", "s16", "s1", "ortho")


def _set(name):
    if name == "ortho":
        return ORTHO_SPECIES, orthogonal_lces()
    sp, _, qc, _ = EDGES[name]
    return sp, inducing(sp, qc, 0)


@pytest.fixture(scope="module", params=SETS)
def inducing_set(request):
    sp, X = _set(request.param)
    ind_z, Pm, nnm = oracle_inducing(X, sp, RC)
    Q = np.asarray(Pm, float).reshape(len(X), -1)
    return request.param, ind_z, Pm, nnm, Q, slots_of(sp, ind_z)


def test_dot_products_of_the_sets(inducing_set):
    name, ind_z, Pm, nnm, Q, zq = inducing_set
    assert np.all(nnm > 0)                                    # (no lone LCE: every entry below is a power of a dot product)
    V = Q @ Q.T
    same = zq[:, None] == zq[None, :]
    if name == "ortho":
        zero = np.zeros_like(same)
        for a, b in ORTHO_PAIRS:
            zero[a, b] = zero[b, a] = True
        assert np.all(V[zero] == 0.0) and np.all(V[same & ~zero] > 0.0)
    else:
        assert V[same].min() > 0.0, (name, V[same].min())


@pytest.mark.parametrize("eta", ETAS)
def test_references_agree(inducing_set, eta):
    from oracle import oracle as orc
    name, ind_z, Pm, nnm, Q, zq = inducing_set
    lone = nnm == 0
    K, bK = ref.knm(Q, Q, zq, zq, lone, lone, eta)
    Ko = orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, eta)
    # (a comparison with a NaN is False: check_knm alone would let one through)
    assert np.all(np.isfinite(Ko)) and np.all(np.isfinite(K.astype(float))) and np.all(np.isfinite(bK)), (name, eta)
    ref.check_knm(Ko, K, bK, zq, zq, what=(name, eta))
    if name == "ortho":
        for a, b in ORTHO_PAIRS:
            assert Ko[a, b] == 0.0 and Ko[b, a] == 0.0 and K[a, b] == 0 and K[b, a] == 0, (eta, a, b)
            assert bK[a, b] == 0.0 and bK[b, a] == 0.0        # every product of the dot is an exact zero: nothing to round
        assert np.count_nonzero(Ko) == 16 - 2 * len(ORTHO_PAIRS)
