"""Records tests/golden/fixed_twins_unmasked.npz: the walks of fixed_common.walks() — the three host twins called without a
`fixed` keyword — on the package found first on the path.  Run against the commit BEFORE the twins learnt `fixed=`:

    PYTHONPATH=<checkout of that commit> python tests/golden/gen/make_fixed_twins.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.append(TESTS)
sys.path.append(os.path.dirname(TESTS))

import autoforce_amd.workloads as wl  # noqa: E402
from fixed_common import walks  # noqa: E402

if __name__ == "__main__":
    print("twins of", wl.__file__)
    np.savez(os.path.join(os.path.dirname(HERE), "fixed_twins_unmasked.npz"), **walks())
