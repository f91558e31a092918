"""Records tests/golden/g18_loop_trace.json: the traces of tests/loop_trace.py's scenarios — what run_md, run_relax and run_neb
do around a scripted engine — on the package found first on the path.  Run against the commit BEFORE the three methods were
moved onto autoforce_amd/device_loop.py (the helper needs nothing newer than their public signatures):

    PYTHONPATH=<checkout of that commit> python tests/golden/gen/make_loop_trace.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.append(TESTS)
sys.path.append(os.path.dirname(TESTS))

import autoforce_amd.calculator as cal  # noqa: E402
from loop_trace import run_all  # noqa: E402

if __name__ == "__main__":
    print("run_md / run_relax / run_neb of", cal.__file__)
    with open(os.path.join(os.path.dirname(HERE), "g18_loop_trace.json"), "w") as f:
        json.dump(run_all(), f, separators=(",", ":"))
        f.write("\n")
