"""The two kernels of the moving-cell MD loop (md_npt.inc, finalize_next_kernel<3>) use no scratch, and the per-atom one
keeps three waves per SIMD (168 VGPRs at most: 512 / 3 in allocation granules of 8).  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_kernel_resources_cpu.py does for the other hot kernels."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

LIMITS = {r"finalize_next_kernelILi3E": (0, 168), r"md_npt_kernel": (0, 128)}


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_moving_cell_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, (scratch, vgpr) in LIMITS.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, m in hits.items():
            assert m.get("private_segment_fixed_size", 0) <= scratch, (name, m)
            assert m.get("vgpr_count", 0) <= vgpr, (name, m)
