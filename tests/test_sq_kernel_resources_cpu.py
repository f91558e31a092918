"""The kernels of the structure-factor accumulator of the device MD loop (md_sq.inc: both forms of md_sq_part_kernel,
md_sq_fold_kernel, md_sq_done_kernel) use no scratch and stay within the 128 VGPRs that leave a SIMD at least four waves: the
powers live in LDS (a static_assert keeps the tables within 64 KiB), the fold's densities too, nothing is indexed at run time but LDS and the kernels' arguments.  What the
include costs the other kernels is test_accumulator_kernel_resources_cpu.py's KEPT, which stands as it is.  Reads the metadata of
the objects autoforce_amd/csrc/build.sh leaves behind."""
import os

import pytest

from test_kernel_resources_cpu import OBJ, _metadata
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects

SQ = (r"md_sq_part_kernelILi64ELi17EE", r"md_sq_part_kernelILi32ELi33EE", r"md_sq_fold_kernel", r"md_sq_done_kernel")


@needs_objects
@pytest.mark.parametrize("pat", SQ)
def test_sq_kernels_do_not_spill(pat, tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    name, m = _one(meta, pat)
    print(name, m)
    assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
    assert 0 < m.get("vgpr_count", 0) <= FOUR_WAVES, (name, m)
