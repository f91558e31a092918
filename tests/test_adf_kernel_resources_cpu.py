"""The kernels of the bond-angle accumulator (md_adf.inc: both counter forms of md_adf_kernel, md_adf_done_kernel) use no scratch
and stay within the 128 VGPRs that leave a SIMD at least four waves (512 / 128) — nothing indexed at run time but LDS and the
kernels' arguments (the per-species counts of a centre live one per lane, not in an array).  The fused loop launches the kernels it
launched before: every kernel test_vanhove_kernel_resources_cpu.KEPT lists and the kernels of md_vanhove.inc keep the register
counts of the build without md_adf.inc (read from that build's objects).  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_vanhove_kernel_resources_cpu.py does."""
import os

from test_kernel_resources_cpu import OBJ, _metadata
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects
from test_vanhove_kernel_resources_cpu import KEPT as KEPT_VANHOVE

NEW = (r"md_adf_kernelILb0EE", r"md_adf_kernelILb1EE", r"md_adf_done_kernel")
KEPT = dict(KEPT_VANHOVE)
KEPT.update({r"md_vh_pair_kernelILb0EE": 38, r"md_vh_pair_kernelILb1EE": 54, r"md_vh_self_kernel": 44, r"md_vh_done_kernel": 6})


@needs_objects
def test_adf_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat in NEW:
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert 0 < m.get("vgpr_count", 0) <= FOUR_WAVES, (name, m)


@needs_objects
def test_fused_loop_and_accumulator_kernels_are_the_ones_they_were(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in KEPT.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) == vgpr, (name, m)
