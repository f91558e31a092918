"""The two kernels of the displacement accumulator (md_msd.inc) use no scratch and stay within the 128 VGPRs that leave a SIMD
at least four waves (512 / 128) — md_msd_part_kernel keeps one atom per thread and its seven sums in registers, nothing is
indexed at run time but LDS.  The fused loop launches the kernels it launched before: every form of finalize_next_kernel,
md_record_kernel and md_nh_kernel keep the register counts of the build without md_msd.inc.  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_pimd_kernel_resources_cpu.py does."""
import os

from test_kernel_resources_cpu import OBJ, _metadata
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects

NEW = (r"md_msd_part_kernel", r"md_msd_fold_kernel")
KEPT = {r"finalize_next_kernelILi1EE": 90, r"finalize_next_kernelILi2EE": 94, r"finalize_next_kernelILi3EE": 136, r"finalize_next_kernelILi4EE": 95,
        r"finalize_next_kernelILi5EE": 96, r"finalize_next_kernelILi6EE": 97, r"finalize_next_kernelILi7EE": 138,
        r"md_record_kernel": 10, r"md_nh_kernel": 8}


@needs_objects
def test_msd_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat in NEW:
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert 0 < m.get("vgpr_count", 0) <= FOUR_WAVES, (name, m)


@needs_objects
def test_fused_loop_kernels_are_the_ones_they_were(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in KEPT.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) == vgpr, (name, m)
