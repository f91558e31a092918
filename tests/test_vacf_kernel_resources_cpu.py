"""The four kernels of the velocity-correlation accumulator (md_vacf.inc) use no scratch and stay within the 128 VGPRs that leave a
SIMD at least four waves (512 / 128) — one atom per thread, its velocity in registers, nothing indexed at run time but LDS and
the kernels' arguments.  The fused loop launches the kernels it launched before: every form of finalize_next_kernel,
md_record_kernel and md_nh_kernel keep the register counts test_msd_kernel_resources_cpu.py lists, and the kernels of md_msd.inc
and md_rdf.inc those of the build without md_vacf.inc.  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves
behind, as test_msd_kernel_resources_cpu.py does."""
import os

from test_kernel_resources_cpu import OBJ, _metadata
from test_msd_kernel_resources_cpu import KEPT as KEPT_MSD
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects

NEW = (r"md_vacf_store_kernel", r"md_vacf_corr_kernel", r"md_vacf_fold_kernel", r"md_vacf_done_kernel")
KEPT = dict(KEPT_MSD)
KEPT.update({r"md_msd_part_kernel": 24, r"md_msd_fold_kernel": 62, r"md_rdf_pair_kernelILb0EE": 38, r"md_rdf_pair_kernelILb1EE": 54,
             r"md_rdf_done_kernel": 6})


@needs_objects
def test_vacf_kernels_do_not_spill(tmp_path):
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
