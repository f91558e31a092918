"""The kernels of the pair-distance accumulator (md_rdf.inc) use no scratch and stay within the 128 VGPRs that leave a SIMD at
least four waves (512 / 128) — both forms of md_rdf_pair_kernel keep one i-atom per thread in registers and index nothing at
run time but LDS and the kernel's arguments.  The fused loop launches the kernels it launched before: every form of
finalize_next_kernel, md_record_kernel and md_nh_kernel keep the register counts test_msd_kernel_resources_cpu.py lists: those
of the build without md_rdf.inc.  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves behind, as
test_msd_kernel_resources_cpu.py does."""
import os

from test_kernel_resources_cpu import OBJ, _metadata
from test_msd_kernel_resources_cpu import KEPT as KEPT_MSD
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects

NEW = (r"md_rdf_pair_kernelILb0EE", r"md_rdf_pair_kernelILb1EE", r"md_rdf_done_kernel")
KEPT = dict(KEPT_MSD)


@needs_objects
def test_rdf_kernels_do_not_spill(tmp_path):
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
