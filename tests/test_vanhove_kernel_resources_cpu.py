"""The kernels of the van Hove accumulator (md_vanhove.inc: both forms of md_vh_pair_kernel, md_vh_self_kernel, md_vh_done_kernel)
use no scratch and stay within the 128 VGPRs that leave a SIMD at least four waves (512 / 128) — one atom per thread, nothing
indexed at run time but LDS and the kernels' arguments.  The fused loop launches the kernels it launched before: every kernel
test_vacf_kernel_resources_cpu.KEPT lists and the four kernels of md_vacf.inc keep the register counts of the build without
md_vanhove.inc (read from that build's objects).  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves behind, as
test_vacf_kernel_resources_cpu.py does."""
import os

from test_kernel_resources_cpu import OBJ, _metadata
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects
from test_vacf_kernel_resources_cpu import KEPT as KEPT_VACF

NEW = (r"md_vh_pair_kernelILb0EE", r"md_vh_pair_kernelILb1EE", r"md_vh_self_kernel", r"md_vh_done_kernel")
KEPT = dict(KEPT_VACF)
KEPT.update({r"md_vacf_store_kernel": 42, r"md_vacf_corr_kernel": 18, r"md_vacf_fold_kernel": 56, r"md_vacf_done_kernel": 4})


@needs_objects
def test_vanhove_kernels_do_not_spill(tmp_path):
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
