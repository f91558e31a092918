"""The kernels of the accumulators of the device MD loop (md_msd.inc, md_rdf.inc, md_vacf.inc, md_vanhove.inc, md_adf.inc; NEW has
one list per accumulator) use no scratch and stay within the 128 VGPRs that leave a SIMD at least four waves (512 / 128): a thread
keeps its atom and its sums in registers, nothing is indexed at run time but LDS and the kernels' arguments.  And an accumulator
costs the others nothing: every form of finalize_next_kernel, md_record_kernel, md_nh_kernel and the accumulator kernels that had
a successor built beside them (KEPT) keep the register counts of the builds without it — a further accumulator adds its list to
NEW and leaves KEPT's numbers alone.  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves behind, as
test_pimd_kernel_resources_cpu.py does."""
import os

import pytest

from test_kernel_resources_cpu import OBJ, _metadata
from test_pimd_kernel_resources_cpu import FOUR_WAVES, _one, needs_objects

NEW = dict(msd=(r"md_msd_part_kernel", r"md_msd_fold_kernel"),
           rdf=(r"md_rdf_pair_kernelILb0EE", r"md_rdf_pair_kernelILb1EE", r"md_rdf_done_kernel"),
           vacf=(r"md_vacf_store_kernel", r"md_vacf_corr_kernel", r"md_vacf_fold_kernel", r"md_vacf_done_kernel"),
           vanhove=(r"md_vh_pair_kernelILb0EE", r"md_vh_pair_kernelILb1EE", r"md_vh_self_kernel", r"md_vh_done_kernel"),
           adf=(r"md_adf_kernelILb0EE", r"md_adf_kernelILb1EE", r"md_adf_done_kernel"))
KEPT = {r"finalize_next_kernelILi1EE": 90, r"finalize_next_kernelILi2EE": 94, r"finalize_next_kernelILi3EE": 136, r"finalize_next_kernelILi4EE": 95,
        r"finalize_next_kernelILi5EE": 96, r"finalize_next_kernelILi6EE": 97, r"finalize_next_kernelILi7EE": 138,
        r"md_record_kernel": 10, r"md_nh_kernel": 8,
        r"md_msd_part_kernel": 24, r"md_msd_fold_kernel": 62,
        r"md_rdf_pair_kernelILb0EE": 38, r"md_rdf_pair_kernelILb1EE": 54, r"md_rdf_done_kernel": 6,
        r"md_vacf_store_kernel": 42, r"md_vacf_corr_kernel": 18, r"md_vacf_fold_kernel": 56, r"md_vacf_done_kernel": 4,
        r"md_vh_pair_kernelILb0EE": 38, r"md_vh_pair_kernelILb1EE": 54, r"md_vh_self_kernel": 44, r"md_vh_done_kernel": 6}


@needs_objects
@pytest.mark.parametrize("which", list(NEW))
def test_accumulator_kernels_do_not_spill(which, tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat in NEW[which]:
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
