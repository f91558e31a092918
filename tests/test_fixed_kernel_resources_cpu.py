"""The kernels that hold atoms and components (sgpr_md_fix) use no scratch, and the ones a run WITHOUT a mask launches are the
ones it launched before the mask existed: the masked paths are instantiations of their own.  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_relax_kernel_resources_cpu.py does.

VGPRs / scratch bytes, gfx950, from the compiler's resource report:

    kernel                        before the mask    with it
    finalize_next_kernel<1>            90 / 0          90 / 0
    finalize_next_kernel<2>            94 / 0          94 / 0      (the limit of test_kernel_resources_cpu.py: 96)
    finalize_next_kernel<3>           136 / 0         136 / 0
    finalize_next_kernel<4>               -            95 / 0      (new: <2> with the mask, held to <2>'s limit)
    shard_next_kernel<1>               44 / 0          44 / 0
    shard_next_kernel<2>               79 / 0          79 / 0
    shard_next_kernel<4>                  -            79 / 0      (new)
    md_nh_kernel                        8 / 0           8 / 0      (only its constants change)
    md_fire_kernel        (<false>)   122 / 0         122 / 0
    md_fire_kernel<true>                  -           122 / 0      (new)
    md_fire_move_kernel   (<false>)    24 / 0          24 / 0
    md_fire_move_kernel<true>             -            26 / 0      (new)
"""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

# pattern -> (scratch bytes, VGPRs at most, VGPRs exactly — the count of the commit before the mask — or None)
UNMASKED = {r"finalize_next_kernelILi1E": 90, r"finalize_next_kernelILi2E": 94, r"finalize_next_kernelILi3E": 136,
            r"shard_next_kernelILi1E": 44, r"shard_next_kernelILi2E": 79, r"md_nh_kernel": 8,
            r"md_fire_kernelILb0E": 122, r"md_fire_move_kernelILb0E": 24}
MASKED = {r"finalize_next_kernelILi4E": 96, r"shard_next_kernelILi4E": 128, r"md_fire_kernelILb1E": 128, r"md_fire_move_kernelILb1E": 64}


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_masked_kernels_do_not_spill_and_unmasked_ones_are_unchanged(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in UNMASKED.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert len(hits) == 1, (pat, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
            assert m.get("vgpr_count", 0) == vgpr, (name, m)
    for pat, vgpr in MASKED.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert len(hits) == 1, (pat, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
            assert m.get("vgpr_count", 0) <= vgpr, (name, m)
