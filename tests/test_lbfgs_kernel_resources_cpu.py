"""The four kernels of L-BFGS in the device relaxation (md_lbfgs.inc) use no scratch, and a FIRE run launches the kernels it
launched before: md_fire_kernel and md_fire_move_kernel share md_relax.inc's device functions with the new kernels and keep the
register counts test_fixed_kernel_resources_cpu.py records for them (122 and 24 VGPRs, no scratch).  md_lbfgs_dir_kernel and
md_lbfgs_move_kernel are per-row kernels whose waves should all be resident: within 64 VGPRs a SIMD holds eight of them.
md_lbfgs_dots_kernel (seven block sums) and md_lbfgs_solve_kernel (one workgroup, the 3 x 3 algebra on lane 0) are held to the 128
of md_fire_kernel.  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves behind, as
test_relax_kernel_resources_cpu.py does."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

NEW = {r"md_lbfgs_dots_kernelILb0E": 128, r"md_lbfgs_dots_kernelILb1E": 128, r"md_lbfgs_solve_kernel": 128,
       r"md_lbfgs_dir_kernelILb0E": 64, r"md_lbfgs_dir_kernelILb1E": 64, r"md_lbfgs_move_kernelILb0E": 64, r"md_lbfgs_move_kernelILb1E": 64}
FIRE = {r"md_fire_kernelILb0E": 122, r"md_fire_move_kernelILb0E": 24}

needs_objects = pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                                   reason="no build objects / LLVM tools")


def _one(meta, pat):
    hits = {k: v for k, v in meta.items() if re.search(pat, k)}
    assert len(hits) == 1, (pat, sorted(hits))
    (name, m), = hits.items()
    print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
    return name, m


@needs_objects
def test_lbfgs_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in NEW.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) <= vgpr, (name, m)


@needs_objects
def test_fire_kernels_are_the_ones_they_were(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in FIRE.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) == vgpr, (name, m)
