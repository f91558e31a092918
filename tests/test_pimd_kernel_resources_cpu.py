"""The three kernels of the ring polymer in the device loop (md_pimd.inc) use no scratch — md_pimd_move_kernel keeps its modes in
LDS and registers: no per-thread array indexed at run time — and md_pimd_move_kernel stays within the 128 VGPRs that leave a SIMD
at least four waves (512 / 128); the build gives it 104, md_pimd_sums_kernel 66 and md_pimd_gate_kernel 30, and those counts are
held as they are.  A band and the fused loop launch the kernels they launched before: md_neb_* and every form of
finalize_next_kernel keep the register counts of the build without md_pimd.inc.  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_lbfgs_kernel_resources_cpu.py does."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

NEW = {r"md_pimd_sums_kernel": 66, r"md_pimd_gate_kernel": 30, r"md_pimd_move_kernel": 104}
FOUR_WAVES = 128
KEPT = {r"md_neb_sums_kernel": 62, r"md_neb_fire_kernel": 98, r"md_neb_move_kernel": 58,
        r"finalize_next_kernelILi1EE": 90, r"finalize_next_kernelILi2EE": 94, r"finalize_next_kernelILi3EE": 136, r"finalize_next_kernelILi4EE": 95,
        r"finalize_next_kernelILi5EE": 96, r"finalize_next_kernelILi6EE": 97, r"finalize_next_kernelILi7EE": 138}

needs_objects = pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                                   reason="no build objects / LLVM tools")


def _one(meta, pat):
    hits = {k: v for k, v in meta.items() if re.search(pat, k)}
    assert len(hits) == 1, (pat, sorted(hits))
    (name, m), = hits.items()
    print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
    return name, m


@needs_objects
def test_pimd_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in NEW.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) == vgpr <= FOUR_WAVES, (name, m)


@needs_objects
def test_band_and_fused_loop_kernels_are_the_ones_they_were(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in KEPT.items():
        name, m = _one(meta, pat)
        assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("vgpr_count", 0) == vgpr, (name, m)
