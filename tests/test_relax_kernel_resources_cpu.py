"""The two kernels of the device relaxation (md_relax.inc) use no scratch.  md_fire_move_kernel, the per-atom one, is bound by
its two dependent memory round trips (permutation -> force), so it is launched as many small waves that must all be resident at
once: within 64 VGPRs a SIMD holds eight of them, the most the hardware schedules, and the kernel has no use for more
registers (a dozen live doubles per lane).  md_fire_kernel is one workgroup whose lane 0 carries the 3 x 3 algebra: 128 VGPRs,
the bound md_npt_kernel is held to.  Reads the metadata of the objects autoforce_amd/csrc/build.sh leaves behind, as
test_npt_kernel_resources_cpu.py does."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

LIMITS = {r"md_fire_move_kernel": (0, 64), r"md_fire_kernel": (0, 128)}


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_relaxation_kernels_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, (scratch, vgpr) in LIMITS.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, m in hits.items():
            print(name, {k: m.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
            assert m.get("private_segment_fixed_size", 0) <= scratch, (name, m)
            assert m.get("vgpr_count", 0) <= vgpr, (name, m)
