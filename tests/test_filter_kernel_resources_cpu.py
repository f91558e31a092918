"""The last kernels of a run with the filter of model-update jumps (sgpr_md_filter) are instantiations of their own —
finalize_next_kernel<5>, <6>, <7>: <2>, <4>, <3> with the accumulator's load and store —, exactly one each, without scratch; the
constant-cell forms stay within 128 VGPRs (four waves per SIMD), the moving-cell form within the 168 that <3> is held to;
md_npt_kernel, which now carries the stress accumulator, and the push kernel keep to md_npt_kernel's limit (no scratch, 128
VGPRs).  That the kernels a run WITHOUT a filter launches are built as before is what the exact counts of
test_fixed_kernel_resources_cpu.py and test_kernel_resources_cpu.py hold.  Reads the metadata of the objects
autoforce_amd/csrc/build.sh leaves behind, as test_fixed_kernel_resources_cpu.py does.

VGPRs / scratch bytes, gfx950, from the compiler's resource report:

    kernel                        without the filter    with it
    finalize_next_kernel<2>            94 / 0             94 / 0
    finalize_next_kernel<3>           136 / 0            136 / 0
    finalize_next_kernel<4>            95 / 0             95 / 0
    finalize_next_kernel<5>               -               96 / 0      (new: <2> with the filter)
    finalize_next_kernel<6>               -               97 / 0      (new: <4> with the filter)
    finalize_next_kernel<7>               -              138 / 0      (new: <3> with the filter)
    md_npt_kernel                     122 / 0            122 / 0
    md_filter_push_kernel                 -               15 / 0      (new)

and the three sgpr_md_filter* entry points are exported by the library and bound in _lib.py."""
import os
import re

import pytest

from test_kernel_resources_cpu import LLVM, OBJ, _metadata

# pattern -> VGPRs at most
FILTERED = {r"finalize_next_kernelILi5E": 128, r"finalize_next_kernelILi6E": 128, r"finalize_next_kernelILi7E": 168,
            r"md_npt_kernel": 128, r"md_filter_push_kernel": 128}


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_filtered_kernels_exist_once_and_do_not_spill(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for pat, vgpr in FILTERED.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert len(hits) == 1, (pat, sorted(hits))
        for name, m in hits.items():
            print(name, m)
            assert m.get("private_segment_fixed_size", 0) == 0, (name, m)
            assert m.get("vgpr_count", 0) <= vgpr, (name, m)
    # the integer template parameter is the only one: no second family of instantiations
    assert len([k for k in meta if "finalize_next_kernel" in k]) == 7


def test_filter_entry_points_are_exported_and_bound():
    import ctypes

    from autoforce_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgpr_hip.h")).read()
    so = os.path.join(root, "autoforce_amd", "libsgpr_hip.so")
    for name in ("sgpr_md_filter", "sgpr_md_filter_push", "sgpr_md_filter_state"):
        assert re.search(r"\bint %s\(sgpr_model \*h" % name, header), name
        assert name in _lib.SIGNATURES, name
    if not os.path.isfile(so):
        pytest.skip("the library has not been built")
    lib = ctypes.CDLL(so)
    for name in ("sgpr_md_filter", "sgpr_md_filter_push", "sgpr_md_filter_state"):
        assert hasattr(lib, name), name
