"""The Steinhardt Q_l colvar without a GPU: workloads.meta_bias's kind "qlvar" — the definition the device loop's kernels are
compared with — against the reference's own Qlvar (tests/golden/g17_qlvar.npz, made by tests/golden/gen/make_qlvar.py from
calculator/meta.py's Qlvar over descriptor/ql.py with autograd), its gradient against central differences, its invariances,
the images of a small cell, and autoforce_amd.meta.Qlvar inside Meta / Catvar.

  Against the fixture, for a fixed dV/dQ: Q, forces -sum_d g_d dQ_d/dx and the virial the reference's grads() forms from
-sum x (x) F plus the cell-gradient term, gated at 1e-6 of the largest component (BASELINE's force contract).  Measured on the
first run, relative to the largest component: Q <= 1.2e-15, forces <= 1.1e-14, virial <= 4.1e-15 over the eight cases
(DESIGN section 3 has them per case) — the addition theorem and the reference's Y_lm sum agree to rounding.  That includes
si32 atom 5 (its own images stand ON the z axis) and slab18_nearz: there the reference's Ylm shears the whole environment by 1e-2
(descriptor/ylm.py:10-23), which moves Q_l itself by a few 1e-5 (x keeps its scale, y and z gain sqrt(1 + 1e-4)); the twin applies
the same shear (workloads.ql_rows) — without it Q4 / Q6 of slab18_nearz differ by 4.0e-6 / 1.8e-5 from the fixture, with it by
rounding, and the twin's central difference agrees with its gradient on that case (below)."""
import os

import numpy as np
import pytest

from helpers import load
from test_kernel_resources_cpu import LLVM, OBJ, _metadata

GATE = 1e-6
RC = 6.0


@pytest.fixture(scope="module")
def g17():
    return load("g17_qlvar")


NAMES = ["si32_a0", "si32_a5_images", "tric24_a0", "tric24_last", "mixed64_zr_c4", "mixed64_zr_c6", "slab18_nearz", "cluster16_a0"]
SELECTED = dict(si32_a0=16, si32_a5_images=46, tric24_a0=34, tric24_last=21, mixed64_zr_c4=11, mixed64_zr_c6=27, slab18_nearz=9, cluster16_a0=4)


def case(g17, name):
    g = load(str(g17[f"{name}_frame"]))
    cvs = [("qlvar", int(g17[f"{name}_index"]), int(g17[f"{name}_j"]), float(g17[f"{name}_cutoff"]), tuple(int(l) for l in g17[f"{name}_l"]))]
    return g["numbers"], g["positions"], g["cell"].reshape(3, 3), np.asarray(g["pbc"], bool), cvs


def biased(cvs, numbers, x, cell, pbc, sigma=0.05, w=1.0, tem=None, off=0.03, **kw):
    """The twin with one hill `off` beside the CV: dV/dQ is not zero in any dimension."""
    from autoforce_amd.workloads import meta_bias
    cv0 = meta_bias(cvs, sigma, w, numbers, x, cell, None, pbc=pbc, rc=RC, **kw)["cv"]
    return meta_bias(cvs, sigma, w, numbers, x, cell, (cv0 + off)[None, :], tem=tem, pbc=pbc, rc=RC, **kw), cv0 + off


def test_fixture_holds_the_cases_of_the_issue(g17):
    assert sorted(str(n) for n in g17["names"]) == sorted(NAMES) and float(g17["rc"]) == RC
    for name in NAMES:
        assert int(g17[f"{name}_selected"]) == SELECTED[name], name
        assert float(g17[f"{name}_gap"]) > 1e-2 and g17[f"{name}_Q"].min() >= 0.15, name   # no neighbour on the sphere, every Q_l well away from 0
        D = len(g17[f"{name}_l"])
        N = len(load(str(g17[f"{name}_frame"]))["numbers"])
        assert g17[f"{name}_dQdx"].shape == (D, N, 3) and g17[f"{name}_dQdcell"].shape == (D, 3, 3)
        assert np.isfinite(g17[f"{name}_dQdx"]).all() and np.isfinite(g17[f"{name}_dQdcell"]).all()
    g = load("g5_mixed64")
    assert int(g17["mixed64_zr_c4_index"]) == int(np.where(g["numbers"] == 40)[0][0])       # the first Zr
    assert int(g17["tric24_last_index"]) == len(load("g5_tric24")["numbers"]) - 1


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_the_reference(g17, name):
    from autoforce_amd.workloads import ql_environment
    numbers, x, cell, pbc, cvs = case(g17, name)
    out, _ = biased(cvs, numbers, x, cell, pbc)
    assert len(ql_environment(numbers, x, cell, pbc, cvs[0][1], cvs[0][2], cvs[0][3])[0]) == SELECTED[name]
    g = out["dcv"]
    assert np.abs(g).min() > 1e-3                                     # every dimension pulls
    Qr, gx, gc = g17[f"{name}_Q"], g17[f"{name}_dQdx"], g17[f"{name}_dQdcell"]
    F_ref = -np.tensordot(g, gx, axes=1)
    # the reference's grads(): virial = sum x (x) dV/dx + cell^T dV/dcell
    vir_ref = (x[:, :, None] * (-F_ref)[:, None, :]).sum(0) + np.tensordot(g, np.einsum("ka,dkb->dab", cell, gc), axes=1)
    figs = dict(Q=np.abs(out["cv"] - Qr).max() / np.abs(Qr).max(), F=np.abs(out["forces"] - F_ref).max() / np.abs(F_ref).max(),
                vir=np.abs(out["virial"].reshape(3, 3) - vir_ref).max() / np.abs(vir_ref).max())
    print(f"qlvar twin vs reference {name}: Q {out['cv']} relative gaps " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert np.abs(F_ref).max() > 1e-2
    assert figs["Q"] <= GATE and figs["F"] <= GATE and figs["vir"] <= GATE, figs
    vol = abs(np.linalg.det(cell))
    if vol > 0:
        np.testing.assert_allclose(out["stress"], out["virial"][[0, 4, 8, 5, 2, 1]] / vol, rtol=1e-15)


@pytest.mark.parametrize("name", ["si32_a5_images", "slab18_nearz", "tric24_a0", "cluster16_a0"])
def test_gradient_against_central_differences(g17, name):
    """Forces on the index atom, three of its neighbours and one atom outside the environment; slab18_nearz and si32 atom 5 are the
    cases whose environment the reference shears: the twin's own difference quotient agrees with its gradient there too."""
    from autoforce_amd.workloads import meta_bias, ql_environment
    numbers, x, cell, pbc, cvs = case(g17, name)
    out, hill = biased(cvs, numbers, x, cell, pbc)
    env = ql_environment(numbers, x, cell, pbc, cvs[0][1], cvs[0][2], cvs[0][3])[0]
    outside = [a for a in range(len(numbers)) if a not in set(env.tolist()) | {cvs[0][1]}][:1]
    h, worst = 1e-5, 0.0
    for a in [cvs[0][1]] + sorted(set(env.tolist()))[:3] + outside:
        for k in range(3):
            e = []
            for s in (+h, -h):
                xs = x.copy()
                xs[a, k] += s
                e.append(meta_bias(cvs, 0.05, 1.0, numbers, xs, cell, hill[None, :], pbc=pbc, rc=RC)["energy"])
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - out["forces"][a, k]))
    print(f"qlvar central differences {name}: worst gap {worst:.2e} of max |F| {np.abs(out['forces']).max():.2e}")
    assert worst <= 1e-7 * np.abs(out["forces"]).max()               # h^2 f''' / 6 with h = 1e-5, and the rounding of the difference
    for a in outside:
        assert not out["forces"][a].any()
    # the strain derivative: x -> x (1 + e), cell -> cell (1 + e) moves every r_t alike: dV/de_ab = virial_ab
    for a, b in ((0, 0), (1, 2), (2, 1)):
        e = []
        for s in (+h, -h):
            m = np.eye(3)
            m[a, b] += s
            e.append(meta_bias(cvs, 0.05, 1.0, numbers, x @ m, cell @ m, hill[None, :], pbc=pbc, rc=RC)["energy"])
        assert abs((e[0] - e[1]) / (2 * h) - out["virial"][3 * a + b]) <= 1e-7 * np.abs(out["virial"]).max(), (a, b)


def test_rigid_rotation_leaves_q_alone_and_the_virial_is_symmetric(g17):
    from autoforce_amd.workloads import QL_TINY_ANGLE, ql_environment
    rng = np.random.default_rng(5)
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    cone = lambda r: bool(((np.abs(r[:, 0]) < QL_TINY_ANGLE * np.abs(r[:, 2])) & (np.abs(r[:, 1]) < QL_TINY_ANGLE * np.abs(r[:, 2]))).any())
    sheared, rotated = [], []
    for name in NAMES:
        numbers, x, cell, pbc, cvs = case(g17, name)
        out, hill = biased(cvs, numbers, x, cell, pbc)
        v = out["virial"].reshape(3, 3)
        r = ql_environment(numbers, x, cell, pbc, cvs[0][1], cvs[0][2], cvs[0][3])[2]
        if cone(r):
            # the reference's shear is tied to the z axis: it leaves a torque of the order of the shear's anisotropy, 1e-2^2 / 2,
            # in the reference's own virial too (test_twin_against_the_reference compares it) — small, and not rounding
            sheared.append(name)
            assert 1e-12 * np.abs(v).max() < np.abs(v - v.T).max() <= 1e-4 * np.abs(v).max(), name
            continue
        # r_t (x) G_t summed over an environment whose Q_l is invariant under rotation: no torque, a symmetric virial
        assert np.abs(v - v.T).max() <= 1e-13 * np.abs(v).max(), name
        if (not pbc.all() and pbc.any()) or cone(r @ R):
            continue                                                       # (a slab's open direction is tied to the cell axes)
        rot, _ = biased(cvs, numbers, x @ R, cell @ R, pbc)
        rotated.append(name)
        assert np.abs(rot["cv"] - out["cv"]).max() <= 1e-13, name
        assert np.abs(rot["forces"] - out["forces"] @ R).max() <= 1e-12 * np.abs(out["forces"]).max(), name
    assert sheared == ["si32_a5_images", "slab18_nearz"] and len(rotated) == 6, (sheared, rotated)


def test_empty_environment_is_zero_with_no_gradient():
    """g5_cluster16 atom 14 has no neighbour inside the cutoff: the reference gives NaN (0 / 0); here Q = 0 and nothing pulls."""
    from autoforce_amd.workloads import meta_bias
    g = load("g5_cluster16")
    assert np.diff(g["nl_ptr"])[14] == 0
    cvs = [("qlvar", 14, 10, 6.0, (6,))]
    out = meta_bias(cvs, 0.05, 1.0, g["numbers"], g["positions"], g["cell"], np.array([[0.02]]), pbc=g["pbc"], rc=RC)
    assert out["cv"][0] == 0.0 and out["energy"] > 0 and out["dcv"][0] != 0.0
    assert not out["forces"].any() and not out["virial"].any()


def test_two_atoms_in_a_cell_smaller_than_the_cutoff():
    """The same j under many images, and the index atom's own images: those count in Q and in the virial and pull on nobody."""
    from autoforce_amd.workloads import meta_bias, ql_environment
    numbers = np.array([14, 14])
    cell = np.array([[2.9, 0.0, 0.0], [0.3, 3.1, 0.0], [0.2, -0.4, 3.3]])
    x = np.array([[0.1, 0.2, 0.3], [1.4, 1.9, 1.2]])
    pbc = np.array([True, True, True])
    cvs = [("qlvar", 0, 14, 4.0, (4, 6))]
    jn, sh, r, ln = ql_environment(numbers, x, cell, pbc, 0, 14, 4.0)
    own = jn == 0
    assert own.sum() >= 6 and (~own).sum() >= 8 and (ln < 4.0).all()
    assert list(jn) == sorted(jn) and all(tuple(sh[t]) < tuple(sh[t + 1]) for t in range(len(jn) - 1) if jn[t] == jn[t + 1])   # (atom, image) order
    out, hill = biased(cvs, numbers, x, cell, pbc)
    F = out["forces"]
    assert np.abs(F).max() > 1e-3 and np.abs(F.sum(0)).max() <= 1e-14 * np.abs(F).max()
    # the virial by strain: it holds the own images' share, which -sum x (x) F of the two atoms cannot
    h = 1e-5
    for a, b in ((0, 0), (1, 1), (0, 2)):
        e = []
        for s in (+h, -h):
            m = np.eye(3)
            m[a, b] += s
            e.append(meta_bias(cvs, 0.05, 1.0, numbers, x @ m, cell @ m, hill[None, :], pbc=pbc, rc=RC)["energy"])
        assert abs((e[0] - e[1]) / (2 * h) - out["virial"][3 * a + b]) <= 1e-7 * np.abs(out["virial"]).max()
    raw = -(x[:, :, None] * F[:, None, :]).sum(0)
    assert np.abs(raw.reshape(9) - out["virial"]).max() > 1e-3 * np.abs(out["virial"]).max()
    # moving atom 1 alone changes the bias by F_1; moving atom 0 by F_0: the own images moved with it and did not count
    for a in (0, 1):
        for k in range(3):
            e = []
            for s in (+h, -h):
                xs = x.copy()
                xs[a, k] += s
                e.append(meta_bias(cvs, 0.05, 1.0, numbers, xs, cell, hill[None, :], pbc=pbc, rc=RC)["energy"])
            assert abs(-(e[0] - e[1]) / (2 * h) - F[a, k]) <= 1e-7 * np.abs(F).max()


def test_a_neighbour_list_object_gives_the_enumerations_bits(g17):
    """Qlvar.__call__(numbers, xyz, cell, pbc, nl): the reference's interface, get_neighbors(i) -> (indices, offsets)."""
    from autoforce_amd.meta import Qlvar
    g = load("g5_tric24")

    class NL:
        def get_neighbors(self, i):
            lo, hi = g["nl_ptr"][i], g["nl_ptr"][i + 1]
            return g["nl_j"][lo:hi], g["nl_off"][lo:hi]
    v = Qlvar(int(g["numbers"][0]), 16, index=0, cutoff=6.0, l=[4, 6])
    a = v(g["numbers"], g["positions"], g["cell"], g["pbc"], NL())
    b = v(g["numbers"], g["positions"], g["cell"], g["pbc"])
    assert np.array_equal(a, b) and np.abs(a - g17["tric24_a0_Q"]).max() <= 1e-14


def test_meta_over_a_catvar_of_qlvar_and_distance(g17, tmp_path):
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar, Qlvar
    from autoforce_amd.workloads import meta_bias, meta_cv_dim
    g = load("g5_mixed64")
    numbers, x, cell, pbc = g["numbers"], g["positions"], g["cell"], g["pbc"]
    hist = str(tmp_path / "meta.hist")
    ql = Qlvar(40, 8, cutoff=4.0, l=[4, 6])
    meta = Meta(Catvar(ql, Distance(0, 5)), sigma=0.05, w=0.02, hist=hist)
    meta.rc = RC
    assert meta.device_spec() == [("qlvar", None, 8, 4.0, (4, 6)), ("distance", 0, 5)]            # index=None until the numbers are seen
    first_zr = int(np.where(numbers == 40)[0][0])
    xs = [x, x + 0.01 * np.random.default_rng(2).normal(size=x.shape)]
    for n in range(2):
        V, F, S = meta.bias(xs[n], cell, numbers, pbc=pbc)
        meta.update()
    spec = meta.device_spec()
    assert spec == [("qlvar", first_zr, 8, 4.0, (4, 6)), ("distance", 0, 5)] and meta_cv_dim(spec) == 3
    want = meta_bias(spec, 0.05, 0.02, numbers, xs[1], cell, np.array(meta.hills[:1]), pbc=pbc, rc=RC)
    assert V == want["energy"] and np.array_equal(F, want["forces"]) and V > 0
    np.testing.assert_allclose(meta.hills[0][:2], g17["mixed64_zr_c4_Q"], rtol=1e-12)
    # meta.hist in the reference's format: the header, then one line of D values led by a blank each
    lines = open(hist).read().splitlines()
    assert lines[0] == "# 0.05" and len(lines) == 3 and all(ln.startswith(" ") and len(ln.split()) == 3 for ln in lines[1:])
    np.testing.assert_array_equal(np.loadtxt(hist, comments="#"), np.array(meta.hills))
    # refusals: a cutoff beyond the model's list, no rc at all, another species at the index, more than six dimensions, l out of range
    with pytest.raises(ValueError, match="rc"):
        Meta(Qlvar(40, 8, cutoff=6.5), hist=None).bias(x, cell, numbers, pbc=pbc, rc=RC)
    with pytest.raises(ValueError, match="rc"):
        Meta(Qlvar(40, 8, cutoff=4.0), hist=None).bias(x, cell, numbers, pbc=pbc)
    with pytest.raises(RuntimeError, match=r"numbers\[0\] != 8"):
        Meta(Qlvar(8, 8, index=0), hist=None).bias(x, cell, numbers, pbc=pbc, rc=RC)
    with pytest.raises(ValueError, match="l ="):
        Meta(Qlvar(40, 8, l=[13]), hist=None).bias(x, cell, numbers, pbc=pbc, rc=RC)
    assert Meta(Catvar(Qlvar(40, 8, l=[2, 4, 6, 8]), Posvar(0)), hist=None).device_spec() is None      # 7 dimensions
    assert Meta(Catvar(Qlvar(40, 8, l=[2, 4, 6]), Posvar(0)), hist=None).device_spec() is not None     # 6
    assert Meta(Catvar(*[Qlvar(40, 8)] * 5), hist=None).device_spec() is None                          # 5 components
    # a spec without a qlvar is what it was: no pbc, no rc, the same bits
    d = [("distance", 0, 5), ("posvar", 1, 8)]
    a = meta_bias(d, 0.1, 0.3, numbers, x, cell, np.array([[3.0, 0.1, 0.2, 0.3]]))
    b = meta_bias(d, 0.1, 0.3, numbers, x, cell, np.array([[3.0, 0.1, 0.2, 0.3]]), pbc=pbc, rc=RC)
    assert a["energy"] == b["energy"] and np.array_equal(a["forces"], b["forces"]) and np.array_equal(a["virial"], b["virial"])


def test_entry_point_is_exported_declared_and_bound():
    from autoforce_amd import SGPRModel, _lib
    lib = _lib.load()
    assert hasattr(lib, "sgpr_md_meta_ql") and "sgpr_md_meta_ql" in _lib.SIGNATURES
    assert "sgpr_md_meta_ql" in open(os.path.join(os.path.dirname(OBJ), "..", "..", "include", "sgpr_hip.h")).read()
    assert SGPRModel.META_KINDS == {"distance": 0, "posvar": 1, "qlvar": 2}


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_the_qlvar_kernels_are_forms_of_their_own_without_scratch(tmp_path):
    """The kernels of a spec without a qlvar are the instantiations they were (test_meta_twin_cpu / test_meta_merge_cpu hold their
    counts); the two new ones keep their rows' gradients in registers, not in scratch."""
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for kernel in ("md_meta_ql_kernel", "md_meta_merged_ql_kernel"):
        mine = {k: v for k, v in meta.items() if kernel in k and "private_segment_fixed_size" in v}
        assert len(mine) == 1, (kernel, sorted(mine))
        for name, md in mine.items():
            print(name, md)
            assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_count", 0) <= 256, (name, md)
