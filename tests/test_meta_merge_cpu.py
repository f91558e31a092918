"""The merged form of the metadynamics bias on the host (workloads.meta_density / meta_bias / meta_table(merge=), meta.Meta(merge=)):
against the unmerged twin within a derived bound, the rule of the table, and against the reference's own Gaussian_kde.histogram()
and Meta.energy (tests/golden/g16_meta_kde.npz, made by tests/golden/gen/make_meta_kde.py importing the reference).

  Merged against unmerged: both forms evaluate the same exp on the same arguments and every term of S is non-negative.  The
merged form replaces e + e + ... (cnt times) by cnt e — one rounding instead of cnt - 1 — and sums in another order; either sum
of H non-negative terms is within H 2^-53 S of the exact one (first order), so |S_m - S_u| <= 2 H 2^-53 S; with |t_d| < 10 inside
the neighbouring blocks the terms of A_d are bounded by 10 e, so |A_m - A_u| <= 20 H 2^-53 S.  kde = S / norm, V = w kde and
dcv_d = -w (A_d / sigma_d) / norm scale these bounds by their factors (the plain form)."""
import numpy as np
import pytest

from helpers import load

RTOL = 1e-10   # tests/test_meta_twin_cpu.py's figure against the reference (g15_meta.npz): summation order and the last bits of exp differ
EPS = 2.0 ** -53
MARGIN = 1e-6


def _hills(H, D, sg, seed=5, spread=1.2):
    return 2.0 + spread * np.asarray(sg) * np.random.default_rng(seed).normal(size=(H, D))


def _margin(c, sg):
    u, u5 = np.asarray(c) / sg, np.asarray(c) / (5.0 * sg)
    return float(min(np.min(np.minimum(u - np.floor(u), np.ceil(u) - u)), 5.0 * np.min(np.minimum(u5 - np.floor(u5), np.ceil(u5) - u5))))


@pytest.mark.parametrize("CH", [1, 8, 256, 257])
@pytest.mark.parametrize("D", [1, 3])
def test_merged_twin_against_unmerged_twin_within_the_derived_bound(CH, D):
    from autoforce_amd.workloads import meta_density
    sg = np.array([0.1, 0.15, 0.2])[:D]
    w = 1.7
    norm = np.sqrt(2.0 * np.pi) ** D
    c = np.full(D, 2.0) + 0.31 * sg
    for H in (0, 1, CH - 1, CH, CH + 1, 3 * CH, 4096):
        hills = _hills(H, D, sg)
        Vu, gu, ku = meta_density(c, sg, w, hills)
        Vm, gm, km = meta_density(c, sg, w, hills, merge=CH)
        S = ku * norm
        bS, bA = 2 * H * EPS * S, 20 * H * EPS * S
        assert abs(km - ku) <= bS / norm, (H, km, ku)
        assert abs(Vm - Vu) <= w * bS / norm, (H, Vm, Vu)
        assert np.all(np.abs(gm - gu) <= w * (bA / sg) / norm), (H, gm, gu)
        if H >= CH and H:
            assert ku > 0
        # None is the path of today: the bits of a call without the keyword
        Vn, gn, kn = meta_density(c, sg, w, hills, merge=None)
        assert (Vn, kn) == (Vu, ku) and np.array_equal(gn, gu)


def test_merge_none_keeps_the_bits_of_meta_bias_and_the_well_tempered_form_follows():
    from autoforce_amd.workloads import meta_bias
    rng = np.random.default_rng(3)
    numbers, x, cell = np.array([1, 8, 1, 8, 1]), rng.uniform(0, 4, size=(5, 3)), 6.0 * np.eye(3)
    cvs = [("posvar", 1, 1), ("distance", 0, 4)]
    c0 = meta_bias(cvs, 0.2, 1.0, numbers, x, cell, None)["cv"]
    hills = c0 + 0.25 * rng.normal(size=(600, 4))
    for tem in (None, 900.0):
        a = meta_bias(cvs, 0.2, 1.0, numbers, x, cell, hills, tem=tem)
        b = meta_bias(cvs, 0.2, 1.0, numbers, x, cell, hills, tem=tem, merge=None)
        m = meta_bias(cvs, 0.2, 1.0, numbers, x, cell, hills, tem=tem, merge=8)
        assert a["energy"] == b["energy"] and np.array_equal(a["forces"], b["forces"]) and np.array_equal(a["stress"], b["stress"])
        assert a["energy"] > 0 and abs(m["energy"] - a["energy"]) <= 1e-13 * a["energy"]
        assert np.abs(m["forces"] - a["forces"]).max() <= 1e-12 * np.abs(a["forces"]).max()
        assert np.array_equal(m["cv"], a["cv"]) and m["margin"] == a["margin"]


def test_table_rule():
    from autoforce_amd.workloads import meta_density, meta_table
    sg = np.array([0.1, 0.2])
    rng = np.random.default_rng(11)
    hills = 1.0 + 0.3 * rng.normal(size=(203, 2))
    CH = 8
    tc, tk, cnt, B = meta_table(hills, sg, CH)
    assert B == 200 and cnt.sum() == B and cnt.max() > 1 and np.all(cnt == np.round(cnt))
    # the order of first occurrence, the key of the first row
    centre = (np.floor(hills[:B] / sg) + 0.5) * sg
    seen = []
    for r in range(B):
        if not any(np.array_equal(centre[r], s) for s in seen):
            seen.append(centre[r])
            assert np.array_equal(tk[len(seen) - 1], np.floor(hills[r] / (5.0 * sg)))
    assert np.array_equal(tc, np.array(seen))
    # all rows in one bin: one entry with count B; all rows in bins of their own: B entries
    one = np.tile([[1.03, 2.07]], (19, 1)) + 1e-3 * rng.uniform(size=(19, 2))
    tc1, _, cnt1, B1 = meta_table(one, sg, 6)
    assert B1 == 18 and len(tc1) == 1 and cnt1[0] == 18.0
    own = np.stack([0.05 + 0.1 * np.arange(19), np.full(19, 0.1)], axis=1)
    tc2, _, cnt2, B2 = meta_table(own, sg, 6)
    assert B2 == 18 and len(tc2) == 18 and np.all(cnt2 == 1.0)
    assert meta_table(np.zeros((0, 2)), sg, 4)[3] == 0 and len(meta_table(None, sg, 4)[0]) == 0
    with pytest.raises(ValueError):
        meta_table(hills, sg, 0)
    # the rows fed in two uploads or in one: the table is a function of the rows — chunk after chunk it grows by appending
    c = np.array([1.02, 0.97])
    V_all = meta_density(c, sg, 1.0, hills, merge=CH)
    for cut in (8, 64, 101):
        ta = meta_table(hills[:cut], sg, CH)
        n = len(ta[0])
        assert np.array_equal(ta[0], tc[:n]) and np.array_equal(ta[1], tk[:n]) and np.all(ta[2] <= cnt[:n])
    V_two = meta_density(c, sg, 1.0, np.concatenate([hills[:101], hills[101:]]), merge=CH)
    assert V_all[0] == V_two[0] and np.array_equal(V_all[1], V_two[1]) and V_all[0] > 0


@pytest.fixture(scope="module")
def g16():
    return load("g16_meta_kde")


@pytest.mark.parametrize("name", ["k1", "k3"])
def test_table_and_energies_against_the_reference(g16, name):
    from autoforce_amd.workloads import meta_density, meta_table
    sg, dep, probes = g16[f"{name}_sigma"], g16[f"{name}_deposits"], g16[f"{name}_probes"]
    D = dep.shape[1]
    assert D == {"k1": 1, "k3": 3}[name] and len(dep) >= 300 and len(probes) >= 16
    sgv = np.broadcast_to(sg, (D,))
    # the precondition, from the reference's numbers alone: every point kept is clear of the bin and block edges
    assert min(_margin(c, sgv) for c in dep) > MARGIN and min(_margin(c, sgv) for c in probes) > MARGIN
    # the twin's table is the reference's histogram as a set, with equal counts
    hx, hw = g16[f"{name}_hist_x"], g16[f"{name}_hist_w"]
    assert hw.sum() == len(dep) and hw.max() > 1
    tc, _, cnt, B = meta_table(dep, sgv, 1)
    assert B == len(dep) and len(tc) == len(hx)
    ref = {tuple(np.floor(x / sgv).astype(int)): w for x, w in zip(hx, hw)}
    got = {tuple(np.floor(x / sgv).astype(int)): w for x, w in zip(tc, cnt)}
    assert len(ref) == len(hx) and got == ref
    np.testing.assert_allclose(sorted(map(tuple, tc)), sorted(map(tuple, hx)), rtol=1e-15)
    # energies at the probes: merged with several chunk lengths (a tail of every length class) and unmerged
    w, tem = float(g16["w"]), float(g16["tem"])
    for tag, t in (("plain", None), ("wt", tem)):
        e_ref = g16[f"{name}_energy_{tag}"]
        assert (e_ref > 0).sum() >= len(e_ref) // 2
        for merge in (None, 1, 8, 256, 257):
            for q, e in zip(probes, e_ref):
                V = meta_density(q, sgv, w, dep, tem=t, merge=merge)[0]
                assert abs(V - e) <= RTOL * abs(e), (name, tag, merge, V, e)


@pytest.mark.parametrize("tem", [None, 900.0])
def test_meta_with_merge_is_the_twin_on_its_accumulated_hills(tmp_path, tem):
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    from autoforce_amd.workloads import meta_bias, meta_table
    rng = np.random.default_rng(8)
    numbers, cell = np.array([1, 8, 1, 8, 1, 1]), 7.0 * np.eye(3)
    x0 = rng.uniform(1, 5, size=(6, 3))
    meta = Meta(Catvar(Posvar(1, select=8), Distance(0, 5)), sigma=0.1, w=0.5, tem=tem, hist=str(tmp_path / "meta.hist"), merge=4)
    plain = Meta(Catvar(Posvar(1, select=8), Distance(0, 5)), sigma=0.1, w=0.5, tem=tem, hist=None)
    assert meta.merge == 4 and plain.merge is None
    x, hills, differs = x0.copy(), [], 0
    for n in range(30):
        x = x0 + 0.05 * rng.normal(size=(6, 3))
        V, F, S = meta.bias(x, cell, numbers)
        want = meta_bias(meta.device_spec(), 0.1, 0.5, numbers, x, cell, np.array(hills), tem=tem, merge=4)
        assert V == want["energy"] and np.array_equal(F, want["forces"]) and np.array_equal(S, want["stress"])
        Vp = plain.bias(x, cell, numbers)[0]
        assert abs(V - Vp) <= 1e-13 * max(Vp, 1e-300)
        differs += V != Vp
        meta.update()
        plain.update()
        hills.append(want["cv"])
    assert V > 0 and len(meta.hills) == 30
    assert len(open(meta.hist).read().splitlines()) == 31          # the header and one line per deposit, as without merge
    hc, hn = meta.histogram()
    tc, _, cnt, B = meta_table(np.array(hills), 0.1, 4)
    assert B == 28 and np.array_equal(hc, tc) and np.array_equal(hn, cnt) and hn.sum() == 28 and hn.max() > 1
    pc, pn = plain.histogram()                                      # without merge: every hill counted
    assert pn.sum() == 30
    e = Meta(Distance(0, 1), hist=None, merge=3).histogram()
    assert e[0].shape[0] == 0 and e[1].shape == (0,)
    with pytest.raises(ValueError):
        Meta(Distance(0, 1), hist=None, merge=0)


def test_new_entry_points_are_exported_declared_and_bound():
    import os
    import re
    from autoforce_amd import SGPRModel, _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sgpr_hip.h")).read(), flags=re.S)
    for name, nargs in (("sgpr_md_meta_merge", 2), ("sgpr_md_meta_table", 5)):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/sgpr_hip.h"
        assert len(m.group(1).split(",")) == nargs and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(SGPRModel.md_meta_table)


def test_the_new_kernels_have_no_scratch_and_the_unmerged_kernel_is_still_one(tmp_path):
    import os
    from test_kernel_resources_cpu import LLVM, OBJ, _metadata
    if not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("no build objects / LLVM tools")
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    for kernel in ("md_meta_merged_kernel", "md_meta_merge_kernel", "md_meta_kernel"):
        mine = {k: v for k, v in meta.items() if kernel in k and "private_segment_fixed_size" in v}
        assert len(mine) == 1, (kernel, sorted(mine))
        for name, md in mine.items():
            assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_count", 0) <= 256, (name, md)   # (two waves per SIMD, as md_meta_kernel)
