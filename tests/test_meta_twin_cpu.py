"""Metadynamics without a GPU: workloads.meta_bias — the definition the device loop's md_meta_kernel is compared with —
against the reference's own Meta / Posvar / Catvar / Gaussian_kde (tests/golden/g15_meta.npz, made by
tests/golden/gen/make_meta.py), the block rule and Posvar's quirks, pace and meta.hist of autoforce_amd.meta.Meta, the twins'
meta= keyword, what ActiveCalculator.calculate() does with a Meta and with a plain callable, and the kernel's resources."""
import os
import re

import numpy as np
import pytest

import active_common as ac
from helpers import OracleModel, load
from test_kernel_resources_cpu import LLVM, OBJ, ROOT, _metadata

RTOL = 1e-10   # the bound of the descriptor parity tests against the reference: summation order and the last bits of exp differ


def _spec(rows):
    return [("distance", int(a), int(b)) if k == 0 else ("posvar", int(a), None if b < 0 else int(b)) for k, a, b in rows]


@pytest.fixture(scope="module")
def g15():
    return load("g15_meta")


def test_fixture_covers_the_dimensions_the_issue_names(g15):
    dims = {str(n): g15[f"{n}_cv"].shape[1] for n in g15["names"]}
    assert {dims["d1_plain"], dims["d3_plain"], dims["d4_plain"], dims["d1_wt"], dims["d3_wt"], dims["d4_wt"]} == {1, 3, 4}
    assert _spec(g15["d4_plain_spec"]) == [("posvar", 1, 8), ("distance", 0, 7)]
    assert len(g15["numbers"]) == 8 and len(set(g15["numbers"].tolist())) == 3 and len(g15["walk"]) == 200


@pytest.mark.parametrize("name", ["d1_plain", "d1_wt", "d3_plain", "d3_wt", "d4_plain", "d4_wt", "d3_vector_sigma", "d3_lonely"])
def test_meta_bias_reproduces_the_reference_walk(g15, name):
    from autoforce_amd.workloads import meta_bias
    spec, sigma = _spec(g15[f"{name}_spec"]), g15[f"{name}_sigma"]
    tem = None if np.isnan(g15[f"{name}_tem"]) else float(g15[f"{name}_tem"])
    cv_ref, e_ref, g_ref = g15[f"{name}_cv"], g15[f"{name}_energy"], g15[f"{name}_grad"]
    hills, margin, nonzero = [], np.inf, 0
    for n in range(len(cv_ref)):
        out = meta_bias(spec, sigma, float(g15["w"]), g15["numbers"], g15["walk"][n], g15["cell"], np.array(hills), tem=tem)
        margin = min(margin, out["margin"])
        np.testing.assert_allclose(out["cv"], cv_ref[n], rtol=RTOL, atol=0)
        assert abs(out["energy"] - e_ref[n]) <= RTOL * abs(e_ref[n]), (n, out["energy"], e_ref[n])
        assert np.abs(-out["forces"] - g_ref[n]).max() <= RTOL * max(np.abs(g_ref[n]).max(), 1e-300), n
        # stress: -(1/V) sum x (x) F, the reference's grads() (active.py:604-610), from these forces
        s_ref = (-(g15["walk"][n][:, :, None] * out["forces"][:, None, :]).sum(0) / abs(np.linalg.det(g15["cell"]))).reshape(9)[[0, 4, 8, 5, 2, 1]]
        assert np.abs(out["stress"] - s_ref).max() <= 1e-12 * max(np.abs(g15["walk"][n]).max() * np.abs(out["forces"]).max(), 1e-300)
        nonzero += e_ref[n] > 0
        hills.append(out["cv"])
    assert margin > 1e-9, margin        # no CV on a bin edge: the comparison means what it says
    assert nonzero > 100                # the walk does revisit its hills


def test_block_rule_one_block_away_counts_two_blocks_away_does_not():
    from autoforce_amd.workloads import meta_bias
    numbers, cell = np.array([1, 1]), np.eye(3) * 10
    x = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.04]])   # cv = 1.04: block floor(1.04 / 0.5) = 2
    for hill, counts in ((1.26, True), (0.74, True), (1.76, True), (0.49, False), (2.01, False)):
        out = meta_bias([("distance", 0, 1)], 0.1, 1.0, numbers, x, cell, np.array([[hill]]))
        centre = (np.floor(hill / 0.1) + 0.5) * 0.1
        want = np.exp(-0.5 * ((1.04 - centre) / 0.1) ** 2) / np.sqrt(2 * np.pi)
        assert abs(int(np.floor(hill / 0.5)) - 2) == {1.26: 0, 0.74: 1, 1.76: 1, 0.49: 2, 2.01: 2}[hill]
        if counts:
            assert abs(out["energy"] - want) <= 1e-15 + 1e-13 * want, hill
        else:
            assert out["energy"] == 0.0 and not out["forces"].any(), hill
    # in two dimensions and more the rule holds per dimension: one dimension two blocks away is enough
    numbers, x = np.array([1, 1, 1]), np.array([[0.0, 0.0, 0.0], [0.3, 0.2, 0.1], [0.1, 0.3, 0.2]])
    cv = meta_bias([("posvar", 0, None)], 0.1, 1.0, numbers, x, cell, None)["cv"]
    far = cv + np.array([0.0, 0.0, 1.0])
    assert meta_bias([("posvar", 0, None)], 0.1, 1.0, numbers, x, cell, np.array([far]))["energy"] == 0.0
    assert meta_bias([("posvar", 0, None)], 0.1, 1.0, numbers, x, cell, np.array([cv]))["energy"] > 0.0


def test_posvar_counts_the_index_atom_and_the_mean_of_nothing_is_zero():
    from autoforce_amd.workloads import meta_bias
    numbers, cell = np.array([3, 9, 9, 3]), np.eye(3) * 8
    x = np.arange(12.0).reshape(4, 3) * 0.37 + 1.0
    out = meta_bias([("posvar", 1, 9)], 0.1, 1.0, numbers, x, cell, None)
    np.testing.assert_allclose(out["cv"], x[1] - x[2] / 2.0, rtol=1e-15)      # n = 2: the index atom counts
    out = meta_bias([("posvar", 0, 9)], 0.1, 1.0, numbers, x, cell, None)
    np.testing.assert_allclose(out["cv"], x[0] - (x[1] + x[2]) / 2.0, rtol=1e-15)   # index outside sel: n = 2 still
    numbers = np.array([3, 9, 9, 40])
    out = meta_bias([("posvar", 3, 40)], 0.1, 1.0, numbers, x, cell, np.array([x[3]]))
    np.testing.assert_array_equal(out["cv"], x[3])                          # n = 1, the mean of nothing
    assert out["energy"] > 0 and not out["forces"][:3].any() and np.abs(out["forces"][3]).max() > 0


def test_forces_are_the_gradient_of_the_energy_and_the_margin_is_what_it_says():
    from autoforce_amd.workloads import meta_bias
    rng = np.random.default_rng(3)
    numbers, cell = np.array([1, 8, 1, 8, 8, 40, 1]), np.eye(3) * 9
    x = rng.uniform(1, 7, size=(7, 3))
    spec, sigma = [("posvar", 1, 8), ("distance", 0, 6)], np.array([0.2, 0.25, 0.3, 0.15])
    cv0 = meta_bias(spec, sigma, 1.0, numbers, x, cell, None)["cv"]
    hills = cv0 + 0.1 * rng.normal(size=(40, 4))
    for tem in (None, 500.0):
        out = meta_bias(spec, sigma, 0.02, numbers, x, cell, hills, tem=tem)
        num = np.zeros_like(x)
        for i in range(7):
            for k in range(3):
                d = np.zeros_like(x)
                d[i, k] = 1e-6
                num[i, k] = -(meta_bias(spec, sigma, 0.02, numbers, x + d, cell, hills, tem=tem)["energy"] -
                              meta_bias(spec, sigma, 0.02, numbers, x - d, cell, hills, tem=tem)["energy"]) / 2e-6
        assert np.abs(num - out["forces"]).max() < 1e-6 * np.abs(out["forces"]).max()
        # (the index atom counts in n: the bias is not translation invariant — the net force is -g / n of the posvar, the reference's quirk)
        np.testing.assert_allclose(out["forces"].sum(0), -out["dcv"][:3] / 3.0, rtol=1e-12)
    u = cv0 / sigma
    want = min(np.min(np.minimum(u - np.floor(u), np.ceil(u) - u)),
               5 * np.min(np.minimum(u / 5 - np.floor(u / 5), np.ceil(u / 5) - u / 5)))
    assert abs(out["margin"] - want) < 1e-12


def test_forces_sum_rule_of_a_dense_posvar():
    """posvar(select=None): the forces on all atoms sum to g (1/n - ... ): -g on the index atom, g / n on each of the n - 1 others."""
    from autoforce_amd.workloads import meta_bias
    rng = np.random.default_rng(5)
    N = 300   # more than one trip of 256 in the mean
    numbers, cell, x = np.ones(N, int), np.eye(3) * 20, rng.uniform(0, 20, size=(N, 3))
    cv = meta_bias([("posvar", 7, None)], 0.3, 1.0, numbers, x, cell, None)["cv"]
    np.testing.assert_allclose(cv, x[7] - (x.sum(0) - x[7]) / N, rtol=1e-13)
    out = meta_bias([("posvar", 7, None)], 0.3, 1.0, numbers, x, cell, np.array([cv + 0.2]))
    g = out["dcv"]
    np.testing.assert_allclose(out["forces"][7], -g, rtol=1e-15)
    np.testing.assert_allclose(out["forces"][8], g / N, rtol=1e-15)


def test_hill_sum_in_the_kernels_order_at_its_trip_boundaries():
    """0, 1, 255, 256, 257, 1024, 1025 hills (the kernel's strided sum takes 1024 per trip): the fixed-order sum against math.fsum."""
    import math
    from autoforce_amd.workloads import META_TRIP, meta_bias
    assert META_TRIP == 1024
    rng = np.random.default_rng(9)
    numbers, cell = np.array([1, 1]), np.eye(3) * 10
    x = np.array([[0.0, 0.0, 0.0], [0.6, 0.8, 1.2]])
    r = float(np.sqrt(0.36 + 0.64 + 1.44))
    allh = r + 0.3 * rng.normal(size=(1025, 1))
    for H in (0, 1, 255, 256, 257, 1024, 1025):
        out = meta_bias([("distance", 0, 1)], 0.1, 0.5, numbers, x, cell, allh[:H])
        cvv = out["cv"][0]
        terms = [math.exp(-0.5 * ((cvv - (math.floor(h / 0.1) + 0.5) * 0.1) / 0.1) ** 2) for h in allh[:H, 0]
                 if abs(math.floor(h / 0.5) - math.floor(cvv / 0.5)) <= 1]
        want = 0.5 * math.fsum(terms) / math.sqrt(2 * math.pi)
        assert abs(out["energy"] - want) <= 1e-13 * max(want, 1e-300), H


def test_pace_and_the_hist_file_in_the_references_format(g15, tmp_path):
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    hist = str(tmp_path / "meta.hist")
    meta = Meta(Catvar(Posvar(1, select=8), Distance(0, 7)), sigma=0.1, w=0.013, hist=hist)
    assert meta.device_spec() == [("posvar", 1, 8), ("distance", 0, 7)]
    for n in range(3):
        meta.bias(g15["walk"][n], g15["cell"], g15["numbers"])
        meta.update()
    got = open(hist).read()
    ref = str(g15["hist_text"])
    assert got.splitlines()[0] == ref.splitlines()[0] == "# 0.1"
    assert len(got.splitlines()) == len(ref.splitlines()) == 4
    for a, b in zip(got.splitlines()[1:], ref.splitlines()[1:]):
        assert a.startswith(" ") and len(a.split()) == len(b.split()) == 4
        np.testing.assert_allclose([float(t) for t in a.split()], [float(t) for t in b.split()], rtol=RTOL)
    # the lines are the CVs of the fixture, written with repr precision: they read back exactly
    np.testing.assert_array_equal(np.loadtxt(hist, comments="#"), np.array(meta.hills))
    # pace = 3 deposits the configurations 0, 3, 6, ...
    m3 = Meta(Distance(0, 5), sigma=0.1, w=0.013, pace=3, hist=str(tmp_path / "m3.hist"))
    for n in range(10):
        m3.bias(g15["walk"][n], g15["cell"], g15["numbers"])
        m3.update()
    np.testing.assert_allclose(np.array(m3.hills)[:, 0], g15["d1_plain_cv"][[0, 3, 6, 9], 0], rtol=RTOL)
    assert len(open(str(tmp_path / "m3.hist")).read().splitlines()) == 1 + 4
    # a colvar that is not built in has no device form
    assert Meta(lambda numbers, xyz, cell, pbc, nl: xyz[1] - xyz[0], hist=None).device_spec() is None
    assert Meta(Catvar(Posvar(0), Posvar(1), Posvar(2)), hist=None).device_spec() is None   # 9 dimensions


@pytest.mark.parametrize("loop", ["langevin", "nose_hoover"])
def test_twins_with_meta_add_the_bias_by_evaluation_index(loop, tmp_path):
    """The loop with meta= sees, at every configuration, exactly the calculator's forces plus meta_bias of the hills of the
    configurations before it, and without meta= it is the loop it was."""
    import autoforce_amd.workloads as wl
    from autoforce_amd.meta import Distance, Meta
    from helpers import PairTeacher
    rng, numbers, pos, cell = ac.start(0)
    seen = []

    class Spy(PairTeacher):
        def calculate(self, atoms=None, *a, **k):
            super().calculate(atoms, *a, **k)
            seen.append(np.array(atoms.positions))

    fn = wl.langevin_nvt if loop == "langevin" else wl.nose_hoover_nvt
    meta = Meta(Distance(0, 1), sigma=0.05, w=0.5, pace=2, hist=str(tmp_path / "h"))
    rows = list(fn(Spy(rc=4.0), numbers, pos, cell, True, 6, temperature=300.0, seed=4, meta=meta))
    assert len(rows) == 7 and len(meta.hills) == 4            # configurations 0, 2, 4, 6
    hills = []
    plain = PairTeacher(rc=4.0)
    from autoforce_amd.ase_shim import Atoms
    for n, (row, x) in enumerate(zip(rows, seen)):
        at = Atoms(numbers, x, cell, True)
        at.calc = plain
        e0 = at.get_potential_energy()
        b = wl.meta_bias([("distance", 0, 1)], 0.05, 0.5, numbers, x, cell, np.array(hills))
        assert row[1] == e0 + b["energy"]
        if n % 2 == 0:
            hills.append(b["cv"])
    assert sum(r[1] for r in rows) != sum(r[1] for r in fn(PairTeacher(rc=4.0), numbers, pos, cell, True, 6, temperature=300.0, seed=4))


def test_calculate_adds_the_bias_of_a_meta_and_only_logs_a_plain_callable(tmp_path):
    from autoforce_amd.ase_shim import Atoms
    from autoforce_amd.meta import Catvar, Distance, Meta, Posvar
    (tmp_path / "plain").mkdir()
    calc, teacher, trace = ac.run(OracleModel(3, 3, 4, 4.5, species=ac.SPECIES), tmp_path / "plain", steps=3, tape=False)
    at = trace[-1][-1]
    calc._calc = None   # (evaluate only: the model stays as it is)
    from oracle import oracle as orc
    orc.set_num_threads(1)   # (a fixed summation order in the oracle: two evaluations of one configuration give the same bits)
    def evaluate():   # (calculate() itself: the atoms' cache would answer for an unchanged configuration)
        calc.results = {}
        calc.calculate(Atoms(at.numbers, at.positions, at.cell, True))
        return {k: np.array(calc.results[k]) for k in ("energy", "forces", "stress")}
    base = evaluate()
    # a plain callable: logged, nothing added (today's behaviour)
    calls = []
    calc.meta = lambda c: (calls.append(1) or np.array([0.125]), {"op": "+=", "is_meta": True})
    got = evaluate()
    assert calls and all(np.array_equal(got[k], base[k]) for k in base)
    assert "meta: 0.125" in open(str(tmp_path / "plain" / "active.log")).read()
    # a Meta with hills: results = model + bias
    meta = Meta(Catvar(Posvar(2, select=3), Distance(0, 5)), sigma=0.3, w=0.05, tem=700.0, hist=str(tmp_path / "meta.hist"))
    cv0 = meta.colvar(at.numbers, at.positions)
    meta.hills = [cv0 + 0.1, cv0 - 0.05]
    V, Fb, Sb = meta.bias(at.positions, at.cell, at.numbers)
    assert V > 0 and np.abs(Fb).max() > 0
    calc.meta = meta
    got = evaluate()
    assert got["energy"] == base["energy"] + V
    np.testing.assert_array_equal(got["forces"], base["forces"] + Fb)
    np.testing.assert_array_equal(got["stress"], base["stress"] + Sb)
    assert f"meta: {V}" in open(str(tmp_path / "plain" / "active.log")).read()
    assert len(meta.hills) == 2        # calculate() deposits nothing: the dynamics do (dyn.attach(meta.update))
    # a colvar that is not built in, the reference's interface: the bias acts through autograd and equals the built-in's
    custom = Meta(lambda numbers, xyz, cell, pbc, nl: (xyz[5] - xyz[0]).norm().view(1), sigma=0.3, w=0.05, hist=None)
    builtin = Meta(Distance(0, 5), sigma=0.3, w=0.05, hist=None)
    custom.hills = builtin.hills = [np.array([cv0[3] + 0.1])]
    Vc, Fc, Sc = custom.bias(at.positions, at.cell, at.numbers)
    Vb, Fb2, Sb2 = builtin.bias(at.positions, at.cell, at.numbers)
    assert abs(Vc - Vb) <= 1e-14 * Vb and np.abs(Fc - Fb2).max() <= 1e-13 * np.abs(Fb2).max()
    assert np.abs(Sc - Sb2).max() <= 1e-12 * np.abs(at.positions).max() * np.abs(Fb2).max()
    assert calc._meta_spec() is None                    # the oracle engine has no md_meta: the host loop
    orc.set_num_threads(os.cpu_count() or 1)


def test_entry_points_are_exported_declared_and_bound():
    from autoforce_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "sgpr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("sgpr_md_meta", 11), ("sgpr_md_meta_info", 5), ("sgpr_md_meta_hills", 5)):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/sgpr_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
    from autoforce_amd import SGPRModel
    for name in ("md_meta", "md_meta_hills", "md_meta_info"):
        assert callable(getattr(SGPRModel, name))


@pytest.mark.skipif(not (os.path.isfile(os.path.join(OBJ, "api.o")) and os.path.isfile(os.path.join(LLVM, "llvm-readelf"))),
                    reason="no build objects / LLVM tools")
def test_meta_kernel_has_no_scratch_and_the_last_kernels_are_untouched(tmp_path):
    meta = _metadata(os.path.join(OBJ, "api.o"), str(tmp_path))
    mine = {k: v for k, v in meta.items() if "md_meta_kernel" in k and "private_segment_fixed_size" in v}
    assert len(mine) == 1, sorted(meta)[:20]
    for name, md in mine.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md.get("vgpr_count", 0) <= 256, (name, md)      # (two waves per SIMD of 512 registers: the launch is ceil(N / 256) workgroups, DESIGN section 3: 178)
    assert len([k for k in meta if "finalize_next_kernel" in k]) == 7    # no new instantiation of the step's last kernel
