"""GPU tests of the neighbour-list / descriptor path at EXACT list lengths, in every compiled form, each against the CPU
oracle on identical inputs.  The frames are the islands of islands.py: every atom of an island of n atoms has exactly n - 1
neighbours (test_islands_cpu.py proves, with the oracle alone, every length and candidate count named below).

(a) every (lmax, nmax, species-slot) instantiation on frame A — lists of exactly 47|48|49 (the rows whose virial / own-force
    sums are added first), 63|64|65 (one tile of 64 or two, register sort or LDS sort) and 127|128|129 (two tiles or three)
    mixed inside the workgroups;
(b) the sharded (scatter) form of the reverse pass and the training rows on the same frame, in four forms;
(c) the training rows where the sixteen-column form hands over to the one-column form: longest list 63, 64, 65;
(d) reuse steps (candidates kept, hits filtered) with 63 ... 129 candidates and fewer hits than candidates;
(e) lists of 255|256|257 around the sortable part of a candidate list;
(f) the device MD loop with lmax != 3 and with more than eight species slots, lists of 48, 64 and 128.

Tolerances are the project's own: compare() of test_hip_paths.py (K_mm, cov 1e-9, energy 1e-9, forces and stress 1e-8 of the
largest component, beta 3e-6, the covloss bound), descriptors at 1e-10 / 1e-13 as in test_hip_tile64.py, rows as in
test_hip_rows.py.  None of them needed widening at rc = 10 with 129-neighbour lists: the oracle's own outputs on frame A move
by 5e-15 of the largest force, 8e-14 of the largest stress and 2.5e-4 of the descriptor tolerance when every atom's
neighbour order is permuted (ten permutations; (3,3) with 3 and 12 species, (4,4) with 6), and the library sits at most
1e-13 of the largest force from it."""
import numpy as np
import pytest

import islands
from islands import A, B, SHELL, SPECIES

pytestmark = pytest.mark.gpu

ETA, M = 4.0, 24
ROUTE16, ROUTE1 = "sixteen columns per workgroup pass", "one column per wave"


def make_model(lmax, nmax, species, frame, rc, seed=2):
    from autoforce_amd import SGPRModel
    numbers, pos, cell, pbc, _ = frame
    mdl = SGPRModel(lmax, nmax, ETA, rc, species=species)
    mdl.set_inducing(islands.inducing(numbers, pos, cell, pbc, rc, M, seed))
    return mdl


def oracle_model(mdl, rc):
    """ind_z, nnm, Pm, choli of the model's inducing set, by the oracle; mu as compare() draws it."""
    from oracle import oracle as orc
    ind_z, ind_ptr, bz, br = islands.inducing_arrays(mdl.X)
    Pm, nnm = orc.inducing_descriptors(mdl.lmax, mdl.nmax, rc, mdl.species, ind_z, ind_ptr, bz, br)
    L, _ = orc.jitcholesky(orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, ETA))
    return ind_z, nnm, Pm, orc.tril_inverse(L), np.random.default_rng(9).normal(size=len(mdl.X))


def by_length(err, nn):
    """Largest entry of a per-atom error for every list length, as text: a failure names the edge it came from."""
    err = np.asarray(err).reshape(len(nn), -1).max(axis=1)
    return ", ".join(f"nn={k}: {err[nn == k].max():.2e}" for k in np.unique(nn))


def check_frame(out, ref, nn, label, desc=None):
    """The frame checks of test_hip_paths.compare (same tolerances) with the errors grouped by list length in the message;
    prints every figure before it asserts."""
    fmax, smax = np.abs(ref["forces"]).max(), max(np.abs(ref["stress"]).max(), 1e-12)
    ferr = np.abs(out["forces"] - ref["forces"])
    cerr = np.abs(out["cov"] - ref["cov"]) / (1e-9 * np.abs(ref["cov"]) + 1e-12)
    berr = np.abs(out["beta"] - ref["beta"])
    serr = np.abs(out["stress"] - ref["stress"]).max()
    eerr = abs(out["energy"] - ref["energy"])
    msg = (f"{label}: forces / (1e-8 fmax) {ferr.max() / (1e-8 * fmax):.3g} [{by_length(ferr / fmax, nn)}]; cov / tol {cerr.max():.3g} "
           f"[{by_length(cerr, nn)}]; beta {berr.max():.2e} [{by_length(berr, nn)}]; stress / (1e-8 smax) {serr / (1e-8 * smax):.3g}; "
           f"energy / tol {eerr / (1e-9 * max(1.0, abs(ref['energy']))):.3g}")
    if desc is not None:
        derr = np.abs(desc - ref["p"]).reshape(len(nn), -1) / (1e-10 * np.abs(ref["p"]).reshape(len(nn), -1) + 1e-13)
        msg += f"; descriptors / tol {derr.max():.3g} [{by_length(derr, nn)}]"
    print(msg)
    assert ferr.max() <= 1e-8 * fmax, msg
    assert cerr.max() <= 1.0, msg
    assert eerr <= 1e-9 * max(1.0, abs(ref["energy"])), msg
    assert serr <= 1e-8 * smax, msg
    assert berr.max() <= 3e-6, msg
    if desc is not None:
        assert derr.max() <= 1.0, msg


def pair_set(ptr, j, off):
    i = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return set(map(tuple, np.column_stack([i, j, off]).tolist()))


def ascending(mdl, numbers, ptr, j, off, limit=256):
    """Atoms whose list is not strictly ascending by (j, image) within its first `limit` entries.  j counts in the device's
    order — atoms sorted by species slot, then by caller index — and the image triple compares component by component."""
    slot = np.array([mdl.species.index(int(z)) for z in numbers])
    key = np.column_stack([slot[j], j, off]).astype(np.int64) + np.array([0, 0, 128, 128, 128])
    key = (((key[:, 0] * (1 << 24) + key[:, 1]) * 256 + key[:, 2]) * 256 + key[:, 3]) * 256 + key[:, 4]
    bad = []
    for a in range(len(ptr) - 1):
        k = key[ptr[a]:min(ptr[a + 1], ptr[a] + limit)]
        if np.any(np.diff(k) <= 0):
            bad.append(a)
    return bad


# ------------------------------------------------------------------ (a) every compiled form on frame A
@pytest.mark.parametrize("lmax,nmax,nspec", islands.FORMS)
def test_every_compiled_form_on_frame_a(lmax, nmax, nspec, monkeypatch):
    """One case per instantiation the dispatch can select.  The reference of a case is computed once: compare() calls
    oracle.frame, and the result is kept for the checks compare() does not make (descriptors, island sums, the grouping)."""
    from oracle import oracle as orc
    from test_hip_paths import compare
    species = SPECIES[:nspec]
    frame = numbers, pos, cell, pbc, isl = islands.frame_a(species)
    rc, N = A["rc"], len(numbers)
    nl = orc.neighbors_cells(pos, cell, pbc, rc)
    mdl = make_model(lmax, nmax, species, frame, rc)
    kept, real = {}, orc.frame
    monkeypatch.setattr(orc, "frame", lambda *a, **k: kept.setdefault("ref", real(*a, **k)))
    label = f"({lmax},{nmax}) {nspec} species"
    try:
        out = compare(mdl, lmax, nmax, ETA, rc, numbers, pos, cell, pbc, nl)
    except AssertionError as e:
        if "ref" in kept:   # name the list lengths the error sits at (check_frame asserts the same bounds)
            check_frame(mdl.predict(numbers, pos, cell, pbc, cov=True), kept["ref"], np.diff(nl[0]), label)
        raise e
    ref = kept["ref"]
    ptr, j, off = mdl.neighbors(N)
    nn = np.diff(ptr)
    assert sorted(set(nn.tolist())) == [47, 48, 49, 63, 64, 65, 127, 128, 129]
    assert np.array_equal(nn, np.diff(nl[0]))
    assert pair_set(ptr, j, off) == pair_set(*nl)        # (compare() has asserted it: kept beside the order check)
    assert ascending(mdl, numbers, ptr, j, off) == []
    check_frame(out, ref, nn, label, desc=mdl.descriptors(N))
    fmax = np.abs(out["forces"]).max()
    sums = np.array([np.abs(out["forces"][isl == k].sum(0)).max() for k in range(isl.max() + 1)])
    assert np.all(sums <= 1e-10 * fmax), (label, dict(zip(islands.A_SIZES, (sums / fmax).tolist())))
    mdl.close()


# ------------------------------------------------------------------ (b) sharded scatter form, training rows
@pytest.mark.parametrize("lmax,nmax,nspec", islands.SPREAD_FORMS)
def test_sharded_scatter_form_and_training_rows_on_frame_a(lmax, nmax, nspec):
    """World 2: every rank's reverse pass scatters with atomics; the partial sums equal the whole, compared as
    test_hip_parity.test_sharded_partials_sum_to_the_whole compares (the whole is the oracle's: case (a)).  Then the training
    rows of the frame — the one-column form, lists being longer than 64 — against oracle.kernel_rows."""
    from oracle import oracle as orc
    species = SPECIES[:nspec]
    frame = numbers, pos, cell, pbc, isl = islands.frame_a(species)
    rc = A["rc"]
    mdl = make_model(lmax, nmax, species, frame, rc)
    ind_z, nnm, Pm, choli, mu = oracle_model(mdl, rc)
    mdl.set_weights(mu, choli=choli)
    whole = mdl.predict(numbers, pos, cell, pbc, cov=True)
    nn = np.diff(mdl.neighbors(len(numbers))[0])     # (before the sharded calls: a rank reports its own atoms' lists only)
    assert sorted(set(nn.tolist())) == [47, 48, 49, 63, 64, 65, 127, 128, 129]
    acc = None
    for r in range(2):
        part = mdl.predict(numbers, pos, cell, pbc, rank=r, world=2, cov=True)
        acc = {k: np.array(v, dtype=float) for k, v in part.items()} if acc is None else {k: acc[k] + part[k] for k in acc}
    assert abs(acc["energy"] - whole["energy"]) <= 1e-12 * max(1.0, abs(whole["energy"]))
    for k in ("forces", "stress", "beta", "cov"):
        err = np.abs(acc[k] - whole[k])
        assert err.max() <= 1e-12 * max(1.0, np.abs(whole[k]).max()), (k, by_length(err, nn) if k != "stress" else err.max())
    Ke, Kf, Kv = mdl.kernel_rows(numbers, pos, cell, pbc)
    assert mdl.solve_info().split("rows=")[1] == ROUTE1
    nl = orc.neighbors_cells(pos, cell, pbc, rc)
    oe, of, ov = orc.kernel_rows(lmax, nmax, rc, ETA, np.array(species, np.int32), numbers, pos, cell, nl, ind_z, nnm, Pm)
    ferr = np.abs(Kf - of).reshape(len(numbers), -1)
    print(f"rows ({lmax},{nmax}) {nspec} species: Kf / (1e-9 max) {ferr.max() / (1e-9 * np.abs(of).max()):.3g} [{by_length(ferr / np.abs(of).max(), nn)}]; "
          f"Kv / (1e-9 max) {np.abs(Kv - ov).max() / (1e-9 * np.abs(ov).max()):.3g}")
    np.testing.assert_allclose(Ke, oe, rtol=1e-11, atol=1e-13)
    assert ferr.max() <= 1e-9 * np.abs(of).max(), by_length(ferr / np.abs(of).max(), nn)
    assert np.abs(Kv - ov).max() <= 1e-9 * np.abs(ov).max()
    mdl.close()


# ------------------------------------------------------------------ (c) the rows16 edge
@pytest.mark.parametrize("nspec", [1, 2, 3])
@pytest.mark.parametrize("sizes", islands.ROWS16_SIZES)
def test_rows_forms_where_the_longest_list_is_63_64_65(sizes, nspec, monkeypatch):
    """The sixteen-column form takes frames whose longest list is at most 64 (its gnn rows are as long as the longest list);
    at 65 the call goes to the one-column form.  One, two and three species: the three instantiations of its finalize
    kernel.  Both forms against the oracle at the tolerances of test_hip_rows.py, and against each other at 1e-12."""
    from oracle import oracle as orc
    species = SPECIES[:nspec]
    frame = numbers, pos, cell, pbc, isl = islands.frame_a(species, sizes)
    rc = A["rc"]
    nl = orc.neighbors_cells(pos, cell, pbc, rc)
    longest = int(np.diff(nl[0]).max())
    assert longest == len(sizes) + 60
    got = {}
    for form in ("1", "0"):
        monkeypatch.setenv("SGPR_ROWS16", form)
        mdl = make_model(3, 3, species, frame, rc)
        got[form] = mdl.kernel_rows(numbers, pos, cell, pbc)
        assert mdl.solve_info().split("rows=")[1] == (ROUTE16 if form == "1" and longest <= 64 else ROUTE1), (form, longest)
        assert int(np.diff(mdl.neighbors(len(numbers))[0]).max()) == longest
        if form == "1":
            ind_z, nnm, Pm, _, _ = oracle_model(mdl, rc)
        mdl.close()
    want = orc.kernel_rows(3, 3, rc, ETA, np.array(species, np.int32), numbers, pos, cell, nl, ind_z, nnm, Pm)
    nn = np.diff(nl[0])
    for form in ("1", "0"):
        Ke, Kf, Kv = got[form]
        ferr = np.abs(Kf - want[1]).reshape(len(numbers), -1) / np.abs(want[1]).max()
        print(f"SGPR_ROWS16={form} longest {longest}, {nspec} species: Kf / 1e-9 {ferr.max() / 1e-9:.3g} [{by_length(ferr, nn)}]")
        np.testing.assert_allclose(Ke, want[0], rtol=1e-11, atol=1e-13)
        assert ferr.max() <= 1e-9, (form, by_length(ferr, nn))
        assert np.abs(Kv - want[2]).max() <= 1e-9 * np.abs(want[2]).max(), form
    for a, b in zip(got["1"], got["0"]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


# ------------------------------------------------------------------ (d) candidate edges on reuse steps
def test_reuse_steps_with_63_to_129_candidates_and_fewer_hits():
    """Shell islands: 63, 64, 65, 127, 128, 129 candidates per atom, of which up to eight are not hits and change from step
    to step — one, two or three words of hit mask, the last of them partly filled, lists of one tile from candidate rows of
    two.  A handle with the default skin (candidates kept over the walk, rebuilt once when an atom is carried through the
    cell) against one with skin 0 (rebuilt every step): bit for bit, lists included; first and last step against the oracle."""
    from autoforce_amd import _lib
    from oracle import oracle as orc
    species = SPECIES[:3]
    frame = numbers, pos, cell, pbc, isl = islands.shell_frame(species)
    rc, N = SHELL["rc"], len(numbers)
    fast, slow = make_model(3, 3, species, frame, rc), make_model(3, 3, species, frame, rc)
    _lib.check(_lib.load().sgpr_set_option(slow.handle, b"skin_milliangstrom", 0))
    ind_z, nnm, Pm, choli, mu = oracle_model(fast, rc)
    fast.set_weights(mu, choli=choli)
    slow.set_weights(mu, choli=choli)
    walk = islands.shell_walk(pos, cell)
    lengths = set()
    for step, p in enumerate(walk):
        a = fast.predict(numbers, p, cell, pbc, cov=True)
        b = slow.predict(numbers, p, cell, pbc, cov=True)
        if step == 0:
            r0 = fast.list_rebuilds(), slow.list_rebuilds()
        for k in ("energy", "forces", "stress", "beta", "cov"):
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"step {step}: {k}")
        la, lb = fast.neighbors(N), slow.neighbors(N)
        for x, y in zip(la, lb):
            np.testing.assert_array_equal(x, y, err_msg=f"step {step}: lists")
        lengths |= set(np.diff(la[0]).tolist())
        if step in (0, len(walk) - 1):
            nl = orc.neighbors_cells(p, cell, pbc, rc)
            assert pair_set(*la) == pair_set(*nl)
            assert ascending(fast, numbers, *la) == []
            ref = orc.frame(3, 3, rc, ETA, species, numbers, p, cell, nl, ind_z, nnm, Pm, mu, choli=choli, want_p=False)
            check_frame(a, ref, np.diff(nl[0]), f"shell step {step}")
    assert {63, 64, 65} <= lengths and max(lengths) <= 129 and min(lengths) < 63
    assert fast.list_rebuilds() - r0[0] == 1, (r0, fast.list_rebuilds())           # the atom carried through the cell, nothing else
    assert slow.list_rebuilds() - r0[1] >= len(walk) - 1
    fast.close(); slow.close()


# ------------------------------------------------------------------ (e) the sort limit
def test_lists_of_255_256_257_around_the_sortable_part():
    """Frame B: the first 256 candidates of an atom are sorted by (j, image), what follows keeps the order of the sweep,
    which depends on where atomics placed the atoms in their bins.  Lists of 255 and 256 are ascending throughout, of 257
    in their first 256 entries; every output against the oracle; two fresh handles give the same bits for the atoms whose
    list fits the sortable part."""
    from oracle import oracle as orc
    species = SPECIES[:3]
    frame = numbers, pos, cell, pbc, isl = islands.frame_b(species)
    rc, N = B["rc"], len(numbers)
    nl = orc.neighbors_cells(pos, cell, pbc, rc)
    outs = []
    for k in range(2):
        mdl = make_model(3, 3, species, frame, rc)
        if k == 0:
            ind_z, nnm, Pm, choli, mu = oracle_model(mdl, rc)
        mdl.set_weights(mu, choli=choli)
        out = mdl.predict(numbers, pos, cell, pbc, cov=True)
        ptr, j, off = mdl.neighbors(N)
        nn = np.diff(ptr)
        assert sorted(set(nn.tolist())) == [255, 256, 257] and np.array_equal(nn, np.diff(nl[0]))
        assert pair_set(ptr, j, off) == pair_set(*nl)
        assert ascending(mdl, numbers, ptr, j, off, limit=256) == []
        if k == 0:
            ref = orc.frame(3, 3, rc, ETA, species, numbers, pos, cell, nl, ind_z, nnm, Pm, mu, choli=choli)
            check_frame(out, ref, nn, "frame B", desc=mdl.descriptors(N))
            fmax = np.abs(out["forces"]).max()
            for i in range(3):
                assert np.abs(out["forces"][isl == i].sum(0)).max() <= 1e-10 * fmax, i
        outs.append((out, (ptr, j, off)))
        mdl.close()
    fits = nn <= 256
    for key in ("forces", "beta", "cov"):
        assert np.array_equal(outs[0][0][key][fits], outs[1][0][key][fits]), key
    pa, ja, oa = outs[0][1]
    pb, jb, ob = outs[1][1]
    for a in np.flatnonzero(fits):
        assert np.array_equal(ja[pa[a]:pa[a + 1]], jb[pb[a]:pb[a + 1]]) and np.array_equal(oa[pa[a]:pa[a + 1]], ob[pb[a]:pb[a + 1]])


# ------------------------------------------------------------------ (f) the device MD loop beyond (3, 3, <= 4 slots)
@pytest.mark.parametrize("lmax,nmax,nspec", islands.MD_FORMS)
def test_device_langevin_on_islands_bit_for_bit(lmax, nmax, nspec):
    """Twelve steps of langevin_nvt_device on islands of 49, 65 and 129 atoms (lists of 48, 64 and 128: the last kernel sums
    G[Nall][maxnn][4] with maxnn of two tiles) against langevin_nvt around the same library, as
    test_hip_tile64.test_device_langevin_with_lists_of_49_to_64_bit_for_bit compares."""
    from autoforce_amd.workloads import langevin_nvt, langevin_nvt_device
    from test_hip_tile64 import _PredictCalc
    species = SPECIES[:nspec]
    frame = numbers, pos, cell, pbc, isl = islands.frame_a(species, islands.MD_SIZES)
    mdl = make_model(lmax, nmax, species, frame, A["rc"])
    rng = np.random.default_rng(2)
    mdl.solve(rng.normal(size=(64, M)), rng.normal(size=64))
    mdl.set_weights(0.02 * rng.normal(size=M), choli=mdl.choli, vscale=mdl.make_vscale())
    steps = 12
    calc = _PredictCalc(mdl)
    host = [(s, E, T, w, p.copy(), v.copy()) for s, E, T, w, p, v in
            langevin_nvt(calc, numbers, pos, cell, pbc, steps, temperature=1200.0, dt_fs=1.0, friction=0.05, seed=3)]
    assert set(calc.nn[0].tolist()) == {48, 64, 128}
    r0 = mdl.list_rebuilds()
    dev = list(langevin_nvt_device(mdl, numbers, pos, cell, pbc, steps, temperature=1200.0, dt_fs=1.0, friction=0.05, seed=3, chunk=16))
    assert mdl.list_rebuilds() - r0 >= 1
    assert len(dev) == len(host) == steps + 1
    for (s0, E0, T0, _, _, _), (s1, E1, T1, bmax), b0 in zip(host, dev, calc.betas):
        assert s0 == s1
        assert E0 == E1, (s0, E0, E1)
        assert abs(T0 - T1) <= 1e-12 * T0
        assert bmax == b0
    st = mdl.md_state(results=True)
    assert np.array_equal(st["positions"], host[-1][4])
    assert np.array_equal(st["velocities"], host[-1][5])
    mdl.close()
