"""The three GEMMs of a step (K_nm, W = Aw.Pm, covloss) where their tile tables change: species block edges against 16-,
32- and 64-row tile edges, inducing blocks against 64-column tile edges, every tile form, both sides of every automatic
switch, choli shapes, one handle over a sequence of frames and inducing edits, sharded shares.  Every result is checked
against the host references of tests/step_ref.py, computed from the device's own descriptors, never against another form:

  K_nm   within the bound of its dot product; cross-species entries exactly zero;
  E      within the bound of sum K mu + sum mean_w;
  c      = 1 - beta^2 (vscale = 1, choli scaled so that max c = 0.9) within the bound of sum_a (choli K)^2 + 4 eps;
  F, virial against the oracle (oracle.frame) at 1e-8 of their largest entry.

sgpr_solve_info's "step=" field names the form each case took; the tests assert it."""
import numpy as np
import pytest

import step_ref as ref

pytestmark = pytest.mark.gpu

SPECIES16 = [1, 6, 7, 8, 16, 3, 9, 15, 11, 12, 13, 14, 17, 19, 20, 29]
RC, ETA = 5.0, 4.0
GHOST_Z = 79


def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------- frames and models
def lattice(n, seed, a=2.3):
    """n atoms on distinct sites of a jittered simple-cubic lattice (periodic cube)."""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(n ** (1 / 3)))
    while g ** 3 < n:
        g += 1
    sites = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = (sites[rng.choice(len(sites), n, replace=False)] + 0.15 * rng.normal(size=(n, 3))) * a
    return pos, np.eye(3) * g * a


def frame(species, counts, seed, ghosts=0):
    """Exactly counts[s] atoms of species[s] (and `ghosts` atoms outside the table), in shuffled order."""
    rng = np.random.default_rng(seed + 7)
    numbers = np.concatenate([np.full(c, z) for z, c in zip(species, counts)] + [np.full(ghosts, GHOST_Z)]).astype(np.int32)
    rng.shuffle(numbers)
    pos, cell = lattice(len(numbers), seed)
    return numbers, pos, cell, [True] * 3


def inducing(species, counts, seed):
    """counts[s] LCEs of central species species[s], each the (perturbed) environment of a distinct atom of a pool frame."""
    from autoforce_amd import Local
    from oracle import oracle as orc
    total = int(sum(counts))
    rng = np.random.default_rng(seed + 11)
    pnum = rng.choice(species, size=total + 8).astype(np.int32)
    pos, cell = lattice(total + 8, seed + 1)
    ptr, j, off = orc.neighbors(pos, cell, [True] * 3, RC)
    X, k = [], 0
    for z, c in zip(species, counts):
        for _ in range(c):
            s = slice(ptr[k], ptr[k + 1])
            r = pos[j[s]] - pos[k] + off[s].astype(float) @ cell + 0.03 * rng.normal(size=(ptr[k + 1] - ptr[k], 3))
            keep = np.linalg.norm(r, axis=1) < RC - 1e-3
            X.append(Local(int(z), pnum[j[s]][keep], r[keep]))
            k += 1
    return X


def model(species, ind_counts, seed=0, ghosts=False, eta=ETA):
    from autoforce_amd import SGPRModel
    mdl = SGPRModel(3, 3, eta, RC, species=species, unknown_species="ignore" if ghosts else "error")
    mdl.set_inducing(inducing(species, ind_counts, seed))
    return mdl


def slots_of(species, numbers):
    idx = {z: s for s, z in enumerate(species)}
    return np.array([idx.get(int(z), -1) for z in numbers])


def weights(mdl, seed=3, general=False):
    """mu, mean, choli = alpha L^-1 (per species block of K_mm; upper entries inside the blocks when `general`), with
    alpha set on the next frame (install)."""
    rng = np.random.default_rng(seed)
    m = mdl.m
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    M = mdl.M
    C = np.zeros((m, m))
    for s in np.unique(zq):
        q = np.flatnonzero(zq == s)
        B = M[np.ix_(q, q)]
        L = np.linalg.cholesky(B + 1e-6 * np.mean(np.diag(B)) * np.eye(len(q)))
        Ci = np.linalg.inv(L)
        if general and len(q) > 1:
            Ci = Ci + np.triu(0.05 * rng.normal(size=Ci.shape) * np.abs(Ci).max(), 1)
        C[np.ix_(q, q)] = Ci
    mu = rng.normal(size=m)
    mean = {z: 0.01 * (k + 1) for k, z in enumerate(mdl.species)}
    return mu, mean, C


def install(mdl, mu, mean, C, alpha=1.0):
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    vs = {z: 1.0 for s, z in enumerate(mdl.species) if np.any(zq == s)}   # (no inducing LCE: +inf, the header's rule)
    mdl.set_weights(mu, mean=mean, vscale=vs, choli=alpha * C)


def step_form(mdl):
    return mdl.solve_info().split("step=")[1].split(";")[0]


# ---------------------------------------------------------------------------------------------- the check
def check(mdl, fr, mu, mean, C, what="", rank_world=None, view=False, oracle=True, eta=ETA):
    """Predict `fr` on `mdl` (weights mu / mean / C installed here, C rescaled so that max c = 0.9) and check every
    output against the references (eta: the exponent `mdl` was created with).  Returns the device output."""
    numbers, pos, cell, pbc = fr
    N = len(numbers)
    install(mdl, mu, mean, C)
    out = mdl.predict(numbers, pos, cell, pbc, cov=True)
    zi = slots_of(mdl.species, numbers)
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    P = mdl.descriptors(N).reshape(N, -1)
    Q = mdl.inducing_descriptors().reshape(mdl.m, -1)
    nptr = mdl.neighbors(N)[0]
    lone_i = np.diff(nptr) == 0
    lone_q = np.array([not np.isin(x._b, mdl.species).any() for x in mdl.X])
    K, bK = ref.knm(P, Q, zi, zq, lone_i, lone_q, eta)
    c0 = ref.covloss(K, bK, C, zi, zq)[0]
    alpha = ref.scale_for_c(c0)
    Ca = alpha * C
    install(mdl, mu, mean, Ca)
    if view:
        v = mdl.predict_view(numbers, pos, cell, pbc)
        out = dict(energy=float(v["energy"]), forces=v["forces"].copy(), stress=v["stress"].copy(), beta=v["beta"].copy(),
                   cov=mdl.last_cov(N))
    else:
        out = mdl.predict(numbers, pos, cell, pbc, cov=True)
    meanw = [mean[z] for z in mdl.species]
    ref.check_knm(out["cov"], K, bK, zi, zq, what=what)
    E, bE = ref.energy(K, bK, mu, zi, meanw)
    ref.check_energy(out["energy"], E, bE, what=what)
    c, bc = ref.covloss(K, bK, Ca, zi, zq)
    has_q = np.isin(zi, zq) & (zi >= 0)
    ref.check_c(ref.c_from_beta(out["beta"]), c, bc, rows=np.flatnonzero(has_q), what=what)
    assert np.all(np.isinf(out["beta"][(zi >= 0) & ~has_q])), what          # vscale = +inf: no inducing LCE of the species
    assert np.all(out["beta"][zi < 0] == 0) and np.all(out["forces"][zi < 0] == 0), what   # ghosts
    if oracle:
        from oracle import oracle as orc
        keep = zi >= 0
        X = mdl.X
        sp = np.array(mdl.species, np.int32)
        ind_z = np.array([x.number for x in X], np.int32)
        ind_ptr = np.concatenate([[0], np.cumsum([len(x._b) for x in X])])
        Pm, nnm = orc.inducing_descriptors(3, 3, RC, sp, ind_z, ind_ptr, np.concatenate([x._b for x in X]).astype(np.int32),
                                           np.concatenate([x._r for x in X]))
        nl = orc.neighbors(pos[keep], cell, pbc, RC)
        o = orc.frame(3, 3, RC, eta, sp, numbers[keep], pos[keep], cell, nl, ind_z, nnm, Pm, mu, want_p=False)
        fmax = np.abs(o["forces"]).max()
        assert np.abs(out["forces"][keep] - o["forces"]).max() <= 1e-8 * fmax, what
        assert np.abs(out["stress"] - o["stress"]).max() <= 1e-8 * max(np.abs(o["stress"]).max(), 1e-12), what
    return out


# ---------------------------------------------------------------------------------------------- edge frames
# (species table, atoms per species, inducing LCEs per species, ghosts).  Species block edges (aoff) at 15 / 16 / 17,
# 31 / 32 / 33, 63 / 64 / 65; inducing blocks (qoff) of 1, 31, 32, 33, 63, 64, 65, 127, 129 LCEs, one of 0; m across
# 64-column edges; species present in the table but not in the frame; a species of one atom; ghosts sharing the last
# species' row tile.
EDGES = {
    "s5": (SPECIES16[:5], [15, 17, 32, 1, 0], [31, 33, 64, 1, 65], 0),
    "s3_ghosts": (SPECIES16[:3], [16, 17, 30], [32, 63, 129], 3),
    "s3_noind": (SPECIES16[:3], [31, 34, 5], [127, 1, 0], 0),
    "s2": (SPECIES16[:2], [63, 2], [64, 1], 0),
    "s1": (SPECIES16[:1], [47], [65], 0),
    "s16": (SPECIES16, [3, 2, 1, 3, 0, 2, 3, 1, 2, 3, 3, 1, 2, 0, 3, 2], [3, 1, 2, 3, 2, 0, 1, 3, 2, 3, 1, 2, 3, 1, 2, 3], 0),
}


def edge_case(name, seed=0):
    sp, ac, qc, g = EDGES[name]
    mdl = model(sp, qc, seed=seed, ghosts=g > 0)
    return mdl, frame(sp, ac, seed + 5, ghosts=g)


# form: (environment, options, expected "step=" prefix or None for the automatic choice, whether fused / rev)
FORMS = {
    "auto": ({}, {}, None),
    "half_off": ({"SGPR_GEMM_HALF": "0"}, {}, "knm32 wcov32"),
    "bm64_kd32_w8": ({"SGPR_GEMM_BM": "64,64", "SGPR_GEMM_KD": "32,32", "SGPR_GEMM_WAVES": "8"}, {}, "knm64 wcov64"),
    "bm32_kd32_w8": ({"SGPR_GEMM_BM": "32,32", "SGPR_GEMM_KD": "32,32", "SGPR_GEMM_WAVES": "8"}, {}, "knm32 wcov32"),
    "bm32_kd16_w4": ({"SGPR_GEMM_BM": "32,32", "SGPR_GEMM_KD": "16,16", "SGPR_GEMM_WAVES": "4"}, {}, "knm32 wcov32"),
    "bm16_kd16_w8": ({"SGPR_GEMM_BM": "16,16", "SGPR_GEMM_KD": "16,16", "SGPR_GEMM_WAVES": "8"}, {}, "knm16 wcov16"),
    "r64_wgs2": ({"SGPR_GEMM_64": "1,1", "SGPR_GEMM_WGS64": "2"}, {}, "knm64 wcov64"),
    "r64_wgs3": ({"SGPR_GEMM_64": "1,1", "SGPR_GEMM_WGS64": "3"}, {}, "knm64 wcov64"),
    "fused": ({"SGPR_GEMM_HALF": "0"}, {"gemm_fused": 1}, "knm32 wcov32 chain0 cov=fused"),
    "cov_in_rev": ({"SGPR_GEMM_HALF": "0"}, {"cov_in_rev": 1}, "knm32 wcov32 chain0 cov=rev"),
    "chain_off": ({"SGPR_TILE_CHAIN": "0"}, {}, None),
    "balance_off": ({"SGPR_TILE_BALANCE": "0"}, {}, None),
    "xcd_quads_off": ({"SGPR_XCD_QUADS": "0"}, {}, None),
}
_ENV = ("SGPR_GEMM_HALF", "SGPR_GEMM_BM", "SGPR_GEMM_KD", "SGPR_GEMM_WAVES", "SGPR_GEMM_64", "SGPR_GEMM_WGS64",
        "SGPR_TILE_CHAIN", "SGPR_TILE_BALANCE", "SGPR_XCD_QUADS", "SGPR_GEMM_FUSED", "SGPR_COV_IN_REV")


def set_form(monkeypatch, form):
    env, opts, want = FORMS[form]
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return opts, want


def apply_opts(mdl, opts):
    from autoforce_amd import _lib
    for k, v in opts.items():
        _lib.check(_lib.load().sgpr_set_option(mdl.handle, k.encode(), int(v)))


def expected_auto(mdl, fr, world=1, rank=0, chain=True, half=True):
    numbers = fr[0]
    zi = slots_of(mdl.species, numbers)
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    S = len(mdl.species)
    aoff, cnt = ref.offsets(zi, S, rank, world)
    qoff = ref.qoffsets(zq, S)
    Dpad = mdl.dims["Dpad"]
    bk, bw = ref.tile_heights(aoff, qoff, cnt, mdl.m, Dpad, ncu(), half=half)
    nch = ref.chained(aoff, qoff, cnt, mdl.m, Dpad, ncu(), bw, chain=chain)
    return f"knm{bk} wcov{bw} chain{nch} cov=grouped"


@pytest.mark.parametrize("form", list(FORMS))
def test_edge_frames_in_every_tile_form(form, monkeypatch):
    opts, want = set_form(monkeypatch, form)
    for name in EDGES:
        mdl, fr = edge_case(name)
        apply_opts(mdl, opts)
        mu, mean, C = weights(mdl)
        check(mdl, fr, mu, mean, C, what=(form, name))
        got = step_form(mdl)
        exp = want if want is not None else expected_auto(mdl, fr, chain=form not in ("chain_off", "balance_off"))
        if form == "cov_in_rev" and len(mdl.species) > 8:
            exp = expected_auto(mdl, fr, half=False)      # (see test_cov_in_rev_sixteen_species)
        assert got.startswith(exp), (form, name, got, exp)
        mdl.close()


def test_cov_in_rev_sixteen_species(monkeypatch):
    """Found here: with option cov_in_rev at nine to sixteen species the reverse kernel (one atom per workgroup there)
    silently dropped the covloss tiles handed to it, and every c came back 0 (beta = sqrt(vscale)).  The step now keeps
    the covloss product in the grouped launch at those species counts."""
    opts, _ = set_form(monkeypatch, "cov_in_rev")
    mdl, fr = edge_case("s16")
    apply_opts(mdl, opts)
    mu, mean, C = weights(mdl)
    out = check(mdl, fr, mu, mean, C, what="cov_in_rev s16")
    assert step_form(mdl) == expected_auto(mdl, fr, half=False)
    assert step_form(mdl).startswith("knm32 wcov32 ")
    zi = slots_of(mdl.species, fr[0])
    assert np.max(ref.c_from_beta(out["beta"][np.isfinite(out["beta"]) & (zi >= 0)])) > 0.5
    mdl.close()


# ---------------------------------------------------------------------------------------------- automatic switches
SW_SPECIES = SPECIES16[:2]
SW_DPAD = 160      # (3, 3), two species: U = 8, Dc = 144


def _n32(q, which):
    def f(tot):
        a, m = [0, tot // 2, tot], q[-1]
        if which == "k":
            return ref.count_tiles(a, q, tot, m, SW_DPAD, 0, 32)
        return ref.count_tiles(a, q, tot, m, SW_DPAD, 1, 32) + ref.count_tiles(a, q, tot, m, SW_DPAD, 2, 32)
    return f


def _straddle(f, t, step=4):
    """The last frame size (atoms, half of each species) with f <= t and the next one, with f > t."""
    tot = step
    while f(tot + step) <= t:
        tot += step
    return tot, tot + step


# (name, inducing per species, product, largest n32 of the lower form, height below / above); thresholds follow the CU count
def _switches(nc):
    return [
        ("knm_half", (200, 201), "k", (2 * nc) // 5, 16, 32),          # half tiles while 5 n32 <= 2 ncu
        ("wcov_half", (200, 201), "w", (3 * nc) // 5, 16, 32),         # half tiles while 5 n32 <= 3 ncu
        ("knm_64", (1000, 1001), "k", 3 * nc - 1, 32, 64),             # 64 rows from n32 >= 3 ncu
        ("wcov_64", (1000, 1001), "w", -(-11 * nc // 2) - 1, 32, 64),   # 64 rows from 2 n32 >= 11 ncu
    ]


@pytest.mark.parametrize("idx", range(4))
def test_automatic_tile_heights_on_both_sides(idx, monkeypatch):
    """One row tile (4 atoms) either side of each threshold of decide_tile_heights / build_tiles."""
    set_form(monkeypatch, "auto")
    name, (m0, m1), which, t, below, above = _switches(ncu())[idx]
    mdl = model(SW_SPECIES, [m0, m1], seed=idx)
    assert mdl.dims["Dpad"] == SW_DPAD
    mu, mean, C = weights(mdl)
    for tot, h in zip(_straddle(_n32([0, m0, m0 + m1], which), t), (below, above)):
        fr = frame(SW_SPECIES, [tot // 2, tot - tot // 2], 40 + idx)
        check(mdl, fr, mu, mean, C, what=(name, tot), oracle=tot <= 700)
        got = step_form(mdl)
        assert got.startswith(expected_auto(mdl, fr)), (name, got)
        pos = 1 if which == "w" else 0
        assert int(got.split()[pos][4 if pos else 3:]) == h, (name, tot, got)
    mdl.close()


def test_chaining_window_both_ends(monkeypatch):
    """Frames whose largest XCD share of the grouped W + covloss table lies just below, inside (both ends) and just above
    the window (4 ncu/8, 5 ncu/8] in which the tiles beyond four per CU are chained: the successor count must be the
    restated one."""
    set_form(monkeypatch, "auto")
    nc = ncu()
    cx = nc // 8
    m0, m1 = 500, 501
    q = [0, m0, m0 + m1]
    mdl = model(SW_SPECIES, [m0, m1], seed=9)
    mu, mean, C = weights(mdl)

    def top(tot):
        return max(ref.xcd_shares([0, tot // 2, tot], q, tot, m0 + m1, SW_DPAD, 32))
    lo_out, lo_in = _straddle(top, 4 * cx, step=32)
    hi_in, hi_out = _straddle(top, 5 * cx, step=32)
    seen = []
    for tot in (lo_out, lo_in, hi_in, hi_out):
        fr = frame(SW_SPECIES, [tot // 2, tot - tot // 2], 60)
        assert ref.tile_heights([0, tot // 2, tot], q, tot, m0 + m1, SW_DPAD, nc)[1] == 32
        check(mdl, fr, mu, mean, C, what=("chain", tot), oracle=False)
        got = step_form(mdl)
        assert got == expected_auto(mdl, fr), (tot, top(tot), got)
        seen.append(int(got.split()[2][5:]))
    # none below the window; some at its lower end; at its upper end more than once the largest share has left it
    assert seen[0] == 0 and seen[1] > 0 and seen[2] > seen[3], seen
    mdl.close()


# ---------------------------------------------------------------------------------------------- choli shapes
def test_choli_general_blocks_then_lower_again():
    mdl, fr = edge_case("s3_ghosts")
    mu, mean, C = weights(mdl)
    _, _, G = weights(mdl, general=True)
    assert np.any(np.triu(G, 1) != 0)
    for M, what in ((C, "lower"), (G, "general"), (C, "lower again")):
        check(mdl, fr, mu, mean, M, what=what)
    mdl.close()


def test_cross_species_choli_is_refused():
    from autoforce_amd import SgprError
    mdl, fr = edge_case("s2")
    mu, mean, C = weights(mdl)
    check(mdl, fr, mu, mean, C, what="before")
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    a, b = np.flatnonzero(zq == 0)[-1], np.flatnonzero(zq == 1)[0]
    bad = C.copy()
    bad[b, a] = 1e-3            # (a lower-triangular entry in caller order, but across two species)
    with pytest.raises(SgprError):
        install(mdl, mu, mean, bad)
    check(mdl, fr, mu, mean, C, what="after the refusal")
    mdl.close()


# ---------------------------------------------------------------------------------------------- one handle, many calls
def test_one_handle_over_frames_and_inducing_edits():
    sp = SPECIES16[:3]
    mdl = model(sp, [63, 20, 40], seed=4)
    mu, mean, C = weights(mdl)
    A = frame(sp, [40, 30, 26], 70)
    B = frame(sp, [10, 60, 26], 71)                       # same N, other composition
    check(mdl, A, mu, mean, C, what="A")
    check(mdl, B, mu, mean, C, what="B")
    check(mdl, A, mu, mean, C, what="A view", view=True)
    check(mdl, B, mu, mean, C, what="B view", view=True)
    Cn = frame(sp, [70, 1, 33], 72)                       # another N
    check(mdl, Cn, mu, mean, C, what="N")
    extra = inducing(sp, [2, 0, 0], 99)
    for k in range(2):                                    # species 0: 63 -> 64 -> 65 columns
        mdl.add_inducing(extra[k])
        mu, mean, C = weights(mdl, seed=10 + k)
        check(mdl, Cn, mu, mean, C, what=("add", k))
        check(mdl, A, mu, mean, C, what=("add A", k))
    mdl.remove_inducing(-1)
    mu, mean, C = weights(mdl, seed=20)
    check(mdl, Cn, mu, mean, C, what="remove")
    sel = list(range(0, mdl.m, 2))[::-1]
    mdl.select_inducing(sel)
    mu, mean, C = weights(mdl, seed=21)
    check(mdl, B, mu, mean, C, what="select")
    mdl.close()


# ---------------------------------------------------------------------------------------------- sharded shares
@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_shares(world):
    mdl, fr = edge_case("s5")
    numbers, pos, cell, pbc = fr
    N = len(numbers)
    mu, mean, C = weights(mdl)
    full = check(mdl, fr, mu, mean, C, what="world 1")
    P = mdl.descriptors(N).reshape(N, -1)
    Q = mdl.inducing_descriptors().reshape(mdl.m, -1)
    zi = slots_of(mdl.species, numbers)
    zq = slots_of(mdl.species, [x.number for x in mdl.X])
    lone_i = np.diff(mdl.neighbors(N)[0]) == 0
    lone_q = np.array([not np.isin(x._b, mdl.species).any() for x in mdl.X])
    K, bK = ref.knm(P, Q, zi, zq, lone_i, lone_q, ETA)
    Ca = ref.scale_for_c(ref.covloss(K, bK, C, zi, zq)[0]) * C
    c, bc = ref.covloss(K, bK, Ca, zi, zq)
    install(mdl, mu, mean, Ca)
    perm = np.argsort(np.where(zi < 0, len(mdl.species), zi), kind="stable")
    E = 0.0
    F = np.zeros((N, 3))
    beta = np.zeros(N)
    for r in range(world):
        out = mdl.predict(numbers, pos, cell, pbc, rank=r, world=world, cov=True)
        mine = perm[r::world]
        ref.check_knm(out["cov"], K, bK, zi, zq, rows=mine, what=("rank", r))
        others = np.setdiff1d(np.arange(N), mine)
        assert np.all(out["cov"][others] == 0) and np.all(out["beta"][others] == 0)
        has_q = mine[np.isin(zi[mine], zq)]
        ref.check_c(ref.c_from_beta(out["beta"]), c, bc, rows=has_q, what=("rank", r))
        got = step_form(mdl)
        assert got.startswith(expected_auto(mdl, fr, world=world, rank=r)), (r, got)
        E += out["energy"]
        F += out["forces"]
        beta += out["beta"]
    Er, bE = ref.energy(K, bK, mu, zi, [mean[z] for z in mdl.species])
    ref.check_energy(E, Er, bE + 1e-15 * world * abs(float(Er)), what="sum of shares")
    assert np.abs(F - full["forces"]).max() <= 1e-12 * np.abs(full["forces"]).max()
    has_q = np.flatnonzero(np.isin(zi, zq) & (zi >= 0))
    ref.check_c(ref.c_from_beta(beta), c, bc, rows=has_q, what="sum of shares")
    mdl.close()
