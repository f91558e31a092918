"""Independent references for the six accumulators of the device MD loop (md_msd, md_rdf, md_vacf's neighbours md_vanhove,
md_adf, md_sq), in plain numpy.  Nothing here shares code with the twins of autoforce_amd/workloads.py or with rdf_geometry: pairs
come from oracle.neighbors (all pairs over all images) or from a fixed block of shifts, a distance is np.linalg.norm(pos[j] + off
@ cell - pos[i]), angles are arccos / arctan2, phases are exp(i q . r) with q from np.linalg.inv.  Nothing rounds a fractional
coordinate and nothing uses a cell height.

A frame is (numbers, pos, cell, pbc) as in lattices.py.  Every integer table comes with a table `near` of the same shape: the
number of entries that lie within NEAR (1e-9 of a bin width, 1e-9 rad, 1e-9 A of a cutoff) of an edge of that bin, on either side —
the entries another correct evaluation may put on the other side.

THE COMPARISON RULE, once (mismatch()): no more than NEAR_SHARE = 1e-4 of a table's entries may be near, asserted first; then an
integer table must equal its reference exactly in every bin without a near entry, and may differ by at most the bin's near count
elsewhere."""
import numpy as np

NEAR = 1e-9
NEAR_SHARE = 1e-4
ADF_MAXCOORD = 64    # the coordination table's length (the last entry: 63 and above), restated


def mismatch(got, want, near, what="", loose=0):
    """None if the integer table `got` agrees with `want` by the rule above, else a message.  `loose`: entries that may land in any
    bin (a bond at its cutoff moves every angle it takes part in): added to every bin's allowance."""
    got, want, near = (np.asarray(a).astype(np.int64) for a in (got, want, near))
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} against the reference's {want.shape}"
    entries = int(want.sum())
    if near.sum() + loose > NEAR_SHARE * max(entries, 1):
        return f"{what}: {int(near.sum())} + {loose} of {entries} entries are near an edge: the input decides nothing"
    bad = np.abs(got - want) > near + loose
    if not bad.any():
        return None
    k = tuple(int(v) for v in np.argwhere(bad)[0])
    return (f"{what}: {int(bad.sum())} of {bad.size} bins differ (entries {int(got.sum())} against {entries}); first at {k}: "
            f"{int(got[k])} against {int(want[k])}, near {int(near[k])}")


def _bin(r, lo, hi, bins):
    """(kept [n] bool, k [n], m [n], close [n] bool): md_rdf.inc's rule lo <= r < hi, k = min(int((r - lo) / (hi - lo) bins),
    bins - 1); m the index of the nearest edge lo + m (hi - lo) / bins and whether r is within NEAR widths of it."""
    r = np.asarray(r, float)
    w = (hi - lo) / bins
    kept = (r >= lo) & (r < hi)
    k = np.minimum(((r - lo) / (hi - lo) * bins).astype(np.int64), bins - 1)
    m = np.rint((r - lo) / w).astype(np.int64)
    close = (np.abs(r - (lo + m * w)) <= NEAR * w) & (m >= 0) & (m <= bins)
    return kept, k, m, close


def _hist(r, lo, hi, bins):
    """Counts [bins] and near counts [bins] of the distances r."""
    kept, k, m, close = _bin(r, lo, hi, bins)
    H = np.bincount(k[kept], minlength=bins)
    near = np.zeros(bins, dtype=np.int64)
    for side in (m[close] - 1, m[close]):        # (the bins on either side of the edge)
        side = side[(side >= 0) & (side < bins)]
        near += np.bincount(side, minlength=bins)
    return H, near


def _slots(numbers, species):
    species = [int(z) for z in species]
    return np.array([species.index(int(z)) for z in numbers])


# ------------------------------------------------------------------------------------------------------------------ rdf
def pair_distances(frame, rmax):
    """(i, j, r) of every (i, j, image) of oracle.neighbors within rmax (1 + 1e-6), periodic self-images included."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc = frame
    pos, cell = np.asarray(pos, float), np.asarray(cell, float).reshape(3, 3)
    ptr, j, off = orc.neighbors(pos, cell, pbc, rmax * (1.0 + 1e-6))
    i = np.repeat(np.arange(len(pos)), np.diff(ptr))
    return i, j, np.linalg.norm(pos[j] + off.astype(float) @ cell - pos[i], axis=1)


def rdf(frame, species, rmin, rmax, bins, pairs=None):
    """(H [S, S, bins], near [S, S, bins]) of one configuration.  pairs: pair_distances() of the frame at this rmax or a larger
    one (several rmax share one enumeration)."""
    slot, S = _slots(frame[0], species), len(species)
    i, j, r = pair_distances(frame, rmax) if pairs is None else pairs
    H, near = np.zeros((S, S, bins), dtype=np.int64), np.zeros((S, S, bins), dtype=np.int64)
    for a in range(S):
        for b in range(S):
            pick = (slot[i] == a) & (slot[j] == b)
            H[a, b], near[a, b] = _hist(r[pick], rmin, rmax, bins)
    return H, near


def rdf_run(frames, numbers, cell, pbc, species, every, rmin, rmax, bins):
    """The table of a run: the sum of rdf() over the configurations n with n % every == 0."""
    S = len(species)
    H, near = np.zeros((S, S, bins), dtype=np.int64), np.zeros((S, S, bins), dtype=np.int64)
    for n, x in enumerate(frames):
        if n % every == 0:
            h, e = rdf((numbers, x, cell, pbc), species, rmin, rmax, bins)
            H, near = H + h, near + e
    return H, near


# ------------------------------------------------------------------------------------------------------------------ windows
def windows(count, every, levels):
    """[(level, origin configuration, present configuration)] of MsdBlocks' and VanHoveCounts' scheme, restated: configuration n
    with n % every == 0 is sample s = n / every; at sample s every level l with s % 2^l == 0 measures against its origin if
    s >= 2^l and then takes s as its origin."""
    out = []
    for n in range(0, count, every):
        s = n // every
        for l in range(levels):
            if s % (1 << l):
                break
            if s >= (1 << l):
                out.append((l, (s - (1 << l)) * every, n))
    return out


# ------------------------------------------------------------------------------------------------------------------ van Hove
def shift_block(cell, pbc, reach, spread):
    """All integer shifts [M, 3] with |s_k| <= B along periodic directions: B = ceil(spread + reach |column k of inv(cell)|) + 1,
    where `spread` bounds |(x_j - x_i) inv(cell)| over the atoms: by Cauchy-Schwarz no image beyond the block comes within
    `reach` of anything."""
    inv = np.linalg.inv(np.asarray(cell, float).reshape(3, 3))
    B = [int(np.ceil(spread + reach * np.linalg.norm(inv[:, k]))) + 1 if pbc[k] else 0 for k in range(3)]
    return np.array([[s0, s1, s2] for s0 in range(-B[0], B[0] + 1) for s1 in range(-B[1], B[1] + 1) for s2 in range(-B[2], B[2] + 1)])


def ordered_distances(origin, now, cell, pbc, dmax):
    """(i, j, r) of every triple (i, j, s) with |now_j + s @ cell - origin_i| < dmax (1 + 1e-6), (j, s) != (i, 0), s over the fixed
    block of shift_block.  A float32 product picks the candidates (margin 1e-3 dmax^2 + 0.5 A^2: float32 keeps r^2 of atoms 200 A apart to 0.02), the distance itself is the plain norm in
    float64."""
    origin, now, cell = np.asarray(origin, float), np.asarray(now, float), np.asarray(cell, float).reshape(3, 3)
    N = len(origin)
    inv = np.linalg.inv(cell)
    spread = float(np.abs((now[None, :, :] - origin[:, None, :]) @ inv).max())
    block = shift_block(cell, pbc, dmax, spread)
    t = block.astype(float) @ cell                                   # [M, 3]
    t32, tt = t.astype(np.float32), (t * t).sum(axis=1).astype(np.float32)
    zero = int(np.flatnonzero(~block.any(axis=1))[0])
    lim = np.float32(dmax * dmax * (1.0 + 1e-3) + 0.5)
    I, J, R = [], [], []
    for i in range(N):
        a = now - origin[i]                                          # [N, 3]
        r2 = (a * a).sum(axis=1).astype(np.float32)[:, None] + 2.0 * (a.astype(np.float32) @ t32.T) + tt[None, :]
        jj, ss = np.nonzero(r2 < lim)
        keep = ~((jj == i) & (ss == zero))
        jj, ss = jj[keep], ss[keep]
        r = np.linalg.norm(now[jj] + t[ss] - origin[i], axis=1)
        ok = r < dmax * (1.0 + 1e-6)
        I.append(np.full(int(ok.sum()), i)); J.append(jj[ok]); R.append(r[ok])
    return np.concatenate(I), np.concatenate(J), np.concatenate(R)


def vanhove_distinct(frames, numbers, cell, pbc, species, every, levels, dmaxes, dbins):
    """{dmax: (H [levels, S, S, dbins], near)}: per window of windows() the distances between an atom's place in the origin
    configuration and every image of every atom in the present one (row: the origin's species), binned by md_rdf.inc's rule with
    rmin = 0.  Several dmax share one enumeration."""
    slot, S = _slots(numbers, species), len(species)
    top = max(dmaxes)
    out = {d: (np.zeros((levels, S, S, dbins), dtype=np.int64), np.zeros((levels, S, S, dbins), dtype=np.int64)) for d in dmaxes}
    for l, o, n in windows(len(frames), every, levels):
        i, j, r = ordered_distances(frames[o], frames[n], cell, pbc, top)
        for a in range(S):
            for b in range(S):
                pick = (slot[i] == a) & (slot[j] == b)
                for d in dmaxes:
                    h, e = _hist(r[pick], 0.0, d, dbins)
                    out[d][0][l, a, b] += h
                    out[d][1][l, a, b] += e
    return out


def vanhove_self(frames, numbers, species, every, levels, rmax, rbins, tbins, pbins):
    """(H [levels, S, rbins, tbins, pbins], over [levels, S], near like H, near_over, count [levels]): the raw displacements x(now)
    - x(origin) of every window in spherical bins: r = norm, theta = arccos(d2 / r) over [0, pi], phi = arctan2(d1, d0) over
    [-pi, pi); r >= rmax goes to `over`; r == 0 to (0, 0, pbins / 2).  An entry within NEAR of a radial, polar or azimuthal edge is
    near in its own bin and in the one across that edge."""
    slot, S = _slots(numbers, species), len(species)
    shape = (levels, S, rbins, tbins, pbins)
    H, near = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    over, near_over, count = np.zeros((levels, S), dtype=np.int64), np.zeros((levels, S), dtype=np.int64), np.zeros(levels, dtype=np.int64)
    for l, o, n in windows(len(frames), every, levels):
        count[l] += 1
        d = np.asarray(frames[n], float) - np.asarray(frames[o], float)
        r = np.linalg.norm(d, axis=1)
        kept, kr, mr, close_r = _bin(r, 0.0, rmax, rbins)
        safe = np.where(r > 0.0, r, 1.0)
        th = np.arccos(np.clip(d[:, 2] / safe, -1.0, 1.0))
        ph = np.arctan2(d[:, 1], d[:, 0])
        ft, fp = th / (np.pi / tbins), (ph + np.pi) / (2.0 * np.pi / pbins)
        kt = np.minimum(np.floor(ft).astype(np.int64), tbins - 1)
        kp = np.minimum(np.floor(fp).astype(np.int64), pbins - 1)
        held = r == 0.0
        kt[held], kp[held] = 0, pbins // 2
        close_t = (np.abs(ft - np.rint(ft)) * (np.pi / tbins) < NEAR) & (np.rint(ft) >= 1) & (np.rint(ft) <= tbins - 1)   # (a pole is no edge)
        close_p = (np.abs(fp - np.rint(fp)) * (2.0 * np.pi / pbins) < NEAR) & (pbins > 1)
        for i in range(len(d)):
            z = slot[i]
            if kept[i]:
                H[l, z, kr[i], kt[i], kp[i]] += 1
            else:
                over[l, z] += 1
            if close_r[i] or (kept[i] and (close_t[i] or close_p[i])):
                if close_r[i] and mr[i] == rbins:
                    near_over[l, z] += 1
                for er in ((mr[i] - 1, mr[i]) if close_r[i] else (kr[i],)):
                    for et in ((int(np.rint(ft[i])) - 1, int(np.rint(ft[i]))) if close_t[i] else (kt[i],)):
                        for ep in ((int(np.rint(fp[i])) - 1, int(np.rint(fp[i]))) if close_p[i] else (kp[i],)):
                            if 0 <= er < rbins and 0 <= et < tbins:
                                near[l, z, er, et, ep % pbins] += 1
    return H, over, near, near_over, count


# ------------------------------------------------------------------------------------------------------------------ msd
def msd(frames, numbers, species, masses, every, levels, com):
    """dict(count [L], msd, msd_sq, smd, smd_sq [L, S]): per window d = x(now) - x(origin), c = sum m d / sum m (com; else 0), per
    species msd = mean |d_i - c|^2 and smd = |sum (d_i - c)|^2 / n_z; the table holds their sums and the sums of their squares."""
    slot, S = _slots(numbers, species), len(species)
    m = np.asarray(masses, float)
    out = dict(count=np.zeros(levels, dtype=np.int64), **{k: np.zeros((levels, S)) for k in ("msd", "msd_sq", "smd", "smd_sq")})
    for l, o, n in windows(len(frames), every, levels):
        d = np.asarray(frames[n], float) - np.asarray(frames[o], float)
        if com:
            d = d - (m[:, None] * d).sum(axis=0) / m.sum()
        out["count"][l] += 1
        for z in range(S):
            e = d[slot == z]
            if len(e) == 0:
                continue
            a, b = float((e * e).sum(axis=1).mean()), float((e.sum(axis=0) ** 2).sum() / len(e))
            out["msd"][l, z] += a; out["msd_sq"][l, z] += a * a; out["smd"][l, z] += b; out["smd_sq"][l, z] += b * b
    return out


# ------------------------------------------------------------------------------------------------------------------ adf
def adf_neighbours(frame, species, cut):
    """Per centre the list of (d [3], r, slot) of its bonded neighbours — every (j, image) of oracle.neighbors with r < cut[a, b],
    periodic self-images included —, the smallest gap between a distance and its cutoff, and per centre whether a bond lies within
    NEAR of its cutoff."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc = frame
    pos, cell, cut = np.asarray(pos, float), np.asarray(cell, float).reshape(3, 3), np.asarray(cut, float)
    slot = _slots(numbers, species)
    ptr, j, off = orc.neighbors(pos, cell, pbc, float(cut.max()) + 1e-6)
    out, gap, loose = [], np.inf, np.zeros(len(pos), dtype=bool)
    for i in range(len(pos)):
        nb = []
        for t in range(ptr[i], ptr[i + 1]):
            d = pos[j[t]] + off[t].astype(float) @ cell - pos[i]
            r = float(np.linalg.norm(d))
            c = cut[slot[i], slot[j[t]]]
            if c > 0.0:
                gap = min(gap, abs(r - c))
                loose[i] |= abs(r - c) < NEAR
            if r < c:
                nb.append((d, r, int(slot[j[t]])))
        out.append(nb)
    return slot, out, gap, loose


def adf(frame, species, cut, bins):
    """dict(angles [S, S, S, bins] filled out symmetric in the ends, coord [S, S, 64], near like angles, loose: the angles of
    centres with a bond within NEAR of its cutoff, gap_angle (rad), gap_r, per_centre [N, S] neighbour counts): test_adf_twin_cpu's
    brute force, generalised to a pbc pattern and a cutoff table.  theta = arccos(d . d' / (r r')), bin floor(theta bins / pi)
    (the last bin takes pi)."""
    S = len(species)
    slot, nbs, gap_r, loose_c = adf_neighbours(frame, species, cut)
    H, near = np.zeros((S, S, S, bins), dtype=np.int64), np.zeros((S, S, S, bins), dtype=np.int64)
    C = np.zeros((S, S, ADF_MAXCOORD), dtype=np.int64)
    per = np.zeros((len(nbs), S), dtype=np.int64)
    gap_angle, loose = np.inf, 0
    for i, nb in enumerate(nbs):
        a = slot[i]
        cnt = np.bincount([b for _, _, b in nb], minlength=S)
        per[i] = cnt
        for b in range(S):
            C[a, b, min(cnt[b], ADF_MAXCOORD - 1)] += 1
        if len(nb) < 2:
            continue
        d, r, sl = np.array([x[0] for x in nb]), np.array([x[1] for x in nb]), np.array([x[2] for x in nb])
        u, v = np.triu_indices(len(nb), 1)
        th = np.arccos(np.clip((d[u] * d[v]).sum(axis=1) / (r[u] * r[v]), -1.0, 1.0))
        f = th / (np.pi / bins)
        g = np.abs(f - np.rint(f)) * (np.pi / bins)
        gap_angle = min(gap_angle, float(g.min()))
        k = np.minimum(np.floor(f).astype(np.int64), bins - 1)
        lo, hi = np.minimum(sl[u], sl[v]), np.maximum(sl[u], sl[v])
        np.add.at(H, (a, lo, hi, k), 1)
        close = (g < NEAR) & (np.rint(f) >= 1) & (np.rint(f) <= bins - 1)   # (0 and pi end the range: no bin lies beyond them)
        for e in (np.rint(f[close]).astype(np.int64) - 1, np.rint(f[close]).astype(np.int64)):
            ok = (e >= 0) & (e < bins)
            np.add.at(near, (a, lo[close][ok], hi[close][ok], e[ok]), 1)
        if loose_c[i]:
            loose += len(u) + len(nb)
    for b in range(S):
        for c in range(b):
            H[:, b, c], near[:, b, c] = H[:, c, b], near[:, c, b]
    return dict(angles=H, coord=C, near=near, loose=loose, gap_angle=gap_angle, gap_r=gap_r, per_centre=per)


def adf_run(frames, numbers, cell, pbc, species, cut, every, bins):
    """The tables of a run: adf() summed over the configurations n with n % every == 0."""
    tot = None
    for n, x in enumerate(frames):
        if n % every:
            continue
        t = adf((numbers, x, cell, pbc), species, cut, bins)
        if tot is None:
            tot = t
        else:
            for k in ("angles", "coord", "near", "loose"):
                tot[k] = tot[k] + t[k]
            tot["gap_angle"], tot["gap_r"] = min(tot["gap_angle"], t["gap_angle"]), min(tot["gap_r"], t["gap_r"])
    return tot


# ------------------------------------------------------------------------------------------------------------------ sq
def sq(frames, hkl, every, lags, origin_every, numbers, species, cell):
    """dict(f [lags, nq, S, S], mean [nq, S], count [lags], samples, rho): test_sq_twin_cpu's direct evaluation.  q = 2 pi hkl
    inv(cell)^T with np.linalg.inv, exp(i q . r) per atom and its sum per species in np.longdouble, every density of the run
    kept, the correlations by plain loops over (sample, lag)."""
    LD = np.longdouble
    numbers = np.asarray(numbers)
    q = (2.0 * np.pi * np.asarray(hkl, float) @ np.linalg.inv(np.asarray(cell, float).reshape(3, 3)).T).astype(LD)
    rho = []
    for n, x in enumerate(frames):
        if n % every == 0:
            ph = np.asarray(x, float).astype(LD) @ q.T                      # [atom, nq]
            e = np.cos(ph) + 1j * np.sin(ph)
            rho.append(np.stack([e[numbers == z].sum(axis=0) for z in species], axis=1))
    S, nq = len(species), len(hkl)
    f, mean, count = np.zeros((lags, nq, S, S), dtype=LD), np.zeros((nq, S), dtype=np.clongdouble), np.zeros(lags, dtype=np.int64)
    for s in range(len(rho)):
        mean += rho[s]
        for k in range(lags):
            o = s - k
            if o >= 0 and o % origin_every == 0:
                count[k] += 1
                for a in range(S):
                    for b in range(S):
                        f[k, :, a, b] += (rho[s][:, a] * np.conj(rho[o][:, b])).real
    return dict(f=f.astype(float), mean=mean.astype(complex), count=count, samples=len(rho), rho=[r.astype(complex) for r in rho])
