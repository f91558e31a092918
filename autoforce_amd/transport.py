"""Transport coefficients from the displacement tables of the MD loops: what theforce/analysis/analysis.py:109-176 and :296-338
(`displacements`, `correlator`, `mean_var`, `get_slopes`, `diffusion_constants`) work out of a stored trajectory, from the table
the run itself accumulates — SGPRModel.md_msd on the device, workloads.MsdBlocks on the host.  Per level (lag 2^l samples) and
species the table holds the sums of the tracer msd = mean_i |d_i|^2 and of the collective smd = |sum_i d_i|^2 / n over the
level's windows, and of their squares; the windows of a level do not overlap, so their scatter gives an error bar.
  And the structure beside it: `Rdf` holds the pair-distance counts of SGPRModel.md_rdf / workloads.RdfCounts, and
`radial_distribution` forms the g(r) per species pair of theforce/analysis/rdf.py's `rdf` from them."""
import numpy as np

KEYS = ("msd", "msd_sq", "smd", "smd_sq")


class Msd:
    """Holder of a displacement table: ActiveCalculator.run_md(msd=Msd(every, levels, com)) fills it, the way ml_filter= takes a
    FilterState; add(table) adds the table of a run (SGPRModel.md_msd_table(), MsdBlocks.table()) — the tables of several runs
    with the same settings add up, window by window.  mean() and stderr() are the reference's mean_var per lag."""

    def __init__(self, every, levels, com=False):
        self.every, self.levels, self.com = int(every), int(levels), bool(com)
        self.lags = self.every * 2 ** np.arange(self.levels, dtype=np.int64)   # in evaluations
        self.count = np.zeros(self.levels, dtype=np.int64)
        self.species = self.n = None
        for k in KEYS:
            setattr(self, k, None)

    def add(self, table):
        if not np.array_equal(np.asarray(table["lags"]), self.lags):
            raise ValueError("Msd.add: the table was taken with other settings (every, levels)")
        species = np.asarray(table["species"])
        if self.species is None:
            self.species, self.n = species.copy(), np.asarray(table["n"]).copy()
            for k in KEYS:
                setattr(self, k, np.zeros((self.levels, len(species))))
        elif not (np.array_equal(species, self.species) and np.array_equal(np.asarray(table["n"]), self.n)):
            raise ValueError("Msd.add: the table is of another frame (species, atoms per species)")
        self.count = self.count + np.asarray(table["count"], dtype=np.int64)
        for k in KEYS:
            setattr(self, k, getattr(self, k) + np.asarray(table[k], float))
        return self

    def table(self):
        return dict(lags=self.lags.copy(), count=self.count.copy(), species=self.species, n=self.n, **{k: getattr(self, k).copy() for k in KEYS})

    def _moments(self, key):
        c = np.where(self.count > 0, self.count, 1)[:, None].astype(float)
        mean = np.where(self.count[:, None] > 0, getattr(self, key) / c, np.nan)
        var = np.maximum(getattr(self, key + "_sq") / c - mean * mean, 0.0)   # (np.var of the windows: the reference's mean_var)
        return mean, np.sqrt(var / c)

    def mean(self):
        """dict(msd [L, S], smd [L, S]): the means over a level's windows (nan where a level has none)."""
        return dict(msd=self._moments("msd")[0], smd=self._moments("smd")[0])

    def stderr(self):
        """dict(msd [L, S], smd [L, S]): sqrt(var / count) of a level's windows — independent blocks."""
        return dict(msd=self._moments("msd")[1], smd=self._moments("smd")[1])


def _slopes(x, y, yerr):
    """The reference's get_slopes — the slopes of straight lines through y, y - yerr and y + yerr — with the points weighted
    by 1 / yerr where every error bar is positive."""
    w = 1.0 / yerr if np.all(yerr > 0.0) else None
    return tuple(float(np.polyfit(x, yy, 1, w=w)[0]) for yy in (y, y - yerr, y + yerr))


def diffusion_constants(msd, dt_fs):
    """{Z: dict(Dt=(D, lower, upper), Dj=(D, lower, upper))} in Angstrom^2 / fs per species of the holder `msd` present in the
    frame: the slopes of msd (tracer, D_t) and smd (collective, D_j) against time over the levels with at least two windows,
    divided by 6, and the same through the values less and plus their error bars (the reference's diffusion_constants)."""
    mean, err = msd.mean(), msd.stderr()
    use = msd.count >= 2
    if int(use.sum()) < 2:
        raise ValueError("diffusion_constants: fewer than two lags with at least two windows")
    t = msd.lags[use] * float(dt_fs)
    out = {}
    for k, z in enumerate(msd.species):
        if msd.n[k] == 0:
            continue
        out[int(z)] = dict(Dt=tuple(a / 6.0 for a in _slopes(t, mean["msd"][use, k], err["msd"][use, k])),
                           Dj=tuple(a / 6.0 for a in _slopes(t, mean["smd"][use, k], err["smd"][use, k])))
    return out


class Rdf:
    """Holder of pair-distance counts: ActiveCalculator.run_md(rdf=Rdf(every, rmax, bins, rmin)) fills it, as msd= fills an Msd;
    add(table) adds the table of a run (SGPRModel.md_rdf_table(), RdfCounts.table()) — the tables of several runs of one frame
    with the same settings add up, count by count.  radial_distribution(holder) forms g(r)."""

    def __init__(self, every, rmax, bins=100, rmin=0.0):
        self.every, self.rmax, self.bins, self.rmin = int(every), float(rmax), int(bins), float(rmin)
        self.samples = 0
        self.hist = self.species = self.n = self.volume = None

    def add(self, table):
        if (int(table["bins"]), float(table["rmin"]), float(table["rmax"])) != (self.bins, self.rmin, self.rmax):
            raise ValueError("Rdf.add: the table was taken with other settings (rmin, rmax, bins)")
        species, n = np.asarray(table["species"]), np.asarray(table["n"])
        if self.species is None:
            self.species, self.n, self.volume = species.copy(), n.copy(), float(table["volume"])
            self.hist = np.zeros((len(species), len(species), self.bins), dtype=np.uint64)
        elif not (np.array_equal(species, self.species) and np.array_equal(n, self.n) and float(table["volume"]) == self.volume):
            raise ValueError("Rdf.add: the table is of another frame (species, atoms per species, volume)")
        self.hist = self.hist + np.asarray(table["hist"], dtype=np.uint64)
        self.samples += int(table["samples"])
        return self

    def table(self):
        return dict(hist=self.hist.copy(), species=self.species, n=self.n, samples=self.samples, next_due=self.samples * self.every,
                    every=self.every, bins=self.bins, rmin=self.rmin, rmax=self.rmax, volume=self.volume)


def radial_distribution(rdf, shells=False):
    """(r [bins], {(Za, Zb): g [bins]}) from the holder `rdf`, over the pairs the reference's `rdf` lists for the species present
    in the frame, in ascending atomic number: (a, a), then the combinations a < b.
        g_ab(k) = H[a][b][k] / (samples n_a 4 pi r_k^2 dr n_b / V)
    on the reference's axis r = linspace(rmin, rmax, bins) + dr / 2 with dr = (rmax - rmin) / (bins - 1) — its own quirk: the
    histogram's bins are (rmax - rmin) / bins wide —, kept as the default so that results match it (bins >= 2).  shells=True:
    the true bins, r_k their centres and the shell volume 4 pi / 3 (r_hi^3 - r_lo^3) in the place of 4 pi r_k^2 dr."""
    if rdf.hist is None or rdf.samples == 0:
        raise ValueError("radial_distribution: the holder has no samples")
    if shells:
        edges = rdf.rmin + (rdf.rmax - rdf.rmin) * np.arange(rdf.bins + 1) / rdf.bins
        r = 0.5 * (edges[:-1] + edges[1:])
        shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    else:
        if rdf.bins < 2:
            raise ValueError("radial_distribution: the reference's axis needs two bins; shells=True serves one")
        r = np.linspace(rdf.rmin, rdf.rmax, rdf.bins)
        dr = r[1] - r[0]
        r = r + dr / 2
        shell = 4 * np.pi * r ** 2 * dr
    slot = {int(z): k for k, z in enumerate(rdf.species) if rdf.n[k] > 0}
    zs = sorted(slot)
    pairs = [(z, z) for z in zs] + [(zs[p], zs[q]) for p in range(len(zs)) for q in range(p + 1, len(zs))]
    g = {}
    for za, zb in pairs:
        a, b = slot[za], slot[zb]
        g[(za, zb)] = rdf.hist[a, b].astype(float) / (rdf.samples * float(rdf.n[a]) * shell * (float(rdf.n[b]) / rdf.volume))
    return r, g
