"""Transport coefficients from the displacement tables of the MD loops: what theforce/analysis/analysis.py:109-176 and :296-338
(`displacements`, `correlator`, `mean_var`, `get_slopes`, `diffusion_constants`) work out of a stored trajectory, from the table
the run itself accumulates — SGPRModel.md_msd on the device, workloads.MsdBlocks on the host.  Per level (lag 2^l samples) and
species the table holds the sums of the tracer msd = mean_i |d_i|^2 and of the collective smd = |sum_i d_i|^2 / n over the
level's windows, and of their squares; the windows of a level do not overlap, so their scatter gives an error bar.
  And the structure beside it: `Rdf` holds the pair-distance counts of SGPRModel.md_rdf / workloads.RdfCounts, and
`radial_distribution` forms the g(r) per species pair of theforce/analysis/rdf.py's `rdf` from them.
  And the dynamics: `Vacf` holds the velocity correlations of SGPRModel.md_vacf / workloads.VacfRing; `green_kubo`, `onsager` and
`vibrational_dos` read a diffusion constant, the species' current correlations and a density of states off them.
  And the distributions behind the moments: `VanHove` holds the displacement and pair histograms per lag of SGPRModel.md_vanhove /
workloads.VanHoveCounts; `displacement_histogram` is the return of analysis.py:178-210 (`hist_rtp_displacements`), `self_van_hove`,
`distinct_van_hove` and `non_gaussian` form G_s(r, t), G_d(r, t) and alpha_2(t).
  And the three-body structure: `Adf` holds the bond-angle and coordination counts of SGPRModel.md_adf / workloads.AdfCounts (the
reference has no angular analysis); `angle_distribution` and `coordination` form P(theta) and P(n) per species.
  And reciprocal space: `Sq` holds the density correlations of SGPRModel.md_sq / workloads.SqRing at the wave vectors `q_vectors`
lists (the reference has none); `structure_factor`, `intermediate_scattering` and `dynamic_structure_factor` form S_ab(q),
F_ab(q, t) and S_ab(q, omega)."""
import numpy as np

KEYS = ("msd", "msd_sq", "smd", "smd_sq")


class _InLoop:
    """The face ActiveCalculator.run_md drives every holder through, its only coupling to them.  A holder names the SGPRModel
    method that attaches its accumulator (`md`; md + "_table" reads it) and its host twin in workloads (`twin_of`), both taking
    settings() first; the twin is built with the masses or with the cell (`with_masses`) and fed a step's `feeds`.  Where the
    device loop does not serve the holder: constant_cell (run_md's refusal under a barostat; None: the twin serves one) and
    host_only() (the host loop feeds the twin)."""
    feeds, with_masses, constant_cell = "positions", False, None

    def twin(self, masses, numbers, species, cell, pbc):
        from . import workloads
        frame = (masses, numbers, species) if self.with_masses else (numbers, species, cell, pbc)
        return getattr(workloads, self.twin_of)(*self.settings(), *frame)

    def attach(self, engine):
        getattr(engine, self.md)(*self.settings())

    def read(self, engine):
        return getattr(engine, self.md + "_table")()

    def host_only(self, npt, committee, ranks, filtered, biased):
        return bool(npt or committee or ranks > 1)


class Msd(_InLoop):
    """Holder of a displacement table: ActiveCalculator.run_md(msd=Msd(every, levels, com)) fills it, the way ml_filter= takes a
    FilterState; add(table) adds the table of a run (SGPRModel.md_msd_table(), MsdBlocks.table()) — the tables of several runs
    with the same settings add up, window by window.  mean() and stderr() are the reference's mean_var per lag."""
    md, twin_of, with_masses = "md_msd", "MsdBlocks", True

    def __init__(self, every, levels, com=False):
        self.every, self.levels, self.com = int(every), int(levels), bool(com)
        self.lags = self.every * 2 ** np.arange(self.levels, dtype=np.int64)   # in evaluations
        self.count = np.zeros(self.levels, dtype=np.int64)
        self.species = self.n = None
        for k in KEYS:
            setattr(self, k, None)

    def settings(self):
        return (self.every, self.levels, self.com)

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


class Rdf(_InLoop):
    """Holder of pair-distance counts: ActiveCalculator.run_md(rdf=Rdf(every, rmax, bins, rmin)) fills it, as msd= fills an Msd;
    add(table) adds the table of a run (SGPRModel.md_rdf_table(), RdfCounts.table()) — the tables of several runs of one frame
    with the same settings add up, count by count.  radial_distribution(holder) forms g(r)."""
    md, twin_of, constant_cell = "md_rdf", "RdfCounts", "pair distances are counted"

    def __init__(self, every, rmax, bins=100, rmin=0.0):
        self.every, self.rmax, self.bins, self.rmin = int(every), float(rmax), int(bins), float(rmin)
        self.samples = 0
        self.hist = self.species = self.n = self.volume = None

    def settings(self):
        return (self.every, self.rmax, self.bins, self.rmin)

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


class Adf(_InLoop):
    """Holder of bond-angle and coordination counts: ActiveCalculator.run_md(adf=Adf(every, bins, cutoffs)) fills it, as rdf= fills
    an Rdf; `cutoffs` is a scalar (all pairs) or a dict {(Z1, Z2): r} of bond cutoffs (pairs that are absent never bond).
    add(table) adds the tables of a run (SGPRModel.md_adf_table(), AdfCounts.table()) — those of several runs of one frame with
    the same settings add up, count by count.  angle_distribution(holder, ...) and coordination(holder, ...) read it."""
    md, twin_of, constant_cell = "md_adf", "AdfCounts", "bond angles are counted"

    def __init__(self, every, bins=180, cutoffs=None):
        if cutoffs is None:
            raise ValueError("Adf: cutoffs= (a scalar or {(Z1, Z2): r}) says which pairs bond")
        self.every, self.bins, self.cutoffs = int(every), int(bins), cutoffs
        self.samples = 0
        self.angles = self.coord = self.species = self.n = self.cut = None

    def settings(self):
        return (self.every, self.bins, self.cutoffs)

    def add(self, table):
        if int(table["bins"]) != self.bins:
            raise ValueError("Adf.add: the table was taken with other settings (bins)")
        species, n, cut = np.asarray(table["species"]), np.asarray(table["n"]), np.asarray(table["cut"], float)
        if self.species is None:
            self.species, self.n, self.cut = species.copy(), n.copy(), cut.copy()
            self.angles = np.zeros((len(species),) * 3 + (self.bins,), dtype=np.uint64)
            self.coord = np.zeros((len(species), len(species), np.asarray(table["coord"]).shape[-1]), dtype=np.uint64)
        elif not (np.array_equal(species, self.species) and np.array_equal(n, self.n) and np.array_equal(cut, self.cut)):
            raise ValueError("Adf.add: the table is of another frame or other cutoffs (species, atoms per species, cut)")
        self.angles = self.angles + np.asarray(table["angles"], dtype=np.uint64)
        self.coord = self.coord + np.asarray(table["coord"], dtype=np.uint64)
        self.samples += int(table["samples"])
        return self

    def table(self):
        return dict(angles=self.angles.copy(), coord=self.coord.copy(), species=self.species, n=self.n, samples=self.samples,
                    next_due=self.samples * self.every, every=self.every, bins=self.bins, cut=self.cut)


def _adf_slot(table, z, what):
    species = [int(s) for s in table["species"]]
    if int(z) not in species:
        raise ValueError(f"{what}: no species {z} in the table ({species})")
    return species.index(int(z))


def angle_distribution(table, centre, ends, degrees=True, solid_angle=False):
    """(theta [bins], P [bins]) of the angles end-centre-end from an Adf holder or a table (md_adf_table(), AdfCounts.table()):
    centre an atomic number, ends a pair of them (either order).  theta: the centres of the bins [k pi / bins, (k + 1) pi / bins),
    in degrees or radians; P(theta) normalised to unit area over that axis.  solid_angle=True: the counts divided by sin(theta)
    first — the density per solid angle, flat for directions without correlation — then normalised the same way."""
    t = table.table() if hasattr(table, "table") else table
    a = _adf_slot(t, centre, "angle_distribution")
    b, c = (_adf_slot(t, z, "angle_distribution") for z in ends)
    bins = int(t["bins"])
    h = np.asarray(t["angles"])[a, b, c].astype(float)
    th = (np.arange(bins) + 0.5) * np.pi / bins
    if solid_angle:
        h = h / np.sin(th)
    axis = np.degrees(th) if degrees else th
    width = (180.0 if degrees else np.pi) / bins
    total = h.sum() * width
    if not total > 0.0:
        raise ValueError("angle_distribution: no angle was counted for these species")
    return axis, h / total


def coordination(table, centre, neighbour):
    """(n [M], P [M], mean) of the number of neighbours of species `neighbour` around the centres of species `centre` (atomic
    numbers) from an Adf holder or a table: P(n) over the sampled centres; the last entry, n = M - 1 = 63, stands for that many
    and more (the mean takes it as 63)."""
    t = table.table() if hasattr(table, "table") else table
    a, b = _adf_slot(t, centre, "coordination"), _adf_slot(t, neighbour, "coordination")
    c = np.asarray(t["coord"])[a, b].astype(float)
    if not c.sum() > 0.0:
        raise ValueError("coordination: no centre of this species was sampled")
    n = np.arange(len(c))
    P = c / c.sum()
    return n, P, float(np.sum(n * P))


class Vacf(_InLoop):
    """Holder of a velocity-correlation table: ActiveCalculator.run_md(vacf=Vacf(every, lags, origin_every, com)) fills it, as
    msd= fills an Msd; add(table) adds the table of a run (SGPRModel.md_vacf_table(), VacfRing.table()) — the tables of several
    runs of one frame with the same settings add up, pair by pair.  mean() gives the curves per species; green_kubo, onsager and
    vibrational_dos read them."""
    md, twin_of, with_masses, feeds = "md_vacf", "VacfRing", True, "velocities"

    def __init__(self, every, lags, origin_every=1, com=False):
        self.every, self.nlags, self.origin_every, self.com = int(every), int(lags), int(origin_every), bool(com)
        self.lags = self.every * np.arange(self.nlags, dtype=np.int64)   # in configurations
        self.count = np.zeros(self.nlags, dtype=np.int64)
        self.samples = 0
        self.tracer = self.collective = self.species = self.n = None

    def settings(self):
        return (self.every, self.nlags, self.origin_every, self.com)

    def host_only(self, npt, committee, ranks, filtered, biased):   # (a filtered or a biased run's closing kick is not the packed force's)
        return bool(super().host_only(npt, committee, ranks, filtered, biased) or filtered or biased)

    def add(self, table):
        if not np.array_equal(np.asarray(table["lags"]), self.lags):
            raise ValueError("Vacf.add: the table was taken with other settings (every, lags)")
        species, n = np.asarray(table["species"]), np.asarray(table["n"])
        if self.species is None:
            self.species, self.n = species.copy(), n.copy()
            self.tracer, self.collective = np.zeros((self.nlags, len(species))), np.zeros((self.nlags, len(species), len(species)))
        elif not (np.array_equal(species, self.species) and np.array_equal(n, self.n)):
            raise ValueError("Vacf.add: the table is of another frame (species, atoms per species)")
        self.count = self.count + np.asarray(table["count"], dtype=np.int64)
        self.tracer = self.tracer + np.asarray(table["tracer"], float)
        self.collective = self.collective + np.asarray(table["collective"], float)
        self.samples += int(table["samples"])
        return self

    def table(self):
        return dict(tracer=self.tracer.copy(), collective=self.collective.copy(), count=self.count.copy(), lags=self.lags.copy(),
                    species=self.species, n=self.n, samples=self.samples)

    def mean(self):
        """dict(tracer [lags, S], collective [lags, S, S]): the means over a lag's pairs of samples (nan where a lag has none)."""
        if self.tracer is None:
            raise ValueError("Vacf.mean: the holder has no table")
        c = np.where(self.count > 0, self.count, 1).astype(float)
        ok = self.count > 0
        return dict(tracer=np.where(ok[:, None], self.tracer / c[:, None], np.nan),
                    collective=np.where(ok[:, None, None], self.collective / c[:, None, None], np.nan))


ASE_FS = 0.09822694788464063   # one femtosecond in the time unit of the velocities, A sqrt(amu / eV) (workloads.FS, ase.units.fs)


def _running_integral(y, dt):
    """Trapezoid rule along axis 0 from the first point: [0, (y0 + y1) dt / 2, ...]."""
    out = np.zeros_like(y)
    out[1:] = np.cumsum(0.5 * (y[1:] + y[:-1]), axis=0) * dt
    return out


def green_kubo(vacf, dt_fs, at_fs=None):
    """{Z: dict(t [lags] fs, D [lags], value)} per species of the holder `vacf` present in the frame: the running Green-Kubo
    integral D_z(t) = (1/3) int_0^t C_z of the tracer curve C_z(k) = mean (v_i(s) - c_s).(v_i(s - k) - c) by the trapezoid rule,
    in Angstrom^2 / fs like transport.diffusion_constants (velocities are in Angstrom per ASE time unit), and its value at the
    lag nearest to at_fs (None: the last lag).  Lags without a pair of samples end the curve."""
    C = vacf.mean()["tracer"]
    t = vacf.lags * float(dt_fs)
    use = int(np.argmin(vacf.count > 0)) if not np.all(vacf.count > 0) else len(t)
    if use < 1:
        raise ValueError("green_kubo: the holder has no samples")
    step = vacf.every * float(dt_fs) * ASE_FS ** 2
    k = use - 1 if at_fs is None else int(np.argmin(np.abs(t[:use] - float(at_fs))))
    out = {}
    for q, z in enumerate(vacf.species):
        if vacf.n[q] == 0:
            continue
        D = _running_integral(C[:use, q], step) / 3.0
        out[int(z)] = dict(t=t[:use].copy(), D=D, value=float(D[k]))
    return out


def onsager(vacf, dt_fs):
    """(t [lags] fs, L [lags, S, S]): the running integrals L_ab(t) = (1 / 3N) int_0^t e_a(s).e_b(s - k) of the collective block
    (e_z: the species' current sum_z (v_i - c); N: the atoms of the frame), trapezoid rule, Angstrom^2 / fs — the Onsager
    coefficients behind an ionic conductivity; L_aa of a single tracer species is its Green-Kubo D."""
    col = vacf.mean()["collective"]
    use = int(np.argmin(vacf.count > 0)) if not np.all(vacf.count > 0) else len(vacf.lags)
    if use < 1:
        raise ValueError("onsager: the holder has no samples")
    step = vacf.every * float(dt_fs) * ASE_FS ** 2
    return vacf.lags[:use] * float(dt_fs), _running_integral(col[:use], step) / (3.0 * float(np.sum(vacf.n)))


def vibrational_dos(vacf, dt_fs, window="hann"):
    """(f [lags] THz, {Z: g [lags]}): the cosine transform of the normalised tracer curve C_z(k) / C_z(0),
        g(f_j) = sum_k a_k w_k C_z(k) / C_z(0) cos(2 pi f_j t_k),   f_j = j / (2 L every dt),   a_0 = 1/2, else 1,
    with w the falling half of a Hann window (window="hann") or 1 (None): the vibrational density of states up to a factor."""
    C = vacf.mean()["tracer"]
    L = int(np.argmin(vacf.count > 0)) if not np.all(vacf.count > 0) else vacf.nlags
    if L < 2:
        raise ValueError("vibrational_dos: fewer than two lags with samples")
    if window not in ("hann", None):
        raise ValueError("vibrational_dos: window = 'hann' or None")
    k = np.arange(L)
    w = 0.5 * (1.0 + np.cos(np.pi * k / L)) if window == "hann" else np.ones(L)
    w[0] *= 0.5
    step_fs = vacf.every * float(dt_fs)
    f = k / (2.0 * L * step_fs) * 1e3   # 1 / fs = 1000 THz
    kern = np.cos(np.pi * np.outer(k, k) / L)   # [j, k]: 2 pi f_j t_k
    out = {}
    for q, z in enumerate(vacf.species):
        if vacf.n[q] == 0 or not C[0, q] > 0.0:
            continue
        out[int(z)] = kern @ (w * C[:L, q] / C[0, q])
    return f, out


class VanHove(_InLoop):
    """Holder of van Hove tables: ActiveCalculator.run_md(vanhove=VanHove(every, levels, rmax, rbins, tbins, pbins, dmax, dbins))
    fills it, as msd= fills an Msd; add(table) adds the tables of a run (SGPRModel.md_vanhove_table(), VanHoveCounts.table()) —
    the tables of several runs of one frame with the same settings add up, count by count.  displacement_histogram,
    self_van_hove, distinct_van_hove and non_gaussian read them."""
    md, twin_of, constant_cell = "md_vanhove", "VanHoveCounts", "displacements and pair distances are counted"

    def __init__(self, every, levels, rmax, rbins, tbins=1, pbins=1, dmax=None, dbins=0):
        self.every, self.levels, self.rmax = int(every), int(levels), float(rmax)
        self.rbins, self.tbins, self.pbins, self.dbins = int(rbins), int(tbins), int(pbins), int(dbins)
        self.dmax = float(dmax) if self.dbins else 0.0
        self.lags = self.every * 2 ** np.arange(self.levels, dtype=np.int64)   # in configurations
        self.count = np.zeros(self.levels, dtype=np.int64)
        self.samples = 0
        self.hist = self.over = self.distinct = self.species = self.n = self.volume = None

    def settings(self):
        return (self.every, self.levels, self.rmax, self.rbins, self.tbins, self.pbins, self.dmax, self.dbins)

    def add(self, table):
        got = (int(table["every"]), int(table["levels"]), float(table["rmax"]), int(table["rbins"]), int(table["tbins"]), int(table["pbins"]),
               float(table["dmax"]), int(table["dbins"]))
        if got != self.settings():
            raise ValueError("VanHove.add: the table was taken with other settings (every, levels, rmax, bins, dmax)")
        species, n = np.asarray(table["species"]), np.asarray(table["n"])
        if self.species is None:
            self.species, self.n, self.volume = species.copy(), n.copy(), float(table["volume"])
            S = len(species)
            self.hist = np.zeros((self.levels, S, self.rbins, self.tbins, self.pbins), dtype=np.uint64)
            self.over = np.zeros((self.levels, S), dtype=np.uint64)
            self.distinct = np.zeros((self.levels, S, S, self.dbins), dtype=np.uint64)
        elif not (np.array_equal(species, self.species) and np.array_equal(n, self.n) and float(table["volume"]) == self.volume):
            raise ValueError("VanHove.add: the table is of another frame (species, atoms per species, volume)")
        self.hist = self.hist + np.asarray(table["self"], dtype=np.uint64)
        self.over = self.over + np.asarray(table["over"], dtype=np.uint64)
        self.distinct = self.distinct + np.asarray(table["distinct"], dtype=np.uint64)
        self.count = self.count + np.asarray(table["count"], dtype=np.int64)
        self.samples += int(table["samples"])
        return self

    def table(self):
        tab = dict(over=self.over.copy(), distinct=self.distinct.copy(), count=self.count.copy(), lags=self.lags.copy(), species=self.species,
                   n=self.n, samples=self.samples, next_due=self.samples * self.every, every=self.every, levels=self.levels, rmax=self.rmax,
                   rbins=self.rbins, tbins=self.tbins, pbins=self.pbins, dmax=self.dmax, dbins=self.dbins, volume=self.volume)
        tab["self"] = self.hist.copy()
        return tab

    def slot(self, species):
        """The slot of atomic number `species` in the table."""
        if self.species is None:
            raise ValueError("VanHove: the holder has no table")
        k = np.flatnonzero(self.species == int(species))
        if len(k) == 0 or self.n[k[0]] == 0:
            raise ValueError(f"VanHove: no atoms of species {species} in the frame")
        return int(k[0])


def _centres(lo, hi, bins):
    """The reference's axis: the edges linspace(lo, hi, bins + 1) less the last, plus half the first step."""
    a = np.linspace(lo, hi, bins + 1)
    return a[:-1] + (a[1] - a[0]) / 2


def displacement_histogram(vh, level, species):
    """(r [rbins], theta [tbins], phi [pbins], h [rbins, tbins, pbins], rho) — the return of the reference's
    TrajAnalyser.hist_rtp_displacements(delta = vh.lags[level], rmax, bins=[rbins + 1, tbins + 1, pbins + 1], select=species)
    with the level's non-overlapping windows for its random pairs: the bin centres, the histogram of the displacements over
    N windows, and the density N / V of the selected atoms (0 for a cell without volume)."""
    z = vh.slot(species)
    if vh.count[level] == 0:
        raise ValueError("displacement_histogram: the level has no window yet")
    h = vh.hist[level, z].astype(float) / (float(vh.n[z]) * float(vh.count[level]))
    rho = float(vh.n[z]) / vh.volume if vh.volume else 0.0
    return _centres(0.0, vh.rmax, vh.rbins), _centres(0.0, np.pi, vh.tbins), _centres(-np.pi, np.pi, vh.pbins), h, rho


def self_van_hove(vh):
    """(r [rbins], {Z: G [levels, rbins]}) per species present in the frame: the self part G_s(r, t_l) = P_l(k) / (4 pi r_k^2 dr),
    P_l(k) the fraction of the level's displacements in radial bin k (the table summed over the angles), at the bin centres r_k;
    4 pi int G_s r^2 dr = 1 less the fraction beyond rmax (vh.over).  nan where a level has no window."""
    if vh.hist is None:
        raise ValueError("self_van_hove: the holder has no table")
    r = _centres(0.0, vh.rmax, vh.rbins)
    shell = 4.0 * np.pi * r ** 2 * (vh.rmax / vh.rbins)
    c = np.where(vh.count > 0, vh.count, 1).astype(float)[:, None]
    out = {}
    for z, Z in enumerate(vh.species):
        if vh.n[z] == 0:
            continue
        P = vh.hist[:, z].sum(axis=(2, 3)).astype(float) / (float(vh.n[z]) * c)
        out[int(Z)] = np.where(vh.count[:, None] > 0, P / shell, np.nan)
    return r, out


def distinct_van_hove(vh):
    """(r [dbins], {(Za, Zb): G [levels, dbins]}) for every ordered pair of species present in the frame: the distinct part over
    the density of b, G_d(r, t_l) / rho_b = H[l][a][b][k] / (windows n_a 4 pi r_k^2 dr n_b / V) — a (origin) at time 0, b at
    t_l; at t -> 0 the g_ab(r) of transport.radial_distribution, at large t and r it tends to 1."""
    if vh.hist is None or not vh.dbins:
        raise ValueError("distinct_van_hove: the holder has no distinct part (dbins > 0)")
    r = _centres(0.0, vh.dmax, vh.dbins)
    shell = 4.0 * np.pi * r ** 2 * (vh.dmax / vh.dbins)
    c = np.where(vh.count > 0, vh.count, 1).astype(float)[:, None]
    out = {}
    for a, Za in enumerate(vh.species):
        for b, Zb in enumerate(vh.species):
            if vh.n[a] == 0 or vh.n[b] == 0:
                continue
            G = vh.distinct[:, a, b].astype(float) / (c * float(vh.n[a]) * shell * (float(vh.n[b]) / vh.volume))
            out[(int(Za), int(Zb))] = np.where(vh.count[:, None] > 0, G, np.nan)
    return r, out


def non_gaussian(vh):
    """{Z: alpha_2 [levels]} per species present in the frame: alpha_2(t_l) = 3 <r^4> / (5 <r^2>^2) - 1 of the level's
    displacements, 0 for a Gaussian (flow), positive where a few atoms hop while the rest rattle.  BINNED: the moments are taken
    from the radial marginal at the bin centres, with a relative error O((dr / r)^2) in each, and displacements beyond rmax
    (vh.over) are left out — choose rmax so that `over` stays empty.  nan where a level has no window or no displacement."""
    if vh.hist is None:
        raise ValueError("non_gaussian: the holder has no table")
    r = _centres(0.0, vh.rmax, vh.rbins)
    out = {}
    for z, Z in enumerate(vh.species):
        if vh.n[z] == 0:
            continue
        P = vh.hist[:, z].sum(axis=(2, 3)).astype(float)
        tot = P.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            m2, m4 = (P * r ** 2).sum(axis=1) / tot, (P * r ** 4).sum(axis=1) / tot
            out[int(Z)] = 3.0 * m4 / (5.0 * m2 * m2) - 1.0
    return out


def q_vectors(cell, qmax, limit=8192):
    """hkl int [nq, 3]: every integer triple whose vector of the reciprocal lattice q = 2 pi hkl inv(cell)^T has 0 < |q| <= qmax,
    one of each +- pair — the one whose first non-zero index is positive —, ordered by |q|, then by the triple: what
    SGPRModel.md_sq, workloads.SqRing and Sq take.  More than `limit` (the accumulator's 8192): ValueError."""
    h = np.asarray(cell, float).reshape(3, 3)
    rec = 2.0 * np.pi * np.linalg.inv(h).T     # (rows: the reciprocal vectors b_a; q = hkl @ rec)
    # h_a = q . a_a / 2 pi: |h_a| <= qmax |a_a| / 2 pi
    top = [int(np.floor(float(qmax) * np.linalg.norm(h[a]) / (2.0 * np.pi) + 1e-9)) for a in range(3)]
    grid = np.stack(np.meshgrid(*[np.arange(-t, t + 1) for t in top], indexing="ij"), axis=-1).reshape(-1, 3)
    first = np.where(grid[:, 0] != 0, grid[:, 0], np.where(grid[:, 1] != 0, grid[:, 1], grid[:, 2]))
    grid = grid[first > 0]
    q = np.linalg.norm(grid @ rec, axis=1)
    keep = q <= float(qmax)
    grid, q = grid[keep], q[keep]
    if len(grid) > int(limit):
        raise ValueError(f"q_vectors: {len(grid)} wave vectors within qmax = {qmax:g}; at most {int(limit)}")
    order = np.lexsort((grid[:, 2], grid[:, 1], grid[:, 0], q))
    return grid[order].astype(np.int64)


class Sq(_InLoop):
    """Holder of structure-factor tables: ActiveCalculator.run_md(sq=Sq(every, hkl, lags, origin_every)) fills it, as msd= fills
    an Msd; `hkl` int [nq, 3] names the wave vectors (q_vectors).  add(table) adds the tables of a run (SGPRModel.md_sq_table(),
    SqRing.table()) — those of several runs of one frame with equal settings add up.  structure_factor, intermediate_scattering
    and dynamic_structure_factor read it."""
    md, twin_of, constant_cell = "md_sq", "SqRing", "the wave vectors are the reciprocal lattice"

    def __init__(self, every, hkl, lags=1, origin_every=1):
        self.every, self.nlags, self.origin_every = int(every), int(lags), int(origin_every)
        self.hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3).copy()
        self.lags = self.every * np.arange(self.nlags, dtype=np.int64)   # in configurations
        self.count = np.zeros(self.nlags, dtype=np.int64)
        self.samples = 0
        self.f = self.mean = self.q = self.species = self.n = None

    def settings(self):
        return (self.every, self.hkl, self.nlags, self.origin_every)

    def add(self, table):
        if not (np.array_equal(np.asarray(table["lags"]), self.lags) and np.array_equal(np.asarray(table["hkl"]), self.hkl)
                and int(table["origin_every"]) == self.origin_every):
            raise ValueError("Sq.add: the table was taken with other settings (every, lags, origin_every, hkl)")
        species, n, q = np.asarray(table["species"]), np.asarray(table["n"]), np.asarray(table["q"], float)
        if self.species is None:
            self.species, self.n, self.q = species.copy(), n.copy(), q.copy()
            self.f = np.zeros((self.nlags, len(self.hkl), len(species), len(species)))
            self.mean = np.zeros((len(self.hkl), len(species)), dtype=complex)
        elif not (np.array_equal(species, self.species) and np.array_equal(n, self.n) and np.array_equal(q, self.q)):
            raise ValueError("Sq.add: the table is of another frame (species, atoms per species, cell)")
        self.count = self.count + np.asarray(table["count"], dtype=np.int64)
        self.f = self.f + np.asarray(table["f"], float)
        self.mean = self.mean + np.asarray(table["mean"], complex)
        self.samples += int(table["samples"])
        return self

    def table(self):
        if self.f is None:
            raise ValueError("Sq.table: the holder has no table")
        return dict(f=self.f.copy(), mean=self.mean.copy(), count=self.count.copy(), lags=self.lags.copy(), hkl=self.hkl.copy(), q=self.q,
                    species=self.species, n=self.n, origin_every=self.origin_every, samples=self.samples, next_due=self.samples * self.every)


def _sq_table(sq, who):
    t = sq.table() if hasattr(sq, "table") else sq
    if t.get("f") is None or int(t["count"][0]) == 0:
        raise ValueError(f"{who}: the table has no samples")
    return t


def _q_shells(q, dq):
    """(|q| per shell [nsh], the shell of every wave vector [nq]): dq None — the exact shells, vectors of one length (to nine
    digits); else bins [k dq, (k + 1) dq), the empty ones dropped, each at the mean length of its vectors."""
    qn = np.linalg.norm(np.asarray(q, float), axis=1)
    key = np.round(qn / qn.max(), 9) if dq is None else np.floor(qn / float(dq)).astype(np.int64)
    _, shell = np.unique(key, return_inverse=True)
    shell = shell.reshape(-1)
    return np.bincount(shell, weights=qn) / np.bincount(shell), shell


def _shell_mean(x, shell, axis):
    """The mean of x over the wave vectors of every shell, along `axis`."""
    x = np.moveaxis(np.asarray(x, float), axis, 0)
    out = np.zeros((int(shell.max()) + 1,) + x.shape[1:])
    np.add.at(out, shell, x)
    cnt = np.bincount(shell).astype(float).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.moveaxis(out / cnt, 0, axis)


def _al_norm(n):
    """sqrt(n_a n_b) [S, S] of the Ashcroft-Langreth partials; nan where a species has no atom in the frame."""
    n = np.asarray(n, float)
    r = np.sqrt(n[:, None] * n[None, :])
    return np.where(r > 0.0, r, np.nan)


def structure_factor(sq, weights=None, dq=None, diffuse=False):
    """(q [nsh], S) from an Sq holder or a table (md_sq_table(), SqRing.table()): the Ashcroft-Langreth partials
        S_ab(|q|) = f[0][j][a][b] / (count[0] sqrt(n_a n_b))
    averaged over the wave vectors of a shell — dq None: exact shells, vectors of equal length; else shells of width dq — as
    S [nsh, S, S] (nan for a species without atoms).  diffuse=True takes the Bragg part Re(<rho_a> conj <rho_b>) / sqrt(n_a n_b),
    <rho> = mean / samples, off every vector before the average: what is left is the diffuse scattering.  weights ({Z: w} or
    [S], scattering lengths or form factors at q = 0): the weighted total [nsh]
        S(q) = sum_ab w_a w_b sqrt(c_a c_b) S_ab(q) / sum_a c_a w_a^2,   c_a = n_a / N,
    which tends to 1 at large q."""
    t = _sq_table(sq, "structure_factor")
    n = np.asarray(t["n"], float)
    part = np.asarray(t["f"], float)[0] / float(t["count"][0])
    if diffuse:
        m = np.asarray(t["mean"], complex) / float(t["samples"])
        part = part - (m[:, :, None] * np.conj(m)[:, None, :]).real
    qs, shell = _q_shells(t["q"], dq)
    S = _shell_mean(part, shell, 0) / _al_norm(n)[None]
    if weights is None:
        return qs, S
    w = np.array([float(weights.get(int(z), 0.0)) for z in t["species"]]) if hasattr(weights, "get") else np.asarray(weights, float)
    c = n / n.sum()
    ww = (w[:, None] * w[None, :]) * np.sqrt(c[:, None] * c[None, :])
    return qs, np.nansum(np.where(ww[None] != 0.0, ww[None] * S, 0.0), axis=(1, 2)) / float(np.sum(c * w * w))


def intermediate_scattering(sq, dq=None):
    """(q [nsh], t [lags] in configurations, F [lags, nsh, S, S], Fn [lags, nsh, S, S]): the coherent intermediate scattering
    functions F_ab(|q|, t_k) = f[k][j][a][b] / (count[k] sqrt(n_a n_b)) averaged over the shells of structure_factor (a at time
    t, b at the origin: not symmetric in a, b at t > 0), and Fn = F / F(t = 0), the normalised decay.  nan where a lag has no
    pair of samples."""
    t = _sq_table(sq, "intermediate_scattering")
    cnt = np.asarray(t["count"])
    c = np.where(cnt > 0, cnt, 1).astype(float)[:, None, None, None]
    qs, shell = _q_shells(t["q"], dq)
    F = _shell_mean(np.asarray(t["f"], float) / c, shell, 1) / _al_norm(t["n"])[None, None]
    F = np.where((cnt > 0)[:, None, None, None], F, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        Fn = F / F[0][None]
    return qs, np.asarray(t["lags"]).copy(), F, Fn


def dynamic_structure_factor(sq, dt_fs, window="hann"):
    """(f [L] THz, q [nsh], S [L, nsh, S, S]): the cosine transform over the lags that have samples of the intermediate scattering
    functions on exact shells, windowed as vibrational_dos:
        S_ab(q, f_j) = 2 step sum_k a_k w_k F_ab(q, t_k) cos(2 pi f_j t_k),   f_j = j / (2 L step),  a_0 = 1/2, else 1,
    step = every dt_fs, w the falling half of a Hann window (window="hann") or 1 (None); in fs."""
    if window not in ("hann", None):
        raise ValueError("dynamic_structure_factor: window = 'hann' or None")
    qs, lags, F, _ = intermediate_scattering(sq, None)
    t = _sq_table(sq, "dynamic_structure_factor")
    cnt = np.asarray(t["count"])
    L = int(np.argmin(cnt > 0)) if not np.all(cnt > 0) else len(cnt)
    if L < 2:
        raise ValueError("dynamic_structure_factor: fewer than two lags with samples")
    k = np.arange(L)
    w = 0.5 * (1.0 + np.cos(np.pi * k / L)) if window == "hann" else np.ones(L)
    w[0] *= 0.5
    step_fs = float(lags[1] - lags[0]) * float(dt_fs)
    f = k / (2.0 * L * step_fs) * 1e3   # 1 / fs = 1000 THz
    kern = np.cos(np.pi * np.outer(k, k) / L)   # [j, k]: 2 pi f_j t_k
    return f, qs, 2.0 * step_fs * np.einsum("jk,k,kqab->jqab", kern, w, F[:L])
