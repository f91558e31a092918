// md_host.inc — the host side of the device-resident loops (sgpr_md_*), included by api.hip behind the step's entry points.
// One run at a time per handle (MdRun, api.hip), begun by sgpr_md_begin and shaped by the attach functions, one per mode:
// sgpr_md_thermostat (Nose-Hoover), _barostat (the moving cell), _relax (FIRE on atoms and cell; _relax_lbfgs: L-BFGS in its place), _fix (held components),
// _filter (model-update jumps), _meta and _meta_merge (metadynamics), _record (frames), _msd (displacements), _rdf (pair distances), _vacf (velocity correlations), _vanhove (displacement and pair histograms per lag), _adf (bond angles and coordination), _sq (structure factors and F(q, t)), _committee (the Bayesian committee), _neb
// (the nudged elastic band), _pimd (the ring polymer).  sgpr_md_run drives dynamics itself and hands a relaxation and a committee
// to md_relax_run and md_committee_run, a band and a polymer — R replicas evaluated by the one handle — to md_replica_run with
// the mode's three launches (md_neb_run, md_pimd_run); the four share the look-ahead driver and the frame of a call (MdCall).
// The kernels are in api.hip, md_npt.inc, md_relax.inc, md_record.inc, md_msd.inc, md_rdf.inc, md_vacf.inc, md_vanhove.inc, md_adf.inc, md_sq.inc, md_bcm.inc, md_neb.inc, md_pimd.inc and md_meta.inc (the
// one small kernel of sgpr_md_filter_push stands beside it, further down).
//
// The reference integrates in ASE (cl/md.py:117-128: ase.md.langevin.Langevin around ActiveCalculator; velocities
// from util/aseutil.py:11-20) and crosses into the calculator once per step.  Here the state (positions, velocities)
// lives in HBM, the integrator is part of the step's last kernel (finalize_next_kernel<2>), and the host reads a few
// scalars per step; the covloss gate of calculate() (calculator/active.py:492-499) halts the run ON THE DEVICE at the
// step whose largest covloss reaches `ediff`, with that step's state and results intact for the model update.
static int md_alloc(sgpr_model *h, int N)
{
    MdState &m = h->md;
    bool bad = false;
    bad |= m.X.alloc((size_t)12 * N); bad |= m.V.alloc((size_t)12 * N); bad |= m.P.alloc(4 * (size_t)sgpr_packed_len(N));
    bad |= m.KE.alloc((size_t)8 * N); bad |= m.mass.alloc(N); bad |= m.sig.alloc(N); bad |= m.cell.alloc(9);
    bad |= m.halt.alloc(4); bad |= m.zeta.alloc(8);
    if (bad) return fail(SGPR_E_NODEVICE, "sgpr_md_begin: device allocation failed");
    if (!m.halt_host.p && m.halt_host.alloc_mapped(16)) return fail(SGPR_E_NODEVICE, "sgpr_md_begin: no mapped host memory");
    return SGPR_OK;
}

// Is the handle bound to this system (pbc = NULL: periodic in all three directions)?
static bool md_same_system(const sgpr_model *h, int N, const int32_t *numbers, const int32_t *pbc, int rank, int world)
{
    bool same = (N == h->N && h->rank == rank && h->world == world && (int)h->numbers.size() == N);
    for (int i = 0; i < N && same; i++) same = h->numbers[i] == numbers[i];
    for (int k = 0; k < 3 && same; k++) same = h->pbc[k] == (pbc ? (pbc[k] != 0) : 1);
    return same;
}

// Whatever ran on the handle since sgpr_md_begin (a model update computes the training rows of stored frames and trial models
// evaluate them: each rebinds the handle) — the run's own system is bound again before it goes on (warm = false: the checked
// pass of the run functions)
static int md_rebind(sgpr_model *h)
{
    const MdState &m = h->md;
    if (md_same_system(h, m.run.N, m.run.numbers.data(), m.run.pbc, m.run.rank, m.run.world)) return SGPR_OK;
    return sgpr_bind_system(h, m.run.N, m.run.numbers.data(), m.run.pbc, m.run.rank, m.run.world);
}

// ---- the accumulators of the MD loop: one row each, in the order their launches follow an evaluation.  The attach functions
// (md_acc_run | md_acc_unstarted | md_acc_modes), the modes that exclude them (md_acc_attached) and the run loop
// (md_sample_due) read this table; a further accumulator adds a row, a sampler and its own attach body. ----
static int md_msd_sample(sgpr_model *h, int j, int step, hipStream_t st);
static int md_rdf_sample(sgpr_model *h, int j, int step, hipStream_t st);
static int md_vacf_sample(sgpr_model *h, int j, int step, hipStream_t st);
static int md_vh_sample(sgpr_model *h, int j, int step, hipStream_t st);
static int md_adf_sample(sgpr_model *h, int j, int step, hipStream_t st);
static int md_sq_sample(sgpr_model *h, int j, int step, hipStream_t st);
struct MdAcc {
    const char *fn, *noun;      // the attach function; what it accumulates, as the messages name it
    const char *moving_cell;    // why a barostat and the accumulator exclude each other
    const char *polymer;        // what of a ring polymer it would have to sample: "... not sampled"
    int (*every)(const MdRun &);
    int (*sample)(sgpr_model *h, int j, int step, hipStream_t st);   // the launches behind evaluation j of a call
};
static const MdAcc MD_ACC[] = {
    {"sgpr_md_msd", "displacements", "a displacement in a moving cell mixes in the strain", "centroid is",
     [](const MdRun &r) { return r.msd.every; }, md_msd_sample},
    {"sgpr_md_rdf", "pair distances", "the image block and the densities are those of a constant cell", "beads are",
     [](const MdRun &r) { return r.rdf.every; }, md_rdf_sample},
    {"sgpr_md_vacf", "velocity correlations", "velocities in a moving cell are not sampled", "centroid is",
     [](const MdRun &r) { return r.vacf.every; }, md_vacf_sample},
    {"sgpr_md_vanhove", "van Hove functions", "displacements and the image block are those of a constant cell", "beads are",
     [](const MdRun &r) { return r.vh.every; }, md_vh_sample},
    {"sgpr_md_adf", "bond angles", "the neighbours are read from the list of a constant cell", "beads are",
     [](const MdRun &r) { return r.adf.every; }, md_adf_sample},
    {"sgpr_md_sq", "structure factors", "the wave vectors are the reciprocal lattice of a constant cell", "beads are",
     [](const MdRun &r) { return r.sq.every; }, md_sq_sample},
};
enum { MD_MSD, MD_RDF, MD_VACF, MD_VH, MD_ADF, MD_SQ };

// The first accumulator attached to the run (NULL: none): what a mode that excludes them refuses with.
static const MdAcc *md_acc_attached(const MdRun &r)
{
    for (const MdAcc &a : MD_ACC)
        if (a.every(r)) return &a;
    return nullptr;
}

// The refusals every attach function shares, in three steps (an attach function puts its own argument checks between them where
// a caller can tell the order): a handle with a run; a run that has not started; a run of no mode that excludes the accumulators.
static int md_acc_run(const sgpr_model *h, const MdAcc &a)
{
    if (!h) return fail(SGPR_E_INVALID, "%s: bad arguments", a.fn);
    if (!h->md.active) return fail(SGPR_E_INVALID, "%s: call sgpr_md_begin first", a.fn);
    return SGPR_OK;
}
static int md_acc_unstarted(const sgpr_model *h, const MdAcc &a)
{
    if (h->md.run.t != 0 || h->md.run.started) return fail(SGPR_E_INVALID, "%s: the run has started", a.fn);
    return SGPR_OK;
}
static int md_acc_modes(const sgpr_model *h, const MdAcc &a)
{
    const MdRun &r = h->md.run;
    if (r.world > 1) return fail(SGPR_E_UNSUPPORTED, "%s: the run was begun on %d ranks; %s are accumulated on one", a.fn, r.world, a.noun);
    if (r.npt.on) return fail(SGPR_E_UNSUPPORTED, "%s: the run has a barostat; %s", a.fn, a.moving_cell);
    if (!r.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "%s: the run has a committee (sgpr_md_committee), whose loop does not sample %s", a.fn, a.noun);
    if (r.relax.on) return fail(SGPR_E_UNSUPPORTED, "%s: the run is a relaxation; %s are accumulated over dynamics", a.fn, a.noun);
    if (r.neb.on) return fail(SGPR_E_UNSUPPORTED, "%s: the run is a nudged elastic band; %s are accumulated over dynamics", a.fn, a.noun);
    if (r.pimd.on) return fail(SGPR_E_UNSUPPORTED, "%s: the run is a ring polymer (sgpr_md_pimd); its %s not sampled", a.fn, a.polymer);
    return SGPR_OK;
}

// Give a group of device buffers back, if it holds any: behind whatever the stream still runs, by a move-assign of the empty
// group.  The memory goes whatever the wait says.
template <typename Bufs>
static int md_release(sgpr_model *h, Bufs &b)
{
    if (!b.held()) return SGPR_OK;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    b = Bufs();
    return e == hipSuccess ? SGPR_OK : fail(SGPR_E_NODEVICE, "md_release: %s", hipGetErrorString(e));
}

// The run's sorted atoms by species of the model's table (the sort is by species in table order; anything else is `who`'s
// failure): nz[z] atoms from first[z] on.  With width > 0 also the chunks — runs of at most `width` consecutive atoms of one
// species, one record (first atom, atoms[, species]) each in `tab`; coff[z] ... coff[z + 1]: the chunks of species z.
struct MdSpecies {
    std::vector<int> nz, first, coff, tab;
    int nch = 0;
};
static int md_species_chunks(const sgpr_model *h, const char *who, int width, bool with_species, MdSpecies &s)
{
    const MdRun &r = h->md.run;
    const int S = h->S;
    s.nz.assign(S, 0); s.first.assign(S, 0); s.coff.assign(S + 1, 0);
    for (int i = 0, last = 0; i < r.N; i++) {
        int z = 0;
        while (z < S && h->species[z] != r.numbers[r.perm[i]]) z++;
        if (z == S || z < last) return fail(SGPR_E_INVALID, "%s: the run's atoms are not sorted by the model's species", who);
        last = z; s.nz[z]++;
    }
    for (int z = 1; z < S; z++) s.first[z] = s.first[z - 1] + s.nz[z - 1];
    for (int z = 0; z < S; z++) {
        for (int o = 0; width > 0 && o < s.nz[z]; o += width, s.nch++) {
            s.tab.push_back(s.first[z] + o); s.tab.push_back(std::min(width, s.nz[z] - o));
            if (with_species) s.tab.push_back(z);
        }
        s.coff[z + 1] = s.nch;
    }
    return SGPR_OK;
}

// The tile pairs of a pair sweep, RDF_PAIR ints each, appended to `tab`: tiles are runs of at most RDF_TILE atoms of one species;
// ordered: every ordered pair of tiles, weight 1 (the distinct part of the van Hove functions); else the pairs I <= J, an
// off-diagonal pair of one species with weight 2 (the radial distributions).  Returns the number of pairs.
static int md_tile_pairs(const std::vector<int> &nz, const std::vector<int> &first, bool ordered, std::vector<int> &tab)
{
    const int S = (int)nz.size();
    int npairs = 0;
    for (int a = 0; a < S; a++)
        for (int oa = 0; oa < nz[a]; oa += RDF_TILE)
            for (int b = ordered ? 0 : a; b < S; b++)
                for (int ob = (!ordered && b == a) ? oa : 0; ob < nz[b]; ob += RDF_TILE, npairs++) {
                    const int rec[RDF_PAIR] = {first[a] + oa, std::min(RDF_TILE, nz[a] - oa), first[b] + ob, std::min(RDF_TILE, nz[b] - ob),
                                               a * S + b, (!ordered && a == b && ob != oa) ? 2 : 1};
                    tab.insert(tab.end(), rec, rec + RDF_PAIR);
                }
    return npairs;
}

// The levels of md_msd's scheme that sample s closes (level l: lag 2^l samples, due when 2^l divides s), as a mask; *ndue:
// how many.
static unsigned md_due_levels(long long s, int levels, int *ndue)
{
    unsigned due = 0;
    int n = 0;
    for (int l = 0; l < levels && (s & ((1ll << l) - 1)) == 0; l++, n++) due |= 1u << l;
    if (ndue) *ndue = n;
    return due;
}

extern "C" int sgpr_md_begin(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                             const int32_t *pbc, const double *masses, const double *velocities, double dt,
                             double friction, double kT)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_begin: bad arguments");
    // The new run is put in place at the very end, whole: whatever fails on the way leaves the handle with NO run (the rings of
    // the earlier one are overwritten from md_alloc on), and the other entry points answer "call sgpr_md_begin first".
    MdState &m = h->md;
    m.active = false;
    if (N <= 0 || !numbers || !positions || !cell)   // (masses = NULL: ones — a relaxation, sgpr_md_relax, has no use for them)
        return fail(SGPR_E_INVALID, "sgpr_md_begin: bad arguments");
    if (!(dt > 0.0) || friction < 0.0 || kT < 0.0) return fail(SGPR_E_INVALID, "sgpr_md_begin: dt > 0, friction >= 0, kT >= 0");
    HIPCHK(hipSetDevice(h->device));
    // with the library's own exchange attached the run is sharded over its ranks (every rank integrates all atoms from the
    // summed forces: shard_next_kernel); otherwise a single process
    const int tr = peer_on(h) ? h->peer.rank : 0, tw = peer_on(h) ? h->peer.world : 1;
    int rc_ = md_same_system(h, N, numbers, pbc, tr, tw) ? SGPR_OK : sgpr_bind_system(h, N, numbers, pbc, tr, tw);
    if (rc_) return rc_;
    rc_ = md_alloc(h, N);
    if (rc_) return rc_;
    MdRun run;   // (every mode off, every setting at its default: no mode is named here)
    run.numbers.assign(numbers, numbers + N);
    run.perm = h->perm;
    for (int k = 0; k < 3; k++) run.pbc[k] = pbc ? (pbc[k] != 0) : 1;
    run.rank = tr; run.world = tw;
    run.N = N; run.dt = dt; run.hdt = 0.5 * dt; run.c1 = exp(-friction * dt);
    const double c2 = sqrt(1.0 - run.c1 * run.c1);
    std::vector<double> xs((size_t)3 * N), vs((size_t)3 * N, 0.0), ms(N), sg(N);
    for (int i = 0; i < N; i++) {
        const int c = h->perm[i];
        for (int k = 0; k < 3; k++) {
            xs[3 * (size_t)i + k] = positions[3 * (size_t)c + k];
            if (velocities) vs[3 * (size_t)i + k] = velocities[3 * (size_t)c + k];
        }
        ms[i] = masses ? masses[c] : 1.0;
        if (!(ms[i] > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_begin: mass of atom %d is not positive", c);
        sg[i] = friction > 0.0 ? c2 * sqrt(kT / ms[i]) : 0.0;   // (as workloads.langevin_nvt: c2 * np.sqrt(kT / mass))
    }
    HIPCHK(hipMemcpy(m.X.p, xs.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.V.p, vs.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.mass.p, ms.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.sig.p, sg.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.cell.p, cell, sizeof(double) * 9, hipMemcpyHostToDevice));
    run.mass_sorted = std::move(ms);
    m.run = std::move(run);
    m.active = true;
    h->pre_valid = false;
    return SGPR_OK;
}

// Held atoms and components for the run begun by sgpr_md_begin: fixed3N[N][3] in caller atom order, nonzero = that Cartesian
// component of that atom is held (ase.constraints.FixAtoms: all three of an atom; FixCartesian: the chosen ones).  NULL or all
// zeros: nothing is held, the run is the one without this call.  Inside the device loops (finalize_next_kernel<4>,
// shard_next_kernel<4>, the FIX forms of md_relax.inc) a held component
//   * is integrated / optimised with F = 0 — the forces REPORTED (packed, sgpr_md_state) stay the model's;
//   * has velocity exactly 0 from here on (the value given to sgpr_md_begin is dropped), in sgpr_md_velocities too;
//   * draws no Langevin noise (the free components draw what they draw without a mask: the deviates are counter-based);
//   * keeps its coordinate, selected explicitly: at constant cell the bits uploaded; in a relaxation with a moving cell the
//     undeformed coordinate r is what is held and x = r D^T follows the cell.
// Degrees of freedom g = 3N - n_fixed: sgpr_md_thermostat then uses tfact = 2 / (g kT ttime^2) and K0 = g kT / 2.
// After sgpr_md_begin; before sgpr_md_thermostat, sgpr_md_relax and the first sgpr_md_run (SGPR_E_INVALID otherwise, and
// when every component is held).  sgpr_md_barostat behind a non-empty mask: SGPR_E_UNSUPPORTED.
extern "C" int sgpr_md_fix(sgpr_model *h, const uint8_t *fixed3N)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_fix: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_fix: call sgpr_md_begin first");
    if (m.run.nh.on || m.run.npt.on || m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_fix: call it before sgpr_md_thermostat and sgpr_md_relax");
    if (m.run.neb.on) return fail(SGPR_E_INVALID, "sgpr_md_fix: call it before sgpr_md_neb");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_fix: the run is a ring polymer (sgpr_md_pimd), which runs without a mask");
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_fix: the run has started");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_fix: the run has a committee (sgpr_md_committee), which runs without a mask");
    const int N = m.run.N;
    std::vector<unsigned char> fs((size_t)3 * N, 0);
    int n = 0;
    if (fixed3N)
        for (int i = 0; i < N; i++)
            for (int k = 0; k < 3; k++)
                if (fixed3N[3 * (size_t)m.run.perm[i] + k]) { fs[3 * (size_t)i + k] = 1; n++; }
    if (n == 3 * N) return fail(SGPR_E_INVALID, "sgpr_md_fix: every component is held, nothing is left to move");
    if (n == 0) { m.run.fix.n = 0; m.run.fix.sorted.clear(); return SGPR_OK; }
    HIPCHK(hipSetDevice(h->device));
    if (m.fixed.mask.alloc((size_t)3 * N)) return fail(SGPR_E_NODEVICE, "sgpr_md_fix: device allocation failed");
    HIPCHK(hipMemcpy(m.fixed.mask.p, fs.data(), (size_t)3 * N, hipMemcpyHostToDevice));
    std::vector<double> v((size_t)3 * N);
    HIPCHK(hipMemcpy(v.data(), m.V.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < (size_t)3 * N; e++)
        if (fs[e]) v[e] = 0.0;
    HIPCHK(hipMemcpy(m.V.p, v.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    m.run.fix.n = n;
    m.run.fix.sorted = fs;
    return SGPR_OK;
}

// Nose-Hoover NVT for the run begun by sgpr_md_begin (kind = 1; 0 = back to the Langevin / velocity-Verlet step of
// sgpr_md_begin's friction): what the reference's default md(dynamics="NPT", bulk_modulus=None) is — ase.md.npt.NPT with
// pfactor = None and ttime = tdamp fs (cl/md.py:17, :131-166) — restated in md_nh_advance / md_nh_kernel.  kT as given to
// sgpr_md_begin; tfact = 2 / (3 N kT ttime^2), desired kinetic energy 1.5 (N - 1) kT (ASE's constants).  Before the first
// sgpr_md_run of the run.
extern "C" int sgpr_md_thermostat(sgpr_model *h, int kind, double ttime, double kT)
{
    if (!h || (kind != 0 && kind != 1)) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: kind is 0 (Langevin / velocity Verlet) or 1 (Nose-Hoover)");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: call sgpr_md_begin first");
    if (m.run.t != 0) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: the run has started");
    if (m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: the run is a relaxation (sgpr_md_relax)");
    if (m.run.neb.on) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: the run is a nudged elastic band (sgpr_md_neb)");
    if (m.run.pimd.on) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: the run is a ring polymer (sgpr_md_pimd), which has its own thermostat");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: call it before sgpr_md_committee");
    if (kind == 0) { m.run.nh.on = false; m.run.npt.on = false; m.run.ring = 3; return SGPR_OK; }
    if (!(ttime > 0.0) || !(kT > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_thermostat: ttime > 0 and kT > 0");
    // (held components, sgpr_md_fix: g = 3N - n_fixed degrees of freedom, none removed for the centre of mass — momentum is
    // not conserved beside a held atom; the project's own definition, ASE's NPT takes no constraints)
    const double g = (double)(3 * m.run.N - m.run.fix.n);
    const double tfact = 2.0 / (g * kT * ttime * ttime);
    m.run.nh.on = true; m.run.ring = 4;
    m.run.nh.c1 = m.run.dt * tfact; m.run.nh.c2 = 2.0 * m.run.dt * tfact; m.run.nh.K0 = m.run.fix.n ? 0.5 * g * kT : 1.5 * (double)(m.run.N - 1) * kT;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemset(m.zeta.p, 0, 8 * sizeof(double)));
    return SGPR_OK;
}

// A barostat for the Nose-Hoover run (sgpr_md_thermostat(kind = 1) first, before the first sgpr_md_run): ase.md.npt.NPT with
// a pfactor, the moving cell of cl/md.py:131-166 — md_npt.inc has the scheme.  The cell of sgpr_md_begin must be upper
// triangular (ASE's own condition) and periodic in all three directions.  pfactor = ptime^2 x bulk modulus and the external
// stress (six Voigt components; a pressure P is (-P, -P, -P, 0, 0, 0)) in the units of the run; mask: nine zeros / ones (which
// cell components may move); frac_traceless: 1 = all of the strain rate (with the mask), 0 = its trace only (`iso`).
// Single rank only: the sharded last kernel (peer.inc) integrates at constant cell.  A run that has a committee
// (sgpr_md_committee, attached before or after this call) is refused unless the run's option "md_committee_cell" is set
// (sgpr_set_option after sgpr_md_begin): it then integrates the committee's forces and stress in the moving cell
// (md_committee_run); a bias or held components beside the barostat stay refused.
extern "C" int sgpr_md_barostat(sgpr_model *h, double pfactor, const double *externalstress, const double *mask, double frac_traceless)
{
    if (!h || !externalstress) return fail(SGPR_E_INVALID, "sgpr_md_barostat: bad arguments");
    MdState &m = h->md;
    if (m.active && m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: the run is a ring polymer (sgpr_md_pimd), which runs at constant cell");
    if (!m.active || !m.run.nh.on || m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_barostat: call sgpr_md_begin and sgpr_md_thermostat(kind = 1) first");
    if (m.run.t != 0 || m.run.npt.started) return fail(SGPR_E_INVALID, "sgpr_md_barostat: the run has started");
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: the run was begun on %d ranks; the moving cell runs on one", m.run.world);
    if (!m.run.bcm.members.empty() && !m.run.bcm.cell)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: the run has a committee (sgpr_md_committee), which runs at constant cell unless the run's option "
                    "md_committee_cell is set (sgpr_set_option)");
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: the run has a bias (sgpr_md_meta), which runs at constant cell; the host loop around calculate() serves a biased NPT run");
    if (m.run.fix.n) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: %d components are held (sgpr_md_fix); the moving cell runs without a mask", m.run.fix.n);
    if (const MdAcc *a = md_acc_attached(m.run)) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_barostat: the run accumulates %s (%s) at constant cell: %s", a->noun, a->fn, a->moving_cell);
    if (!(pfactor > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_barostat: pfactor > 0");
    if (!(m.run.pbc[0] && m.run.pbc[1] && m.run.pbc[2])) return fail(SGPR_E_INVALID, "sgpr_md_barostat: the cell must be periodic in all three directions");
    HIPCHK(hipSetDevice(h->device));
    double c[9];
    HIPCHK(hipMemcpy(c, m.cell.p, sizeof(c), hipMemcpyDeviceToHost));
    if (!(c[3] == 0.0 && c[6] == 0.0 && c[7] == 0.0))
        return fail(SGPR_E_INVALID, "sgpr_md_barostat: the cell must be upper triangular (h[1][0] = h[2][0] = h[2][1] = 0)");
    const double det = (c[0] * c[4]) * c[8];
    if (!(det > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_barostat: the cell's diagonal must be positive");
    if (m.npt.ring.alloc(4 * sizeof(NptSlot)) || m.npt.Q.alloc((size_t)12 * m.run.N)) return fail(SGPR_E_NODEVICE, "sgpr_md_barostat: device allocation failed");
    NptParams &p = m.run.npt.par;
    p = NptParams();
    p.dt = m.run.dt; p.c1 = m.run.nh.c1; p.c2 = m.run.nh.c2; p.K0 = m.run.nh.K0;
    p.pfact = 1.0 / (pfactor * det);
    for (int k = 0; k < 6; k++) p.ext[k] = externalstress[k];
    for (int k = 0; k < 9; k++) p.mask[k] = mask ? (mask[k] != 0.0 ? 1.0 : 0.0) : 1.0;
    p.frac = frac_traceless;
    for (int k = 0; k < 3; k++) p.pbc[k] = 1;
    m.run.npt.pfactor = pfactor;
    m.run.npt.on = true; m.run.npt.started = false;
    return SGPR_OK;
}

// Fixed-order sum of md_npt_kernel / md_nh_kernel on the host: 256 strided partial sums, then a pairwise tree
static double md_host_order_sum(const std::vector<double> &x)
{
    double p[256];
    for (int t = 0; t < 256; t++) p[t] = 0.0;
    for (size_t k = 0; k < x.size(); k++) p[k & 255] += x[k];
    for (int w = 256; w > 1; w >>= 1)
        for (int t = 0; t < w / 2; t++) p[t] = p[2 * t] + p[2 * t + 1];
    return p[0];
}

static int md_committee_forces0(sgpr_model *h, int spare_row, hipStream_t st, std::vector<double> &F);

// Start of a moving-cell trajectory (NPT.initialize(), autoforce_amd/npt.py): one synchronised evaluation of configuration 0,
// then q_0 = x_0 h^-1 - 1/2 and q_(-1) by the backward step that is corrected twice (with ASE's test on the mean kinetic
// energy per atom between the two corrections) on the host, in the operations of workloads.npt_moving_cell — once per
// trajectory.  eta_0 = zeta_0 = 0 and therefore h_(-1) = h_1 = h_0; eta_(-1), zeta_(-1) are md_npt_kernel's (n = 0).
// A run with a committee (bcm_row >= 0: the spare row of the call's scalar ring, md_committee_run): the forces of the backward
// step are the committee's — md_committee_forces0 —, as the host twin's calculator answers with them at configuration 0.
static int md_npt_start(sgpr_model *h, hipStream_t st, int bcm_row = -1)
{
#pragma clang fp contract(off)
    MdState &m = h->md;
    const int N = m.run.N;
    NptSlot s0 = {};
    HIPCHK(hipMemcpy(s0.h, m.cell.p, 9 * sizeof(double), hipMemcpyDeviceToHost));
    npt_matrices(m.run.npt.par.dt, s0.h, s0.eta, 0.0, s0.hinv, s0.bm1, s0.bp1inv);
    s0.thr2_keep = s0.thr2_reb = -1.0;
    HIPCHK(hipMemset(m.npt.ring.p, 0, 4 * sizeof(NptSlot)));
    HIPCHK(hipMemcpy(m.slot(0), &s0, sizeof(NptSlot), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.slot(1)->h, s0.h, 9 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(m.zeta.p, 0, 8 * sizeof(double)));
    const int rc_ = run_checked(h, m.X.p, m.slot(0)->h, m.P.p, st);
    if (rc_) return rc_;
    h->warm = true;
    std::vector<double> x((size_t)3 * N), v((size_t)3 * N), F((size_t)3 * N), q((size_t)3 * N), qp((size_t)3 * N), ke(N);
    HIPCHK(hipMemcpy(x.data(), m.X.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v.data(), m.V.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(F.data(), m.P.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));   // (packed forces: caller order)
    if (bcm_row >= 0)
        if (const int rb = md_committee_forces0(h, bcm_row, st, F)) return rb;
    if (m.run.filter.on) {   // the forces the integrator sees at configuration 0 (finalize_next_kernel<7>'s operations; slot 0 stays as it is)
        std::vector<double> a0((size_t)3 * N);
        HIPCHK(hipMemcpy(a0.data(), m.filter.f.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; i++)
            for (int k = 0; k < 3; k++) {
                const double an = a0[3 * (size_t)i + k] * m.run.filter.shrink;
                F[3 * (size_t)m.run.perm[i] + k] = F[3 * (size_t)m.run.perm[i] + k] - std::min(std::max(an, -1.0), 1.0);
            }
    }
    const double dt = m.run.npt.par.dt;
    auto row_mul = [](const double *r, const double *mat, double *o) {
#pragma clang fp contract(off)
        for (int k = 0; k < 3; k++) o[k] = (r[0] * mat[k] + r[1] * mat[3 + k]) + r[2] * mat[6 + k];
    };
    for (int i = 0; i < N; i++) {
        double t[3];
        row_mul(&x[3 * (size_t)i], s0.hinv, t);
        for (int k = 0; k < 3; k++) q[3 * (size_t)i + k] = t[k] - 0.5;
    }
    std::vector<double> vb = v;
    for (int pass = 0; pass < 2; pass++) {
        for (int i = 0; i < N; i++) {
            const int c = m.run.perm[i];
            const double ms = m.run.mass_sorted[i];
            const double *qi = &q[3 * (size_t)i];
            double *qpi = &qp[3 * (size_t)i];
            double t[3], a[3], al[3], num[3], qn[3], dq[3], vc[3];
            row_mul(&vb[3 * (size_t)i], s0.hinv, t);
            for (int k = 0; k < 3; k++) qpi[k] = qi[k] - dt * t[k];
            for (int k = 0; k < 3; k++) a[k] = ((dt * dt) * F[3 * (size_t)c + k]) / ms;
            row_mul(qpi, s0.bm1, t);
            row_mul(a, s0.hinv, al);
            for (int k = 0; k < 3; k++) num[k] = ((2.0 * qi[k]) + t[k]) + al[k];
            row_mul(num, s0.bp1inv, qn);
            for (int k = 0; k < 3; k++) dq[k] = qn[k] - qpi[k];
            row_mul(dq, s0.h, t);
            for (int k = 0; k < 3; k++) vc[k] = t[k] / (2.0 * dt);
            ke[i] = (ms * (vc[0] * vc[0]) + ms * (vc[1] * vc[1])) + ms * (vc[2] * vc[2]);
            for (int k = 0; k < 3; k++) vb[3 * (size_t)i + k] = (v[3 * (size_t)i + k] - vc[k]) + v[3 * (size_t)i + k];
        }
        if (0.5 * md_host_order_sum(ke) / N < 1e-5) break;
    }
    HIPCHK(hipMemcpy(m.npt.Q.p, q.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.npt.Q.p + (size_t)9 * N, qp.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    // the grids of h_0 and h_1 and the rebuild rule of evaluation 0 (which rebuilds: the first of its call)
    hipLaunchKernelGGL(md_npt_kernel, dim3(1), dim3(256), 0, st, N, m.run.npt.par, (NptSlot *)m.npt.ring.p, m.zeta.p, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)h->d_cell0.p, -1,
                       (const int *)m.halt.p, -1, (double *)nullptr, (double *)nullptr, (const double *)nullptr, (double *)nullptr, 0.0);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    m.run.npt.started = true;
    return SGPR_OK;
}

// Cell and strain rate of a moving-cell run, SGPR_MD_CELL = 18 doubles (h[9], eta[9]) per configuration `first` ...
// `first + count - 1` (indices of the trajectory: 0 = the configuration of sgpr_md_begin): those the last sgpr_md_run
// evaluated, and the current one — the cell sgpr_md_state's positions belong to.
extern "C" int sgpr_md_cells(sgpr_model *h, int64_t first, int count, double *out)
{
    if (!h || count <= 0 || !out) return fail(SGPR_E_INVALID, "sgpr_md_cells: bad arguments");
    MdState &m = h->md;
    if (!m.active || !(m.run.npt.on || m.run.relax.on)) return fail(SGPR_E_INVALID, "sgpr_md_cells: call sgpr_md_begin and sgpr_md_barostat (or sgpr_md_relax) first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long have = (long long)(m.run.npt.cells.size() / SGPR_MD_CELL);
    for (int r = 0; r < count; r++) {
        const long long n = (long long)first + r;
        double *o = out + (size_t)SGPR_MD_CELL * r;
        if (n >= m.run.npt.cells_first && n < m.run.npt.cells_first + have)
            memcpy(o, m.run.npt.cells.data() + (size_t)SGPR_MD_CELL * (n - m.run.npt.cells_first), sizeof(double) * SGPR_MD_CELL);
        else if (m.run.relax.on && n == m.run.t)   // a relaxation: the cell and, in the place of eta, the deformation gradient D
            HIPCHK(hipMemcpy(o, m.relax.cells.p + (size_t)RLX_CELL * (n % RLX_RING), RLX_CELL * sizeof(double), hipMemcpyDeviceToHost));
        else if (!m.run.relax.on && n == m.run.t && m.run.npt.started) {
            HIPCHK(hipMemcpy(o, m.slot(n)->h, 9 * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(o + 9, m.slot(n)->eta, 9 * sizeof(double), hipMemcpyDeviceToHost));
        } else if (!m.run.relax.on && n == 0 && m.run.t == 0) {
            HIPCHK(hipMemcpy(o, m.cell.p, 9 * sizeof(double), hipMemcpyDeviceToHost));
            for (int k = 0; k < 9; k++) o[9 + k] = 0.0;
        } else
            return fail(SGPR_E_INVALID, "sgpr_md_cells: configuration %lld is neither the current one (%lld) nor one of the last run's", n, m.run.t);
    }
    return SGPR_OK;
}

// FIRE relaxation for the run begun by sgpr_md_begin (whose masses, velocities, dt, friction and kT it ignores), before the
// first sgpr_md_run: the optimizer of ase/optimize/fire.py on the positions and, with move_cell, on the cell through
// ase.constraints.UnitCellFilter's coordinates — md_relax.inc has the scheme, workloads.fire_relax is the host twin.
// fire: dt, maxstep, dtmax, nmin, finc, fdec, astart, fa (NULL: ASE's defaults); mask6: which of the six Voigt components
// xx yy zz yz xz xy of the cell may move (NULL: all).  sgpr_md_run then evaluates, moves, and stops with halt code 3 at the
// first configuration whose largest generalised force is below fmax — the state IS that configuration, nothing moved.  Single
// rank only.
static const double RLX_ASE[8] = {0.1, 0.2, 1.0, 5.0, 1.1, 0.5, 0.1, 0.99};

// The eight FIRE keywords of sgpr_md_relax and sgpr_md_neb (`who`, for the message), checked and copied into p
static int md_fire_keywords(const char *who, const double *fire, RelaxParams &p)
{
    const double *fp = fire ? fire : RLX_ASE;
    if (!(fp[0] > 0.0 && fp[1] > 0.0 && fp[2] > 0.0 && fp[3] >= 0.0 && fp[4] > 0.0 && fp[5] > 0.0 && fp[6] >= 0.0 && fp[7] > 0.0))
        return fail(SGPR_E_INVALID, "%s: dt, maxstep, dtmax, finc, fdec, fa > 0 and nmin, astart >= 0", who);
    p.dt0 = fp[0]; p.maxstep = fp[1]; p.dtmax = fp[2]; p.nmin = fp[3]; p.finc = fp[4]; p.fdec = fp[5]; p.astart = fp[6]; p.fa = fp[7];
    return SGPR_OK;
}

static int md_relax_init_state(sgpr_model *h)
{
    MdState &m = h->md;
    double s[RLX_LEN] = {};
    HIPCHK(hipMemcpy(s, m.relax.state.p, sizeof(s), hipMemcpyDeviceToHost));
    s[RLX_DT] = m.run.relax.par.dt0; s[RLX_A] = m.run.relax.par.astart; s[RLX_NSTEPS] = 0.0; s[RLX_FRESH] = 1.0;
    for (int k = 0; k < 9; k++) s[RLX_VC + k] = 0.0;
    s[RLX_ALPHA] = s[RLX_BETA] = s[RLX_CD] = 0.0;
    HIPCHK(hipMemcpy(m.relax.state.p, s, sizeof(s), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(m.V.p, 0, sizeof(double) * 3 * (size_t)m.run.N));
    return SGPR_OK;
}

extern "C" int sgpr_md_relax(sgpr_model *h, double fmax, const double *fire, int move_cell, const double *mask6)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_relax: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_relax: call sgpr_md_begin first");
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run was begun on %d ranks; a relaxation runs on one", m.run.world);
    if (m.run.t != 0 || m.run.relax.started) return fail(SGPR_E_INVALID, "sgpr_md_relax: the run has started");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run has a committee (sgpr_md_committee), which serves dynamics only");
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run has a bias (sgpr_md_meta), which serves dynamics only; the host loop around calculate() serves a biased relaxation");
    if (m.run.filter.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run has a filter (sgpr_md_filter), which serves dynamics only");
    if (m.run.nh.on || m.run.npt.on) return fail(SGPR_E_INVALID, "sgpr_md_relax: the run has a thermostat or a barostat");
    if (m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run is a nudged elastic band (sgpr_md_neb), which has its own optimizer");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run is a ring polymer (sgpr_md_pimd), which serves dynamics only");
    if (const MdAcc *a = md_acc_attached(m.run)) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_relax: the run accumulates %s (%s), which serve dynamics only", a->noun, a->fn);
    if (!(fmax > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_relax: fmax > 0");
    RelaxParams p = {};
    if (const int rf = md_fire_keywords("sgpr_md_relax", fire, p)) return rf;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N;
    HIPCHK(hipMemcpy(p.h0, m.cell.p, sizeof(p.h0), hipMemcpyDeviceToHost));
    if (move_cell) {
        if (!(m.run.pbc[0] && m.run.pbc[1] && m.run.pbc[2])) return fail(SGPR_E_INVALID, "sgpr_md_relax: a cell that moves must be periodic in all three directions");
        if (!(fabs(rlx_det(p.h0)) > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_relax: the cell is singular");
    }
    p.fmax2 = fmax * fmax;
    double m6[6];
    for (int k = 0; k < 6; k++) m6[k] = mask6 ? (mask6[k] != 0.0 ? 1.0 : 0.0) : 1.0;
    const double M[9] = {m6[0], m6[5], m6[4], m6[5], m6[1], m6[3], m6[4], m6[3], m6[2]};
    for (int k = 0; k < 9; k++) p.mask[k] = M[k];
    p.cf = (double)N;
    p.cell = move_cell ? 1 : 0;
    // rings of RLX_RING slots, every slot a valid configuration from the start (what runs behind a halt evaluates stale slots)
    std::vector<double> x0((size_t)3 * N);
    HIPCHK(hipMemcpy(x0.data(), m.X.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
    if (m.X.alloc((size_t)3 * N * RLX_RING) || m.P.alloc((size_t)RLX_RING * (size_t)sgpr_packed_len(N)) || m.relax.state.alloc(RLX_LEN) ||
        m.relax.ref.alloc((size_t)3 * N) || m.relax.cells.alloc((size_t)RLX_RING * RLX_CELL))
        return fail(SGPR_E_NODEVICE, "sgpr_md_relax: device allocation failed");
    double slot[RLX_CELL] = {};
    for (int k = 0; k < 9; k++) { slot[k] = p.h0[k]; slot[9 + k] = (k % 4 == 0) ? 1.0 : 0.0; }
    for (int r = 0; r < RLX_RING; r++) {
        HIPCHK(hipMemcpy(m.X.p + (size_t)3 * N * r, x0.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m.relax.cells.p + (size_t)RLX_CELL * r, slot, sizeof(slot), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(m.relax.ref.p, x0.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    double s[RLX_LEN] = {};
    for (int k = 0; k < 9; k++) s[RLX_XC + k] = (k % 4 == 0) ? p.cf : 0.0;
    HIPCHK(hipMemcpy(m.relax.state.p, s, sizeof(s), hipMemcpyHostToDevice));
    m.run.relax.par = p;
    m.run.relax.on = true; m.run.relax.started = false; m.run.ring = RLX_RING;
    m.run.lbfgs = MdRun::Lbfgs();   // (FIRE, until sgpr_md_relax_lbfgs says otherwise)
    m.run.npt.cells.clear(); m.run.npt.cells_first = 0;
    return md_relax_init_state(h);
}

// optimizer.initialize(): v = 0 and dt, a, nsteps back to their start (the reference's relax(clear_hist=True) behind a model update)
extern "C" int sgpr_md_relax_reset(sgpr_model *h)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_relax_reset: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_relax_reset: call sgpr_md_begin and sgpr_md_relax first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    m.run.lbfgs.base = m.run.t;   // (L-BFGS: the history is indexed by evaluation — the next one is the first of an empty one)
    return md_relax_init_state(h);
}

// ---- L-BFGS in the place of FIRE (sgpr_md_relax_lbfgs; md_lbfgs.inc has the scheme, workloads.lbfgs_relax is the host twin) ----
// Everything but the history S | Y in one allocation, carved by md_lbfgs_buf in the order of LbfgsBuf's members.
static size_t md_lbfgs_work_len(int N, int mem)
{
    const size_t R3 = (size_t)3 * N + 9, B = (size_t)(N + 255) / 256, B3 = (size_t)(N + 3 + 63) / 64, M = (size_t)mem;
    return 3 * R3 + 3 * M * M + 2 * M + 4 * M * B + 3 * B + 3 * M + B3 + 18;
}

static LbfgsBuf md_lbfgs_buf(const MdState &m)
{
    const int N = m.run.N;
    const size_t R3 = (size_t)3 * N + 9, B = (size_t)(N + 255) / 256, B3 = (size_t)(N + 3 + 63) / 64, M = (size_t)m.run.lbfgs.mem;
    LbfgsBuf b;
    b.S = m.lbfgs.hist.p; b.Y = b.S + M * R3;
    double *w = m.lbfgs.work.p;
    b.G = w; w += 2 * R3;
    b.dir = w; w += R3;
    b.Rinv = w; w += M * M;
    b.RinvT = w; w += M * M;
    b.YY = w; w += M * M;
    b.Dg = w; w += M;
    b.valid = w; w += M;
    b.part = w; w += 4 * M * B;
    b.pgg = w; w += B;
    b.pgmx = w; w += B;
    b.pbmx = w; w += B;
    b.coef = w; w += 3 * M;
    b.pmax = w; w += B3;
    b.xc = w;
    return b;
}

// L-BFGS without line search in the place of FIRE for the relaxation set up by sgpr_md_relax (whose fmax, cell and mask hold; its
// FIRE keywords are not used), before the first sgpr_md_run: ase/optimize/lbfgs.py on the same generalised coordinates.
// memory: pairs kept at most, 1 ... 128; maxstep, alpha (H0 = 1 / alpha), damping: ASE's keywords (its defaults: 100, 0.2, 70,
// 1).  The history, 2 memory (3N + 9) doubles, is held until sgpr_md_end; sgpr_md_relax_reset empties it.  The scalar columns
// 12..15 of a row: largest |G_row|^2, p.G, the scale applied to the step, valid pairs in use.
extern "C" int sgpr_md_relax_lbfgs(sgpr_model *h, int memory, double maxstep, double alpha, double damping)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_relax_lbfgs: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_relax_lbfgs: call sgpr_md_begin and sgpr_md_relax first");
    if (m.run.t != 0 || m.run.relax.started) return fail(SGPR_E_INVALID, "sgpr_md_relax_lbfgs: the run has started");
    if (memory < 1 || memory > 128) return fail(SGPR_E_INVALID, "sgpr_md_relax_lbfgs: 1 <= memory <= 128");
    if (!(maxstep > 0.0 && alpha > 0.0 && damping > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_relax_lbfgs: maxstep, alpha, damping > 0");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N;
    if (m.lbfgs.hist.alloc((size_t)2 * memory * ((size_t)3 * N + 9)))
        return fail(SGPR_E_NODEVICE, "sgpr_md_relax_lbfgs: no device memory for a history of %d pairs (%zu doubles)", memory,
                    (size_t)2 * memory * ((size_t)3 * N + 9));
    if (m.lbfgs.work.alloc(md_lbfgs_work_len(N, memory))) return fail(SGPR_E_NODEVICE, "sgpr_md_relax_lbfgs: device allocation failed");
    m.run.lbfgs = MdRun::Lbfgs();
    m.run.lbfgs.on = true; m.run.lbfgs.mem = memory; m.run.lbfgs.maxstep = maxstep; m.run.lbfgs.h0 = 1.0 / alpha; m.run.lbfgs.damping = damping;
    double xc[18];
    for (int k = 0; k < 18; k++) xc[k] = ((k % 9) % 4 == 0) ? m.run.relax.par.cf : 0.0;   // (c D at the start, both slots)
    HIPCHK(hipMemcpy(md_lbfgs_buf(m).xc, xc, sizeof(xc), hipMemcpyHostToDevice));
    return SGPR_OK;
}

// ---- the look-ahead driver of the run functions (sgpr_md_run and md_relax_run, its form for a relaxation) ----
// The halt words are three ints in mapped host memory, each the step (h->step_count) of the evaluation that halted the run or
// MD_HALT_NONE: [0] the covloss gate, [1] a capacity overflow, [2] a relaxation's convergence (no MD kernel writes it); the
// device has its own copy of the first two (m.halt).  The earliest one halted the run.
static const int MD_HALT_NONE = 0x7fffffff;
static int md_halt_step(const MdState &m) { return std::min(std::min(m.halt_host.p[0], m.halt_host.p[1]), m.halt_host.p[2]); }

// For the length of a call the positions handed to the binning kernel are in sorted order already (the rings); on every way
// out the handle is an ordinary one again: no pre-binned configuration, no grid of a moving cell.
struct MdBinIdentity {
    sgpr_model *h;
    explicit MdBinIdentity(sgpr_model *h_) : h(h_) { h->bin_identity = true; }
    ~MdBinIdentity() { h->bin_identity = false; h->pre_valid = false; h->step_grid = nullptr; }
};

// Sets a call up: the scalar ring (device rows, a mapped mark word per evaluation, the page-locked buffer the rows are copied
// out to) grown to the call and zeroed, the per-evaluation cell record where the run has one (NPT, relaxation), the halts armed.
static int md_prepare_call(sgpr_model *h, int nevals, hipStream_t st, bool want_cells)
{
    MdState &m = h->md;
    // the frame record of this call (sgpr_md_record): room for the frames it can record, grown like the scalar ring and not
    // zeroed — before anything is enqueued
    m.run.rec.call_t0 = m.run.t; m.run.rec.call_every = m.run.rec.every; m.run.rec.call_what = m.run.rec.what; m.run.rec.call_count = 0;
    if (m.run.rec.every) {
        const size_t fr = (size_t)MdRun::rec_between(m.run.t, m.run.t + nevals, m.run.rec.every), N3 = (size_t)3 * m.run.N;
        if (m.rec.x.alloc(fr * N3, false) || ((m.run.rec.what & 1) && m.rec.v.alloc(fr * N3, false)) ||
            ((m.run.rec.what & 2) && m.rec.p.alloc(fr * (size_t)sgpr_packed_len(m.run.N), false)))
            return fail(SGPR_E_NODEVICE, "sgpr_md_run: no device memory for the record of %zu frames", fr);
    }
    const size_t rows = (size_t)nevals + 1;
    if (m.scal_rows < rows) {
        m.mark.release();
        m.scal_pin.release();
        m.scal_rows = 0;
        if (m.scal_d.alloc((size_t)SGPR_MD_SCAL * rows, false) || m.mark.alloc_mapped(rows) ||
            m.scal_pin.alloc_pinned((size_t)SGPR_MD_SCAL * rows))
            return fail(SGPR_E_NODEVICE, "sgpr_md_run: no memory for the scalar ring");
        m.scal_rows = rows;
    }
    HIPCHK(hipMemsetAsync(m.scal_d.p, 0, sizeof(double) * SGPR_MD_SCAL * rows, st));
    memset(m.mark.p, 0, sizeof(int) * rows);
    if (want_cells) {
        if (m.npt.cells_d.alloc((size_t)SGPR_MD_CELL * (size_t)nevals, false)) return fail(SGPR_E_NODEVICE, "sgpr_md_run: device allocation failed");
        HIPCHK(hipMemsetAsync(m.npt.cells_d.p, 0, sizeof(double) * SGPR_MD_CELL * (size_t)nevals, st));
    }
    m.halt_host.p[0] = m.halt_host.p[1] = m.halt_host.p[2] = MD_HALT_NONE;   // (page-locked: the source of the copy outlives the call)
    HIPCHK(hipMemcpyAsync(m.halt.p, m.halt_host.p, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    return SGPR_OK;
}

// The host runs AHEAD of the device by at most this many evaluations: before evaluation j is enqueued, evaluation j - LA must
// have set its mark (one int per evaluation in mapped host memory, written by the reducer of the overflow word: the ONLY
// posted write of a step — the sixteen scalars stay in device memory and are copied out once per call), or the run must
// have halted.  A halt therefore leaves at most LA + 1 evaluations in the queue (they exit at once or
// recompute a discarded step), where a fixed chunk of 16 left up to 32 (14 ms per halt at 16384 atoms).  LA = 6 at 4096
// atoms (the host needs ~25 us to enqueue a step of ~80 us), 2 at 16384 (~0.5 ms per step).
static int md_look_ahead(int N) { return std::min(6, std::max(2, (int)lround(24576.0 / std::max(N, 1)))); }   // (fewer for large frames: their steps are long)

// The throttle: spins until evaluation `e` of the call has set its mark or a halt word is set (*halted).  Both are posted
// writes of the device into mapped host memory: the wait costs no call into the runtime — but a dead queue writes neither, so
// every 16384 spins the stream is asked: one that is empty with the mark still unset, or in error, ends the wait with an error.
static int md_wait_for(const MdState &m, hipStream_t st, int e, bool *halted)
{
    const volatile int *mark = m.mark.p + e, *hh = m.halt_host.p;
    auto running = [hh] { return hh[0] == MD_HALT_NONE && hh[1] == MD_HALT_NONE && hh[2] == MD_HALT_NONE; };
    unsigned spins = 0;
    while (*mark == 0 && running()) {
        if ((++spins & 0x3fffu) == 0) {  // (a dead queue must not hang the host)
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess && *mark == 0) return fail(SGPR_E_NODEVICE, "sgpr_md_run: the queue drained without evaluation %d reporting", e);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(SGPR_E_NODEVICE, "sgpr_md_run: %s", hipGetErrorString(q));
        }
    }
    *halted = !running();
    return SGPR_OK;
}

// Enqueues evaluations 0 ... nevals - 1 of a call behind the throttle, until the run halts; *enq: how many.  one(j) enqueues
// evaluation j and returns an error code (a callable inlined here: nothing is allocated or called indirectly per evaluation).
template <typename One>
static int md_enqueue_ahead(sgpr_model *h, int nevals, hipStream_t st, int *enq, One one)
{
    const MdState &m = h->md;
    const int LA = md_look_ahead(m.run.N);
    *enq = 0;
    int rc_ = SGPR_OK;
    bool halted = false;
    for (int j = 0; j < nevals; j++) {
        if (j >= LA) rc_ = md_wait_for(m, st, j - LA, &halted);
        if (rc_ || halted) break;
        rc_ = one(j);
        if (rc_) break;
        *enq = j + 1;
    }
    if (rc_) (void)hipStreamSynchronize(st);   // (the queue is drained before the error is reported)
    return rc_;
}

// The scalars travel behind the last kernel: ONE wait for the whole call (the halt words are in mapped host memory); then the
// cell record of the evaluations enqueued, where the run has one.
static int md_collect(sgpr_model *h, int enq, hipStream_t st, const double *scalars, bool want_cells)
{
    MdState &m = h->md;
    if (scalars && enq > 0)
        HIPCHK(hipMemcpyAsync(m.scal_pin.p, m.scal_d.p, sizeof(double) * SGPR_MD_SCAL * (size_t)enq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (want_cells) {
        m.run.npt.cells.assign((size_t)SGPR_MD_CELL * (size_t)enq, 0.0);
        m.run.npt.cells_first = m.run.t;
        if (enq > 0) HIPCHK(hipMemcpy(m.run.npt.cells.data(), m.npt.cells_d.p, sizeof(double) * SGPR_MD_CELL * (size_t)enq, hipMemcpyDeviceToHost));
    }
    return SGPR_OK;
}

// What a call leaves behind its wait.  k: the evaluation, relative to this call, that halted the run (-1: none); code: 0 none,
// 1 covloss gate, 2 overflow, 3 converged; done: the evaluations whose results stand, the halting one included unless it
// overflowed.  m.run.t moves on: after a halt the state is configuration k, not evaluated as far as the NEXT call goes; otherwise
// every evaluation stands and the state is the next configuration — with final_eval the last one evaluated.
struct MdHalt { int k = -1, code = 0, done = 0; };
static int md_decode_halt(sgpr_model *h, unsigned step0, int enq, int final_eval, bool want_cells, MdHalt *out)
{
    MdState &m = h->md;
    const int hv = md_halt_step(m);
    MdHalt &r = *out;
    r.done = enq;
    if (hv != MD_HALT_NONE) {
        r.k = hv - (int)step0;
        if (r.k < 0 || r.k >= enq) return fail(SGPR_E_INVALID, "sgpr_md_run: inconsistent halt record (%d of %d)", r.k, enq);
        r.code = m.halt_host.p[1] == hv ? 2 : (m.halt_host.p[0] == hv ? 1 : 3);
        r.done = r.k + 1;
        m.run.t += r.k;
        // a capacity overflowed: the next call's checked pass grows it, and the overflowing evaluation's own results are void
        if (r.code == 2) { h->warm = false; r.done -= 1; }
    } else
        m.run.t += final_eval ? enq - 1 : enq;
    if (want_cells) m.run.npt.cells.resize((size_t)SGPR_MD_CELL * (size_t)std::max(r.done, 0));
    return SGPR_OK;
}

// The deviates of a call ([nevals][N][3], caller atom order; null: none) on the device, sorted on upload: m.noise.
static int md_upload_noise(sgpr_model *h, int nevals, const double *noise, hipStream_t st)
{
    MdState &m = h->md;
    if (!noise) return SGPR_OK;
    const size_t len = (size_t)nevals * 3 * m.run.N;
    if (m.noise.alloc(len) || m.noise_raw.alloc(len)) return fail(SGPR_E_NODEVICE, "sgpr_md_run: device allocation failed");
    HIPCHK(hipMemcpyAsync(m.noise_raw.p, noise, sizeof(double) * len, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(md_sort_rows_kernel, dim3(1024), dim3(256), 0, st, m.run.N, nevals, h->d_perm.p, m.noise_raw.p, m.noise.p);
    return SGPR_OK;
}

// Nothing is assumed about a handle's candidate lists, pre-binned configuration or bin populations: the next step on it rebuilds
// the lists and bins into cleared counters.
static int md_reset_lists(sgpr_model *h, hipStream_t st)
{
    h->lists_valid = false;
    h->pre_valid = false;
    HIPCHK(hipMemsetAsync(h->d_bin_count.p, 0, 2 * SGPR_BIN_INTS * sizeof(int), st));
    return SGPR_OK;
}

// The integrator's part of the FinNext record of evaluation j of a call (configuration m.run.t + j), what the fused loop's last
// kernel and md_bcm_move_kernel both read: ring slots, deviates (noise_dev: the call's sorted upload, null: none — then the
// run's seed, if it has one), the Nose-Hoover block, the kinetic terms' slot, the halt word.  pend0: the closing half kick of
// the call's first configuration is due.  Everything else in x is zero.
static void md_fill_integrator(const MdState &m, int j, const double *noise_dev, bool pend0, FinNext &x)
{
    const int RG = m.run.ring, sl = (int)((m.run.t + j) % RG), sn = (sl + 1) % RG, sp = (sl + RG - 1) % RG;
    const size_t N3 = (size_t)3 * m.run.N;
    memset(&x, 0, sizeof(x));
    x.x_cur = m.X.p + N3 * sl; x.v_cur = m.V.p + N3 * sl;
    x.x_next = m.X.p + N3 * sn; x.v_next = m.V.p + N3 * sn;
    x.mass = m.mass.p; x.sig = m.sig.p; x.noise = noise_dev ? noise_dev + N3 * (size_t)j : nullptr;
    x.hdt = m.run.hdt; x.c1 = m.run.c1; x.pending = (j > 0 || pend0) ? 1 : 0;
    if (m.run.nh.on) {
        x.nh = 1; x.nh_first = (m.run.t + j) == 0 ? 1 : 0;
        x.x_prev = m.X.p + N3 * sp; x.v_now = m.V.p + N3 * sl;
        // (v_cur: what the integrator holds when it asks for the forces — ASE sets the momenta of step n after its force
        // call: v_(n-1), the caller's v_0 the first time; its kinetic energy is scalars[13], the calculator's log line)
        if (m.run.t + j > 0) x.v_cur = m.V.p + N3 * sp;
        x.nh_zeta = m.zeta.p + ((m.run.t + j) & 3);
    }
    x.seed = noise_dev ? 0ull : m.seed; x.t_index = m.run.t + j;
    x.ke_cur = m.KE.p + (size_t)2 * m.run.N * sl;
    x.halt = m.halt.p;
    if (m.run.filter.on) { x.filt_cur = m.filter.f.p + N3 * sl; x.filt_next = m.filter.f.p + N3 * sn; x.shrink = m.run.filter.shrink; }
}

// The moving-cell fields of the same record: the ring slots of this evaluation's cell and the next one's, the scaled coordinates.
static void md_fill_moving_cell(const MdState &m, int j, FinNext &x)
{
    const size_t N3 = (size_t)3 * m.run.N, RG = (size_t)m.run.ring, sl = (size_t)(m.run.t + j) % RG, sn = (sl + 1) % RG, sp = (sl + RG - 1) % RG;
    x.npt_cur = m.slot(m.run.t + j); x.npt_next = m.slot(m.run.t + j + 1);
    x.q_cur = m.npt.Q.p + N3 * sl; x.q_prev = m.npt.Q.p + N3 * sp; x.q_next = m.npt.Q.p + N3 * sn;
}

// The cutoffs md_npt_kernel's grids and rebuild rule go by: the lists' as enqueue_step sets it, the model's.
static void md_npt_cutoffs(sgpr_model *h) { NptParams &p = h->md.run.npt.par; p.rc_list = h->rc + (h->use_graph ? 0.0 : h->skin); p.rc_phys = h->rc; }

// The thermostat behind evaluation j of a call, whose results are in `packed`.  Moving cell: zeta, eta and the matrices of the next configuration, the cell after
// it (md_npt.inc; a filter's stress jumps too).  Else Nose-Hoover: zeta of the next configuration from this one's kinetic energy (the next launch's waves need it).
static void md_thermostat_launch(sgpr_model *h, int j, int step, const double *packed, hipStream_t st)
{
    const MdState &m = h->md;
    const int N = m.run.N, sl = (int)((m.run.t + j) % m.run.ring), n30 = (int)((m.run.t + j) & 0x3fffffff);
    double *ke = m.KE.p + (size_t)2 * N * sl, *row = m.scal_d.p + (size_t)SGPR_MD_SCAL * j;
    if (m.run.npt.on)
        hipLaunchKernelGGL(md_npt_kernel, dim3(1), dim3(256), 0, st, N, m.run.npt.par, (NptSlot *)m.npt.ring.p, m.zeta.p, ke, (const double *)(m.V.p + (size_t)3 * N * sl),
                           (const double *)m.mass.p, packed, (const double *)h->d_cell0.p, n30, (const int *)m.halt.p, step, row, m.npt.cells_d.p + (size_t)SGPR_MD_CELL * j,
                           m.run.filter.on ? (const double *)(m.filter.s.p + 6 * ((m.run.t + j) & 3)) : (const double *)nullptr,
                           m.run.filter.on ? m.filter.s.p + 6 * ((m.run.t + j + 1) & 3) : (double *)nullptr, m.run.filter.shrink);
    else if (m.run.nh.on)
        hipLaunchKernelGGL(md_nh_kernel, dim3(1), dim3(256), 0, st, N, ke, m.zeta.p, n30, m.run.dt, m.run.nh.c1, m.run.nh.c2, m.run.nh.K0, (const int *)m.halt.p, step, row);
}

// The checked pass of a handle nothing has sized for its bound system yet (synchronised, capacities grown, results discarded).
static int md_warm(sgpr_model *h, const double *pos, const double *cell, double *packed, hipStream_t st)
{
    const int rc_ = h->warm ? SGPR_OK : run_checked(h, pos, cell, packed, st);
    if (!rc_) h->warm = true;
    return rc_;
}

// What the bias and the bond angles ask of a handle's settings before anything is enqueued (what a step then takes is md_before_last's fused_gather, not this).
static bool md_gather_form(const sgpr_model *h) { return !(h->world != 1 || !h->gather_ok || h->use_graph || !h->fuse_next || !(h->skin > 0.0) || h->comm || (h->use_fork && h->side && !h->profile)); }

// A qlvar's rows in LDS are sized for META_QL_MAXT selected neighbours over its components.  `tail`: how the caller's message ends.
static int md_meta_ql_fits(const sgpr_model *h, const char *tail)
{
    if ((long long)h->md.run.meta.nql * h->maxnn <= META_QL_MAXT) return SGPR_OK;
    return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bias has %d qlvar component(s) and the neighbour list holds up to %d entries per atom; together at "
                                    "most %d%s", h->md.run.meta.nql, h->maxnn, META_QL_MAXT, tail);
}

// enqueue_step's one call for a step of sgpr_md_run: what the run's features refuse when the step did not take the gather form of the fused last kernel,
// then the bias of this configuration (sgpr_md_meta), behind the reverse pass's own sums and in front of the kernel that reads them.
static int md_before_last(sgpr_model *h, const StepNext &nx, bool fused_gather, const double *cell_dev, unsigned step, hipStream_t st)
{
    MdState &m = h->md;
    MdRun::Meta &b = m.run.meta;
    if (nx.md.filt_cur && !fused_gather) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the filter (sgpr_md_filter) runs in the gather form of the fused last kernel only");
    if (m.run.adf.every && !fused_gather)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bond angles (sgpr_md_adf) read the step's list and its overflow word behind the gather form of the "
                                        "fused last kernel only");
    if (!b.on) return SGPR_OK;
    if (!fused_gather)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bias (sgpr_md_meta) runs in the gather form of the fused last kernel only: the scatter form "
                                        "and sharded frames take the host loop around calculate()");
    const long long n = nx.md.t_index, want = b.merge ? m.run.meta_slot(n) / b.merge : 0;
    const int N = h->N, nh = (int)m.run.meta_slot(n), own = n % b.pace == 0 ? nh : -1;   // (nh: the rows below this configuration; own: its own where it deposits)
    if (const int rq = md_meta_ql_fits(h, " (the host loop around calculate() serves longer lists)")) return rq;   // (a qlvar reads this step's list, which may have grown)
    MetaQl ql = b.ql;
    ql.nn = h->d_nn.p; ql.nbr_j = h->d_nbr_j.p; ql.nbr_code = h->d_nbr_shift.p; ql.cell = cell_dev; ql.maxnn = h->maxnn;
    // the merged form: the chunks that lie below this configuration and are not merged yet — at a crossing, or at the first configuration of a call that is behind
    const MetaTab tb = m.meta_tab(want);
    for (long long &j = b.enq; j < want; j++) {
        hipLaunchKernelGGL(md_meta_merge_kernel, dim3(1), dim3(256), 0, st, b.par.D, b.merge, (int)j, (const double *)m.meta.centre.p,
                           (const int *)m.meta.key.p, tb, (const int *)nx.md.halt, (int)step);
        stamp(h, "md_meta_merge", st);
    }
    // md_meta.inc's four entry points take one argument list but for a qlvar's MetaQl (q) and the merged form's MetaTab (t)
    auto with = [&](auto... q) {
        return [&, q...](auto kernel, auto... t) {
            hipLaunchKernelGGL(kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, b.par, q..., nx.md.x_cur, (const unsigned char *)m.meta.sel.p, m.meta.centre.p,
                               m.meta.key.p, m.meta.rows.p, nh, own, h->d_F.p + 3 * (size_t)N, h->d_Epart.p, h->d_virpart.p, h->virpart_len, t...,
                               (const int *)nx.md.halt, (int)step);
        };
    };
    if (b.nql) b.merge ? with(ql)(md_meta_merged_ql_kernel, tb) : with(ql)(md_meta_ql_kernel);
    else b.merge ? with()(md_meta_merged_kernel, tb) : with()(md_meta_kernel);
    stamp(h, "md_meta", st);
    return SGPR_OK;
}

// The close of a call: the scalar rows of the evaluations that stand to the caller — columns 14 and 15 are zeta and its time
// integral under Nose-Hoover, a relaxation's own (keep_14_15), else spare: zeroed — and what the call reports.
// The configuration is evaluated as far as the next call goes behind the covloss gate (1), convergence (3: a relaxation and a band
// only, no kernel of the dynamics writes that halt word) and a `final` call that ran through.
static void md_finish_call(sgpr_model *h, const MdHalt &r, double *scalars, bool keep_14_15, int final_eval, int *evals_done, int *halt_code)
{
    MdState &m = h->md;
    if (scalars && r.done > 0) {
        memcpy(scalars, m.scal_pin.p, sizeof(double) * SGPR_MD_SCAL * (size_t)r.done);
        if (!keep_14_15)
            for (int e = 0; e < r.done; e++) scalars[(size_t)SGPR_MD_SCAL * e + 14] = scalars[(size_t)SGPR_MD_SCAL * e + 15] = 0.0;
    }
    m.run.evaluated = r.code == 1 || r.code == 3 || (r.code == 0 && final_eval != 0);
    *evals_done = r.done;
    if (halt_code) *halt_code = r.code;
    h->lists_valid = false;
}

// The frame of evaluation j of a call (configuration n = m.run.t + j, n % rec.every == 0), behind the evaluation's last launch: the
// ring slots sgpr_md_state(which = -1) would read had the call ended with this evaluation — X and P: n % ring; V: that slot
// (Langevin, velocity Verlet), the slot before it (Nose-Hoover and NPT, n > 0: what the integrator holds when it asks for F_n),
// slot 0 (a relaxation).  Its place in the record: its ordinal among the call's recorded evaluations.
static void md_record_frame(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const long long n = m.run.t + j;
    const int N = m.run.N, RG = m.run.ring, sl = (int)(n % RG), plen = (int)sgpr_packed_len(N);
    const size_t f = (size_t)MdRun::rec_between(m.run.t, n, m.run.rec.every), N3 = (size_t)3 * N;
    const int sv = m.run.relax.on ? 0 : ((m.run.nh.on && n > 0) ? (sl + RG - 1) % RG : sl);
    const bool wv = (m.run.rec.what & 1) != 0, wp = (m.run.rec.what & 2) != 0;
    const int elems = wp ? std::max(3 * N, plen) : 3 * N;
    hipLaunchKernelGGL(md_record_kernel, dim3((elems + 255) / 256), dim3(256), 0, st, N, plen, (const int *)h->d_perm.p,
                       (const double *)(m.X.p + N3 * sl), wv ? (const double *)(m.V.p + N3 * sv) : (const double *)nullptr,
                       wp ? (const double *)(m.P.p + (size_t)plen * sl) : (const double *)nullptr, m.rec.x.p + N3 * f,
                       wv ? m.rec.v.p + N3 * f : (double *)nullptr, wp ? m.rec.p.p + (size_t)plen * f : (double *)nullptr,
                       (const int *)m.halt.p, step);
}

// The sample of evaluation j of a call (configuration n = m.run.t + j, n % msd.every == 0), behind the evaluation's last launch
// like the frame: the two launches of md_msd.inc on the X slot of n.  The due levels follow from n alone; whether n is the
// sample the table waits for (next_due) is the device's decision.
static int md_msd_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::Msd &a = m.run.msd;
    const long long n = m.run.t + j, s = n / a.every;
    const unsigned due = md_due_levels(s, a.levels, nullptr);
    const int acc = s > 0 ? 1 : 0, N = m.run.N;
    const size_t N3 = (size_t)3 * N;
    const int *chunk = m.msd.tab.p, *coff = chunk + 2 * a.nch, *nz = coff + a.S + 1;
    hipLaunchKernelGGL(md_msd_part_kernel, dim3(a.nch), dim3(256), 0, st, chunk, a.nch, (const double *)(m.X.p + N3 * (size_t)(n % m.run.ring)),
                       (const double *)m.mass.p, m.msd.origin.p, N3, due, acc, m.msd.part.p, (const long long *)m.msd.ctl.p, n, (const int *)m.halt.p, step);
    hipLaunchKernelGGL(md_msd_fold_kernel, dim3(1), dim3(256), sizeof(double) * a.levels * a.S * MSD_PART, st, coff, nz, a.nch, a.S, a.levels, a.mtot,
                       a.com, due, acc, (const double *)m.msd.part.p, m.msd.table.p, m.msd.ctl.p, n, a.every, (const int *)m.halt.p, step);
    return SGPR_OK;
}

// The same for the pair distances (md_rdf.inc): the pair sweep over the X slot of configuration n — the R = 0 form where no
// image but the nearest can come within rmax — and the launch that counts the sample.
static int md_rdf_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::Rdf &a = m.run.rdf;
    const long long n = m.run.t + j;
    const double *x = m.X.p + (size_t)3 * m.run.N * (size_t)(n % m.run.ring);
    if (a.npairs)
        hipLaunchKernelGGL(a.images ? md_rdf_pair_kernel<true> : md_rdf_pair_kernel<false>, dim3(a.npairs, a.split), dim3(256), 0, st, (const int *)m.rdf.tab.p, x,
                           a.g, m.rdf.table.p, (const long long *)m.rdf.ctl.p, n, (const int *)m.halt.p, step);
    hipLaunchKernelGGL(md_rdf_done_kernel, dim3(1), dim3(64), 0, st, m.rdf.ctl.p, n, a.every, (const int *)m.halt.p, step);
    return SGPR_OK;
}

// The same for the velocity autocorrelations (md_vacf.inc): the store of sample s = n / every — V slot n, under Langevin and
// velocity Verlet with the closing half kick of the evaluation's packed force (n > 0) — and, for s > 0, the correlation of sample
// s - 1 with its due origins; the launch that advances next_due.  Which lags are due follows from s and origin_every alone;
// whether n is the awaited sample is the device's decision.
static int md_vacf_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::Vacf &a = m.run.vacf;
    const long long n = m.run.t + j, s = n / a.every, p = s - 1;
    const int N = m.run.N, slots = a.lags + 1, sl = (int)(n % m.run.ring);
    const size_t N3 = (size_t)3 * N, ss = (size_t)(s % slots);
    const int *chunk = m.vacf.tab.p, *coff = chunk + 2 * a.nch, *nz = coff + a.S + 1;
    const bool kick = !m.run.nh.on && n > 0;
    const int *halt = m.halt.p;
    hipLaunchKernelGGL(md_vacf_store_kernel, dim3(a.nch), dim3(256), 0, st, chunk, (const double *)(m.V.p + N3 * sl),
                       kick ? (const double *)(m.P.p + (size_t)sgpr_packed_len(N) * sl) : (const double *)nullptr, (const int *)h->d_perm.p,
                       (const double *)m.mass.p, m.fix(), m.run.hdt, m.vacf.ring.p + N3 * ss, m.vacf.vpart.p + (size_t)6 * a.nch * ss, halt, step);
    if (s > 0) {
        hipLaunchKernelGGL(md_vacf_corr_kernel, dim3(a.nch, (a.lags + VACF_GROUP - 1) / VACF_GROUP), dim3(256), 0, st, chunk, a.nch,
                           (const double *)m.vacf.ring.p, N3, slots, p, a.lags, a.origin_every, m.vacf.part.p, (const long long *)m.vacf.ctl.p, n, halt, step);
        hipLaunchKernelGGL(md_vacf_fold_kernel, dim3((a.lags + VACF_FOLD - 1) / VACF_FOLD), dim3(256), sizeof(double) * (6 * a.S + 3), st, coff, nz,
                           a.nch, a.S, a.lags, a.origin_every, slots, p, a.mtot, a.com, (const double *)m.vacf.vpart.p, (const double *)m.vacf.part.p,
                           m.vacf.jring.p, m.vacf.cring.p, m.vacf.tr.p, m.vacf.col.p, m.vacf.ctl.p, n, halt, step);
    }
    hipLaunchKernelGGL(md_vacf_done_kernel, dim3(1), dim3(64), 0, st, m.vacf.ctl.p, n, a.every, s > 0 ? 1 : 0, halt, step);
    return SGPR_OK;
}

// The same for the van Hove functions (md_vanhove.inc): md_msd's due levels; the pair sweep of the distinct part — one grid layer
// per due level, origins against the X slot of n — BEFORE the self part, which measures the displacements and overwrites the
// origins; the launch that counts.  Sample 0 only sets origins.
static int md_vh_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::VanHove &a = m.run.vh;
    const long long n = m.run.t + j, s = n / a.every;
    int ndue = 0;
    const unsigned due = md_due_levels(s, a.levels, &ndue);
    const int acc = s > 0 ? 1 : 0, N = m.run.N;
    const size_t N3 = (size_t)3 * N;
    const double *x = m.X.p + N3 * (size_t)(n % m.run.ring);
    const int *chunk = m.vh.tab.p, *pair = chunk + VH_CHUNK * a.nch, *halt = m.halt.p;
    if (a.dbins && a.npairs && acc)
        hipLaunchKernelGGL(a.images ? md_vh_pair_kernel<true> : md_vh_pair_kernel<false>, dim3(a.npairs, a.split, ndue), dim3(256), 0, st, pair,
                           (const double *)m.vh.origin.p, N3, x, a.g, due, m.vh.hd.p, (size_t)a.S * a.S * a.dbins, (const long long *)m.vh.ctl.p, n,
                           halt, step);
    if (a.nch)
        hipLaunchKernelGGL(md_vh_self_kernel, dim3(a.nch), dim3(256), 0, st, chunk, x, m.vh.origin.p, N3, (const double *)m.vh.edges.p, a.rmax,
                           a.rbins, a.tbins, a.pbins, a.S, due, acc, m.vh.hs.p, (size_t)a.rbins * a.tbins * a.pbins, m.vh.over.p,
                           (const long long *)m.vh.ctl.p, n, halt, step);
    hipLaunchKernelGGL(md_vh_done_kernel, dim3(1), dim3(64), 0, st, m.vh.ctl.p, n, a.every, due, acc, halt, step);
    return SGPR_OK;
}

// The LDS of md_adf_kernel for a list of capacity maxnn: the waves of a workgroup (4 ... 1, 0: one centre's rows alone do not fit)
// and the bytes.
static int md_adf_waves(const MdRun::Adf &a, int maxnn, size_t &bytes)
{
    const size_t fixed = adf_lds_fixed(a.S, a.bins, a.lds);
    for (int w = 4; w >= 1; w--) {
        bytes = fixed + (size_t)w * (size_t)std::max(maxnn, 1) * ADF_ROW_BYTES;
        if (bytes <= ADF_LDS_BYTES) return w;
    }
    return 0;
}

// The same for the bond angles (md_adf.inc): the pass over the list that this evaluation's forward pass has left, for the X slot
// of configuration n, and the launch that counts the sample.  The rows are sized for the list's capacity as it stands now.
static int md_adf_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::Adf &a = m.run.adf;
    const long long n = m.run.t + j;
    size_t bytes = 0;
    const int waves = md_adf_waves(a, h->maxnn, bytes);
    if (!waves)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bond angles (sgpr_md_adf) keep a centre's neighbours in LDS; a list of up to %d entries per atom with "
                    "%d bins and %d species does not fit %d bytes", h->maxnn, a.bins, a.S, ADF_LDS_BYTES);
    if (a.nch) {
        AdfArgs f = {};
        f.chunk = m.adf.tab.p; f.x = m.X.p + (size_t)3 * m.run.N * (size_t)(n % m.run.ring); f.cell = m.cell.p;
        f.nn = h->d_nn.p; f.nbr_j = h->d_nbr_j.p; f.nbr_code = h->d_nbr_shift.p;
        f.cut = m.adf.par.p; f.ct = m.adf.par.p + (size_t)a.S * a.S;
        f.angles = m.adf.angles.p; f.coord = m.adf.coord.p; f.ctl = m.adf.ctl.p; f.halt = m.halt.p;
        f.ov = m.scal_d.p + (size_t)SGPR_MD_SCAL * j + 10;
        f.n = n; f.maxnn = h->maxnn; f.S = a.S; f.bins = a.bins; f.step = step;
        hipLaunchKernelGGL(a.lds ? md_adf_kernel<true> : md_adf_kernel<false>, dim3(a.nch), dim3(64 * waves), bytes, st, f);
    }
    hipLaunchKernelGGL(md_adf_done_kernel, dim3(1), dim3(64), 0, st, m.adf.ctl.p, n, a.every, (const int *)m.halt.p, step,
                       (const double *)(m.scal_d.p + (size_t)SGPR_MD_SCAL * j + 10));
    return SGPR_OK;
}

// The same for the structure factors (md_sq.inc): the phase sums of the X slot of configuration n per chunk and wave vector, the
// fold into the ring, the mean and the due lags of f, and the launch that counts the sample.  Which lags are due follows from s
// and origin_every alone; whether n is the awaited sample is the device's decision.
static int md_sq_sample(sgpr_model *h, int j, int step, hipStream_t st)
{
    MdState &m = h->md;
    const MdRun::Sq &a = m.run.sq;
    const long long n = m.run.t + j, s = n / a.every;
    const double *x = m.X.p + (size_t)3 * m.run.N * (size_t)(n % m.run.ring);
    const int *chunk = m.sq.tab.p, *coff = chunk + 2 * a.nch, *hkl = coff + a.S + 1, *halt = m.halt.p;
    const long long *ctl = m.sq.ctl.p;
    const int tiles = (a.nq + SQ_TILE - 1) / SQ_TILE;
    const auto wide = md_sq_part_kernel<64, SQ_WIDE_H + 1>, narrow = md_sq_part_kernel<32, SQ_MAXH + 1>;
    if (a.nch)
        hipLaunchKernelGGL(a.narrow ? narrow : wide, dim3(a.nch, tiles), dim3(256), 0, st, chunk, x, (const double *)m.sq.inv.p, hkl, a.nq,
                           m.sq.part.p, ctl, n, halt, step);
    static_assert(sizeof(double) * 2 * SGPR_MAX_S * SQ_TILE <= 65536, "the fold's densities [S][2][SQ_TILE] fit the LDS of a workgroup at every S (64 KiB at SGPR_MAX_S: one workgroup per CU there)");
    hipLaunchKernelGGL(md_sq_fold_kernel, dim3(tiles, (a.lags + SQ_FOLD - 1) / SQ_FOLD), dim3(256), sizeof(double) * 2 * a.S * SQ_TILE, st, coff, a.S,
                       a.nq, a.lags, a.origin_every, s, (const double *)m.sq.part.p, m.sq.ring.p, m.sq.mean.p, m.sq.f.p, ctl, n, halt, step);
    hipLaunchKernelGGL(md_sq_done_kernel, dim3(1), dim3(256), 0, st, m.sq.ctl.p, n, a.every, a.lags, a.origin_every, s, halt, step);
    return SGPR_OK;
}

// Behind evaluation j of a call (and its frame): the samples of the accumulators whose interval divides the configuration's
// index, in the table's order.  A run without accumulators tests six integers and launches nothing.
static int md_sample_due(sgpr_model *h, int j, int step, hipStream_t st)
{
    const MdRun &r = h->md.run;
    for (const MdAcc &a : MD_ACC) {
        const int every = a.every(r);
        if (every && (r.t + j) % every == 0)
            if (const int rs = a.sample(h, j, step, st)) return rs;
    }
    return SGPR_OK;
}

// Which frames of a call stand (t0: its first configuration): those of the evaluations whose results stand — less the halting
// one when the covloss gate fired (code 1): that configuration goes to the caller's calculate() and is evaluated, and recorded,
// again by the next call.  An overflow (2) has left the halting evaluation out of `done` already; a converged relaxation (3)
// keeps its frame: the final structure.  Frames that look-ahead evaluations wrote beyond that count are overwritten later.
static void md_record_close(MdState &m, const MdHalt &r)
{
    if (!m.run.rec.call_every) return;
    const int lim = std::max(r.code == 1 ? r.done - 1 : r.done, 0);
    m.run.rec.call_count = (int)MdRun::rec_between(m.run.rec.call_t0, m.run.rec.call_t0 + lim, m.run.rec.call_every);
}

// ---- the frame of the three run functions (md_relax_run, md_committee_run, md_replica_run): md_call_open | the mode's checks, md_prepare_call, its checked pass | md_call_start |
// md_enqueue_ahead | md_call_close | the mode's record of the call | md_finish_call ----
struct MdCall {
    hipStream_t st = nullptr;
    int N = 0;
    size_t plen = 0;      // the packed length 4N + 11
    double gate = 1e300;  // the covloss that halts the run (ediff <= 0: never)
    unsigned step0 = 0;   // the handle's step counter at the first evaluation: what the halt words count from
    int enq = 0;          // evaluations enqueued
};

// The run's own system bound again on its device, nothing done yet as far as the caller's counters go.
static int md_call_open(sgpr_model *h, double ediff, int *evals_done, int *halt_code, MdCall &c)
{
    HIPCHK(hipSetDevice(h->device));
    if (const int rb = md_rebind(h)) return rb;
    c.st = h->stream;
    c.N = h->md.run.N;
    c.plen = (size_t)sgpr_packed_len(c.N);
    c.gate = ediff > 0.0 ? ediff : 1e300;
    *evals_done = 0;
    if (halt_code) *halt_code = 0;
    return SGPR_OK;
}

// Behind the checked pass (which counts as a step): the record of the last call's continuation is void from here on — sgpr_md_run
// reads it first and writes a new one at its end — and the evaluations count from the handle's step counter as it stands.
static void md_call_start(sgpr_model *h, MdCall &c)
{
    h->md.run.chain.ok = false;
    c.step0 = h->step_count;
}

// The one wait of the call, then what it leaves (md_record_close: a committee and a band refuse an armed record, so it does
// nothing for them).  sgpr_md_run spells the same three out: peer_check, the chain decision and its md_reset_lists stand between
// its wait and its decode.
static int md_call_close(sgpr_model *h, const MdCall &c, int final_eval, const double *scalars, bool want_cells, MdHalt *r)
{
    if (const int rc = md_collect(h, c.enq, c.st, scalars, want_cells)) return rc;
    if (const int rd = md_decode_halt(h, c.step0, c.enq, final_eval, want_cells, r)) return rd;
    md_record_close(h->md, *r);
    return SGPR_OK;
}

// sgpr_md_run for a relaxation: every evaluation is the plain step (its own binning kernel, the plain last kernel) with
// md_fire_kernel and md_fire_move_kernel behind it.  The halts — covloss gate (1), capacity overflow (2), convergence (3) — are
// decided by md_fire_kernel on the evaluation itself, before anything moves: what the host has enqueued behind a halt (its
// look-ahead) evaluates stale slots of the rings and changes nothing.  final_eval: the last evaluation moves nothing and leaves
// the optimizer as it was.
static int md_relax_run(sgpr_model *h, int nevals, double ediff, int final_eval, double *scalars, int *evals_done, int *halt_code)
{
    MdState &m = h->md;
    MdCall c;
    if (const int ro = md_call_open(h, ediff, evals_done, halt_code, c)) return ro;
    hipStream_t st = c.st;
    const int N = c.N, RG = RLX_RING;
    const size_t plen = c.plen;
    MdBinIdentity guard(h);
    if (const int rp = md_prepare_call(h, nevals, st, true)) return rp;
    auto cell_of = [&](long long n) -> double * { return m.relax.cells.p + (size_t)RLX_CELL * (size_t)(n % RG); };
    m.run.relax.started = true; m.run.started = true;
    if (const int rw = md_warm(h, m.X.p + (size_t)3 * N * (m.run.t % RG), cell_of(m.run.t), m.P.p + plen * (m.run.t % RG), st)) return rw;
    md_call_start(h, c);
    if (const int rl = md_reset_lists(h, st)) return rl;
    const unsigned step0 = c.step0; const double gate = c.gate;
    const int rc_ = md_enqueue_ahead(h, nevals, st, &c.enq, [&](int j) -> int {
        const int sl = (int)((m.run.t + j) % RG), sn = (sl + 1) % RG;
        double *packed = m.P.p + plen * sl;
        const int re = enqueue_step(h, m.X.p + (size_t)3 * N * sl, cell_of(m.run.t + j), packed, st, nullptr);
        if (re) return re;
        h->lists_valid = true;
        const bool stay = final_eval && j == nevals - 1;
        if (m.run.lbfgs.on) {   // (sgpr_md_relax_lbfgs: md_lbfgs.inc's four kernels in the place of FIRE's two)
            const MdRun::Lbfgs &lb = m.run.lbfgs;
            const RelaxParams &rp = m.run.relax.par;
            const LbfgsBuf b = md_lbfgs_buf(m);
            const long long n = m.run.t + j;
            const int cnt = (int)std::min<long long>(n - lb.base, lb.mem), B = (N + 255) / 256, NR = N + (rp.cell ? 3 : 0), B3 = (NR + 63) / 64;
            const int stp = (int)(step0 + j);
            const bool fx = m.run.fix.n != 0;
            hipLaunchKernelGGL(fx ? md_lbfgs_dots_kernel<true> : md_lbfgs_dots_kernel<false>, dim3(B, std::max(cnt, 1)), dim3(256), 0, st, N, rp.cell, lb.mem, b, n,
                               cnt, (const double *)packed, (const int *)h->d_perm.p, (const double *)cell_of(n), (const int *)m.halt.p, stp, m.fix());
            hipLaunchKernelGGL(md_lbfgs_solve_kernel, dim3(1), dim3(256), 0, st, N, rp, lb.mem, lb.h0, b, n, cnt, B, (const double *)packed,
                               (const double *)cell_of(n), gate, m.halt.p, m.halt_host.dev, stp, m.scal_d.p + (size_t)SGPR_MD_SCAL * j,
                               m.npt.cells_d.p + (size_t)SGPR_MD_CELL * j, m.mark.dev + j, stay ? 1 : 0);
            if (!stay) {
                hipLaunchKernelGGL(fx ? md_lbfgs_dir_kernel<true> : md_lbfgs_dir_kernel<false>, dim3(B3), dim3(64), 0, st, N, NR, lb.mem, lb.h0, b, n, cnt,
                                   (const int *)m.halt.p, stp, m.fix());
                hipLaunchKernelGGL(fx ? md_lbfgs_move_kernel<true> : md_lbfgs_move_kernel<false>, dim3((NR + 255) / 256), dim3(256), 0, st, N, rp, lb.mem,
                                   lb.maxstep, lb.damping, b, n, B3, m.relax.ref.p, m.X.p + (size_t)3 * N * sn, cell_of(n + 1), (const int *)m.halt.p, stp,
                                   m.scal_d.p + (size_t)SGPR_MD_SCAL * j, m.fix());
            }
            if (m.run.rec.every && n % m.run.rec.every == 0) md_record_frame(h, j, stp, st);
            return SGPR_OK;
        }
        // (held components, sgpr_md_fix: the FIX forms; without a mask the kernels of a run without one)
        hipLaunchKernelGGL(m.run.fix.n ? md_fire_kernel<true> : md_fire_kernel<false>, dim3(1), dim3(256), 0, st, N, m.run.relax.par, m.relax.state.p,
                           (const double *)packed, (const int *)h->d_perm.p,
                           (const double *)m.V.p, (const double *)cell_of(m.run.t + j), cell_of(m.run.t + j + 1), gate, m.halt.p, m.halt_host.dev,
                           (int)(step0 + j), m.scal_d.p + (size_t)SGPR_MD_SCAL * j, m.npt.cells_d.p + (size_t)SGPR_MD_CELL * j, m.mark.dev + j, stay ? 1 : 0,
                           m.fix());
        if (!stay)
            hipLaunchKernelGGL(m.run.fix.n ? md_fire_move_kernel<true> : md_fire_move_kernel<false>, dim3((N + 63) / 64), dim3(256), 0, st, N, m.run.relax.par.cell,
                               (const double *)m.relax.state.p,
                               (const int *)h->d_perm.p, (const double *)packed, m.V.p, m.relax.ref.p, m.X.p + (size_t)3 * N * sn,
                               (const double *)cell_of(m.run.t + j), (const double *)cell_of(m.run.t + j + 1), (const int *)m.halt.p, (int)(step0 + j),
                               m.fix());
        // (the frame BEHIND the move: sgpr_md_state reads a relaxation's velocity from slot 0, which the move kernel updates in
        // place — after a cut call that moved out of n it returns the moved velocity with the positions of n; where nothing
        // moves — a halt at n, the last evaluation of a `final` call — it returns the one before the move, and so does this.
        // Positions and results of n are in slots the move does not write.)
        if (m.run.rec.every && (m.run.t + j) % m.run.rec.every == 0) md_record_frame(h, j, (int)(step0 + j), st);
        return SGPR_OK;
    });
    if (rc_) return rc_;
    MdHalt r;
    if (const int rc = md_call_close(h, c, final_eval, scalars, true, &r)) return rc;
    md_finish_call(h, r, scalars, true, final_eval, evals_done, halt_code);
    return SGPR_OK;
}

// The Bayesian committee of the run begun by sgpr_md_begin (md_bcm.inc has the rule): members[K], frozen models evaluated
// beside the live handle h at every configuration, in this order with h last; the run integrates the weighted forces, gates
// on the largest member-wise minimum covloss and reports the weighted energy and virial.  After sgpr_md_begin and, if used,
// sgpr_md_thermostat; before the first sgpr_md_run — a detach (K = 0 or members = NULL: the run is the one without this call)
// too: a run that has started keeps what it has.
// The members are BORROWED: the caller keeps them alive until sgpr_md_end or a detach, and may use them between two
// sgpr_md_run calls (every call binds them to the run's system again).  One rank, no mask, no filter, no bias, no frame record;
// constant cell or — the run's option "md_committee_cell" set (sgpr_set_option; off, a committee and a barostat refuse each
// other), with sgpr_md_barostat before or after this call — the moving cell: every member is then evaluated in the cell of the
// configuration, and the barostat integrates the committee's stress.
extern "C" int sgpr_md_committee(sgpr_model *h, int K, sgpr_model *const *members)
{
    if (!h || K < 0) return fail(SGPR_E_INVALID, "sgpr_md_committee: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_committee: call sgpr_md_begin first");
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_committee: the run has started");
    if (K == 0 || !members) { m.run.bcm.members.clear(); m.run.bcm.info.clear(); return SGPR_OK; }
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run has a bias (sgpr_md_meta), which the committee's loop does not apply; the host loop around calculate() serves it");
    if (m.run.filter.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run has a filter (sgpr_md_filter); a committee, with or without a barostat, integrates unfiltered forces");
    if (m.run.npt.on && !m.run.bcm.cell)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run has a barostat; a committee runs at constant cell unless the run's option "
                    "md_committee_cell is set (sgpr_set_option)");
    if (m.run.relax.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run is a relaxation; a committee serves dynamics only");
    if (m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run is a nudged elastic band; a committee serves dynamics only");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run is a ring polymer (sgpr_md_pimd), which is evaluated by one model");
    if (m.run.fix.n) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: %d components are held (sgpr_md_fix); a committee runs without a mask", m.run.fix.n);
    if (m.run.rec.every) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: a frame record is armed (sgpr_md_record); a committee records no frames");
    if (const MdAcc *a = md_acc_attached(m.run)) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run accumulates %s (%s), which the committee's loop does not sample", a->noun, a->fn);
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: the run was begun on %d ranks; a committee runs on one", m.run.world);
    if (K > BCM_MAX - 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: %d members; at most %d beside the live model", K, BCM_MAX - 1);
    for (int k = 0; k < K; k++) {
        const sgpr_model *mk = members[k];
        if (!mk) return fail(SGPR_E_INVALID, "sgpr_md_committee: member %d is null", k);
        if (mk == h) return fail(SGPR_E_INVALID, "sgpr_md_committee: member %d is the live handle itself", k);
        for (int q = 0; q < k; q++)
            if (members[q] == mk) return fail(SGPR_E_INVALID, "sgpr_md_committee: member %d is member %d again", k, q);
        if (!(mk->m > 0 && mk->has_mu)) return fail(SGPR_E_INVALID, "sgpr_md_committee: member %d has no weights", k);
        if (!mk->has_choli) return fail(SGPR_E_INVALID, "sgpr_md_committee: member %d has no choli (its covloss is part of the rule)", k);
        if (mk->device != h->device)
            return fail(SGPR_E_UNSUPPORTED, "sgpr_md_committee: member %d lives on device %d, the run on device %d", k, mk->device, h->device);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N3 = (size_t)3 * m.run.N;
    if (m.bcm.P.alloc((size_t)(K + 1) * (size_t)sgpr_packed_len(m.run.N)) || m.bcm.x.alloc(N3))
        return fail(SGPR_E_NODEVICE, "sgpr_md_committee: device allocation failed");
    // every slot of the ring of positions a valid configuration from the start: what the host has enqueued behind a halt
    // evaluates stale slots (and changes nothing) — zeros there would overflow the live model's lists
    for (int r = 1; r < 4; r++) HIPCHK(hipMemcpy(m.X.p + N3 * r, m.X.p, sizeof(double) * N3, hipMemcpyDeviceToDevice));
    m.run.bcm.members.assign(members, members + K);
    m.run.bcm.info.clear();
    return SGPR_OK;
}

// Weights and largest covlosses of the committee, K + 1 doubles each (the members in their order, the live model last), of the
// last evaluation whose results stand: the numbers behind the packed results sgpr_md_state returns after a halted or `final` call.
extern "C" int sgpr_md_committee_info(sgpr_model *h, double *w, double *covmax)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_committee_info: bad arguments");
    const MdState &m = h->md;
    if (!m.active || m.run.bcm.members.empty()) return fail(SGPR_E_INVALID, "sgpr_md_committee_info: call sgpr_md_begin and sgpr_md_committee first");
    if (m.run.bcm.info.empty()) return fail(SGPR_E_INVALID, "sgpr_md_committee_info: no evaluation of the run stands yet");
    const size_t K1 = m.run.bcm.members.size() + 1;
    if (w) memcpy(w, m.run.bcm.info.data(), sizeof(double) * K1);
    if (covmax) memcpy(covmax, m.run.bcm.info.data() + BCM_MAX, sizeof(double) * K1);
    return SGPR_OK;
}

// The committee's forces at configuration 0 of a moving-cell trajectory, for md_npt_start's backward step: every member's
// synchronised evaluation in the cell h_0 (the live model's is in slot 0 of the run's packed ring already), the weights by
// md_bcm_kernel — the device's log, as in every evaluation of the run; row `spare_row` of the call's scalar ring, marks and
// committee record takes what else it writes —, then the combination on the host in md_bcm_move_kernel's operations: member
// order, no contraction.  F: [N][3] caller order; in: the live model's forces, out: the committee's.
static int md_committee_forces0(sgpr_model *h, int spare_row, hipStream_t st, std::vector<double> &F)
{
#pragma clang fp contract(off)
    MdState &m = h->md;
    const int N = m.run.N, K = (int)m.run.bcm.members.size(), K1 = K + 1;
    const size_t plen = (size_t)sgpr_packed_len(N);
    for (int k = 0; k < K; k++) {
        sgpr_model *mk = m.run.bcm.members[k];
        const int rc_ = run_checked(mk, m.bcm.x.p, m.slot(0)->h, m.bcm.P.p + plen * k, st);
        if (rc_) return rc_;
        mk->warm = true;
    }
    HIPCHK(hipMemcpyAsync(m.bcm.P.p + plen * K, m.P.p, sizeof(double) * plen, hipMemcpyDeviceToDevice, st));
    double *info = m.bcm.info_d.p + (size_t)BCM_INFO * spare_row;
    hipLaunchKernelGGL(md_bcm_kernel, dim3(1), dim3(256), 0, st, N, K1, plen, (const double *)m.bcm.P.p, m.P.p, info, 1e300, m.halt.p, m.halt_host.dev,
                       (int)h->step_count, m.scal_d.p + (size_t)SGPR_MD_SCAL * spare_row, m.mark.dev + spare_row);
    std::vector<double> w(BCM_INFO), P((size_t)K1 * plen);
    HIPCHK(hipMemcpyAsync(w.data(), info, sizeof(double) * BCM_INFO, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P.data(), m.bcm.P.p, sizeof(double) * K1 * plen, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    // (the checked passes have sized every capacity, so no overflow word has halted anything; the halts are armed as md_prepare_call left them)
    m.halt_host.p[0] = m.halt_host.p[1] = m.halt_host.p[2] = MD_HALT_NONE;
    HIPCHK(hipMemcpyAsync(m.halt.p, m.halt_host.p, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    for (size_t e = 0; e < (size_t)3 * N; e++) {
        double acc = 0.0;
        for (int k = 0; k < K1; k++) acc = acc + w[k] * P[(size_t)k * plen + e];
        F[e] = acc;
    }
    return SGPR_OK;
}

// sgpr_md_run for a run with a committee, in the shape of md_relax_run: every evaluation is K + 1 plain steps on the live
// handle's stream — each member on the caller-order copy of the positions through its own binning kernel and permutation, the
// live handle on its sorted ring slot — with md_bcm_kernel, md_bcm_move_kernel and md_bcm_ke_kernel behind them (Nose-Hoover:
// md_nh_kernel too).  The halts — covloss gate (1), capacity overflow of any member (2) — are decided by md_bcm_kernel on the
// evaluation itself, before anything moves: what the host has enqueued behind a halt evaluates stale slots and changes nothing.
//   With a barostat (sgpr_md_barostat): the K + 1 plain steps of evaluation n run in the cell h_n of the ring (as a relaxation's
// plain steps run in a cell that changes every evaluation: each handle's binning kernel keeps or rebuilds its lists by its own
// affine rule), md_bcm_move_kernel<true> integrates in scaled coordinates, and md_npt_kernel takes md_nh_kernel's place: it
// reads the combined virial md_bcm_kernel left in the run's packed ring slot, so the barostat integrates the committee's stress.
// md_npt_kernel runs at a halting evaluation too (it exits only behind one): of the ring slots n - 1, n, n + 1, n + 2 it reads
// h, eta, zeta of n - 1 and n and h of n + 1, and writes eta, zeta and the matrices of n + 1 and h and the grid of n + 2 —
// nothing it reads —, so the repeat of the halted configuration with the updated model overwrites all of it.
static int md_committee_run(sgpr_model *h, int nevals, const double *noise, double ediff, int final_eval, double *scalars, int *evals_done,
                            int *halt_code)
{
    MdState &m = h->md;
    MdCall c;
    if (const int ro = md_call_open(h, ediff, evals_done, halt_code, c)) return ro;
    hipStream_t st = c.st;
    const int N = c.N, RG = m.run.ring, K = (int)m.run.bcm.members.size(), K1 = K + 1;
    const size_t plen = c.plen, N3 = (size_t)3 * N;
    for (int k = 0; k < K; k++) {
        const sgpr_model *mk = m.run.bcm.members[k];
        if (!(mk->m > 0 && mk->has_mu && mk->has_choli)) return fail(SGPR_E_NOMODEL, "sgpr_md_run: member %d of the committee has lost its weights", k);
        HIPCHK(hipStreamSynchronize(mk->stream));   // (whatever the caller ran on the member between two calls is behind us)
    }
    m.run.started = true;
    MdBinIdentity guard(h);
    const bool cellrun = m.run.npt.on;   // (a barostat: the cell record, the ring of cells)
    if (const int rp = md_prepare_call(h, nevals, st, cellrun)) return rp;
    if (m.bcm.info_d.alloc((size_t)BCM_INFO * ((size_t)nevals + 1), false)) return fail(SGPR_E_NODEVICE, "sgpr_md_run: device allocation failed");
    if (const int ru = md_upload_noise(h, nevals, noise, st)) return ru;
    const int s0 = (int)(m.run.t % RG);
    const unsigned step_a = h->step_count;
    // the current configuration in caller order, for the members (the halt words are armed: nothing has halted this call)
    hipLaunchKernelGGL(md_record_kernel, dim3((3 * N + 255) / 256), dim3(256), 0, st, N, 0, (const int *)h->d_perm.p,
                       (const double *)(m.X.p + N3 * s0), (const double *)nullptr, (const double *)nullptr, m.bcm.x.p, (double *)nullptr,
                       (double *)nullptr, (const int *)m.halt.p, (int)step_a);
    // Whatever ran on a handle since the last call — calculate() on a halt evaluates the same members, a model update binds the
    // live one to stored frames — nothing is assumed about bound frame, lists or bin populations: bound again, a checked pass
    // where the capacities are not sized for this system, lists rebuilt by the first evaluation, bin populations cleared
    // (moving cell: the cell of configuration n is in the ring once the trajectory has started — md_npt_start, below, whose own
    // checked passes size the capacities of every handle; the cell of sgpr_md_begin until then)
    if (cellrun) md_npt_cutoffs(h);
    const bool start = cellrun && !m.run.npt.started;
    auto cell_of = [&](long long n) -> const double * { return (cellrun && m.run.npt.started) ? m.slot(n)->h : m.cell.p; };
    if (const int rw = start ? SGPR_OK : md_warm(h, m.X.p + N3 * s0, cell_of(m.run.t), m.bcm.P.p + plen * K, st)) return rw;
    for (int k = 0; k < K; k++) {
        sgpr_model *mk = m.run.bcm.members[k];
        if (!md_same_system(mk, N, m.run.numbers.data(), m.run.pbc, 0, 1))
            if (const int rb = sgpr_bind_system(mk, N, m.run.numbers.data(), m.run.pbc, 0, 1)) return rb;
        if (const int rw = start ? SGPR_OK : md_warm(mk, m.bcm.x.p, cell_of(m.run.t), m.bcm.P.p + plen * k, st)) return rw;
    }
    if (start) {
        if (const int rs = md_npt_start(h, st, nevals)) return rs;
        // every slot of the ring of cells a valid cell from the start, as the ring of positions is (sgpr_md_committee): what the
        // host has enqueued behind a halt at the first evaluations bins stale slots in them
        for (int r = 2; r < 4; r++) HIPCHK(hipMemcpy(m.slot(r)->h, m.cell.p, 9 * sizeof(double), hipMemcpyDeviceToDevice));
    }
    for (int k = 0; k < K; k++)
        if (const int rl = md_reset_lists(m.run.bcm.members[k], st)) return rl;
    md_call_start(h, c);
    if (const int rl = md_reset_lists(h, st)) return rl;
    const unsigned step0 = c.step0; const double gate = c.gate;
    const bool pend0 = m.run.t > 0;   // (the closing half kick of the first configuration: due unless it is the start of the trajectory)
    const int rc_ = md_enqueue_ahead(h, nevals, st, &c.enq, [&](int j) -> int {
        const int sl = (int)((m.run.t + j) % RG);
        for (int k = 0; k < K; k++) {
            sgpr_model *mk = m.run.bcm.members[k];
            const int re = enqueue_step(mk, m.bcm.x.p, cell_of(m.run.t + j), m.bcm.P.p + plen * k, st, nullptr);
            if (re) return re;
            mk->lists_valid = true;
        }
        const int re = enqueue_step(h, m.X.p + N3 * sl, cell_of(m.run.t + j), m.bcm.P.p + plen * K, st, nullptr);
        if (re) return re;
        h->lists_valid = true;
        const int step = (int)(step0 + j);
        double *packed = m.P.p + plen * sl, *info = m.bcm.info_d.p + (size_t)BCM_INFO * j, *row = m.scal_d.p + (size_t)SGPR_MD_SCAL * j;
        hipLaunchKernelGGL(md_bcm_kernel, dim3(1), dim3(256), 0, st, N, K1, plen, (const double *)m.bcm.P.p, packed, info, gate, m.halt.p,
                           m.halt_host.dev, step, row, m.mark.dev + j);
        FinNext x;
        md_fill_integrator(m, j, noise ? m.noise.p : nullptr, pend0, x);
        x.step = step;   // (the fused loop: enqueue_step sets it)
        const bool stay = final_eval && j == nevals - 1;
        if (cellrun) md_fill_moving_cell(m, j, x);
        hipLaunchKernelGGL(cellrun ? md_bcm_move_kernel<true> : md_bcm_move_kernel<false>, dim3((N + 63) / 64), dim3(256), 0, st, N, K1, plen,
                           (const double *)m.bcm.P.p, (const double *)info, packed, m.bcm.x.p, (const int *)h->d_perm.p, x, stay ? 1 : 0);
        hipLaunchKernelGGL(md_bcm_ke_kernel, dim3(1), dim3(256), 0, st, N, (const double *)(m.KE.p + (size_t)2 * N * sl), (const int *)m.halt.p,
                           step, row);
        md_thermostat_launch(h, j, step, packed, st);   // (the barostat: from the committee's virial in `packed`; no filter: it and a committee refuse each other)
        return SGPR_OK;
    });
    for (int k = 0; k < K; k++) m.run.bcm.members[k]->lists_valid = false;
    h->lists_valid = false;
    if (rc_) return rc_;
    MdHalt r;
    if (const int rc = md_call_close(h, c, final_eval, scalars, cellrun, &r)) return rc;
    // a capacity overflowed (md_decode_halt has cleared the live handle's `warm`): the next call's checked pass grows whatever it
    // was, on whichever member
    if (r.code == 2)
        for (int k = 0; k < K; k++) m.run.bcm.members[k]->warm = false;
    if (r.done > 0) {
        m.run.bcm.info.assign(BCM_INFO, 0.0);
        HIPCHK(hipMemcpy(m.run.bcm.info.data(), m.bcm.info_d.p + (size_t)BCM_INFO * (r.done - 1), sizeof(double) * BCM_INFO, hipMemcpyDeviceToHost));
    }
    md_finish_call(h, r, scalars, m.run.nh.on, final_eval, evals_done, halt_code);
    return SGPR_OK;
}

// ---- replicas: a run whose configuration is R copies of the system evaluated by this one handle (MdRun::Rep) — the interior
// images of a band, the beads of a polymer.  Positions and packed results lie in rings of RLX_RING slots in caller atom order
// (MdState::rep); attach, readers and the frame of sgpr_md_run are here, the mode's own buffers and launches with the mode ----
typedef MdRun::Rep::Kind RepKind;
static const char *rep_attach_name(RepKind kind) { return kind == MdRun::Rep::BAND ? "sgpr_md_neb" : "sgpr_md_pimd"; }

// The close of an attach function (`who`): the rings, every slot the R initial replicas x0[R][N][3] (what runs behind a halt
// evaluates stale slots), and the run is one of `kind` with rows of `width` in its record.
static int md_replica_attach(sgpr_model *h, const char *who, RepKind kind, int R, int width, const double *x0)
{
    MdState &m = h->md;
    const size_t RN3 = (size_t)3 * m.run.N * (size_t)R;
    if (m.rep.X.alloc(RN3 * RLX_RING) || m.rep.P.alloc((size_t)sgpr_packed_len(m.run.N) * (size_t)R * RLX_RING))
        return fail(SGPR_E_NODEVICE, "%s: device allocation failed", who);
    for (int r = 0; r < RLX_RING; r++) HIPCHK(hipMemcpy(m.rep.X.p + RN3 * r, x0, sizeof(double) * RN3, hipMemcpyHostToDevice));
    m.run.rep.kind = kind; m.run.rep.R = R; m.run.rep.width = width;
    m.run.rep.info.clear();
    m.run.ring = RLX_RING;
    return SGPR_OK;
}

// Behind sgpr_md_neb_state and sgpr_md_pimd_state (`who`): positions[R][N][3] of the current configuration (which = 0) or the one
// evaluated before it (-1), packed[R][4N + 11] the replicas' results where the last sgpr_md_run evaluated that configuration, and
// the mode's velocity — one slot (FIRE's, a band) or a ring beside the positions (a polymer).  Any of them NULL.
static int md_replica_state(sgpr_model *h, const char *who, RepKind kind, double *positions, double *velocities, double *packed, int which)
{
    if (!h) return fail(SGPR_E_INVALID, "%s: bad arguments", who);
    MdState &m = h->md;
    const bool band = kind == MdRun::Rep::BAND;
    if (!m.active || m.run.rep.kind != kind) return fail(SGPR_E_INVALID, "%s: call sgpr_md_begin and %s first", who, rep_attach_name(kind));
    if (which != 0 && which != -1) return fail(SGPR_E_INVALID, "%s: which = 0 or -1", who);
    if (which == -1 && m.run.t == 0) return fail(SGPR_E_INVALID, "%s: no earlier %s", who, band ? "band" : "configuration");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t R = (size_t)m.run.rep.R, RN3 = (size_t)3 * m.run.N * R, plen = (size_t)sgpr_packed_len(m.run.N);
    const size_t sl = (size_t)((m.run.t + which + RLX_RING) % RLX_RING);
    if (positions) HIPCHK(hipMemcpy(positions, m.rep.X.p + RN3 * sl, sizeof(double) * RN3, hipMemcpyDeviceToHost));
    if (velocities) HIPCHK(hipMemcpy(velocities, band ? m.neb.V.p : m.pimd.V.p + RN3 * sl, sizeof(double) * RN3, hipMemcpyDeviceToHost));
    if (packed) HIPCHK(hipMemcpy(packed, m.rep.P.p + plen * R * sl, sizeof(double) * plen * R, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// Behind sgpr_md_neb_info and sgpr_md_pimd_info (`who`): out[count][width] = E | covmax, half a row each, of the evaluations
// first ... first + count - 1 (0 = the call's first) of the last sgpr_md_run among those that stand.
static int md_replica_info(sgpr_model *h, const char *who, RepKind kind, int first, int count, double *out)
{
    if (!h || first < 0 || count <= 0 || !out) return fail(SGPR_E_INVALID, "%s: bad arguments", who);
    const MdRun::Rep &rep = h->md.run.rep;
    if (!h->md.active || rep.kind != kind) return fail(SGPR_E_INVALID, "%s: call sgpr_md_begin and %s first", who, rep_attach_name(kind));
    const long long have = (long long)(rep.info.size() / (size_t)rep.width);
    if ((long long)first + count > have)
        return fail(SGPR_E_INVALID, "%s: evaluations %d ... %lld asked for, %lld of the last sgpr_md_run stand", who, first, (long long)first + count - 1, have);
    memcpy(out, rep.info.data() + (size_t)rep.width * first, sizeof(double) * (size_t)rep.width * (size_t)count);
    return SGPR_OK;
}

// What the mode's launches of one evaluation are given: evaluation j of the call, the value the halt words take for it, whether
// it is a `final` call's last (nothing moves), the gate, and where its replicas lie.
struct RepEval {
    hipStream_t st;
    int j, step;
    bool stay;
    double gate;
    size_t sl, sn;      // the ring slots of this configuration and the next: those of the mode's own rings too
    const double *X;    // [R][N][3] the replicas
    double *P, *Xn;     // [R][4N + 11] their packed results, filled by the plain steps in front; [R][N][3] the next configuration
    double *info;       // the evaluation's row of the record
};

// sgpr_md_run for replicas, in the shape of md_relax_run and md_committee_run: every evaluation is R plain steps of the live
// handle — replica i's caller-order positions in the ring through the handle's own binning kernel, into its own packed buffer;
// before each the handle is as md_reset_lists leaves it: every replica rebuilds its candidate lists (one list set per replica
// would save that: not done) — with the mode's kernels behind them: launch(e), a callable inlined here as md_enqueue_ahead inlines
// its own.  The halts are decided by the second of them on the evaluation itself, before anything moves: what the host has
// enqueued behind a halt evaluates stale slots and changes nothing.  The halt words count evaluations of the R replicas from the
// handle's step counter at the call's start (the handle's own counter advances R per evaluation; no plain step reads the words).
// noise: [nevals][R][N][3] uploaded as it comes into m.noise_raw, or null.
template <typename Launch>
static int md_replica_run(sgpr_model *h, int nevals, const double *noise, double ediff, int final_eval, double *scalars, int *evals_done, int *halt_code,
                          Launch launch)
{
    MdState &m = h->md;
    MdCall c;
    if (const int ro = md_call_open(h, ediff, evals_done, halt_code, c)) return ro;
    hipStream_t st = c.st;
    const int RG = RLX_RING, R = m.run.rep.R;
    const size_t plen = c.plen, N3 = (size_t)3 * c.N, RN3 = N3 * (size_t)R, width = (size_t)m.run.rep.width;
    if (const int rp = md_prepare_call(h, nevals, st, false)) return rp;
    if (m.rep.info_d.alloc(width * ((size_t)nevals + 1), false)) return fail(SGPR_E_NODEVICE, "sgpr_md_run: device allocation failed");
    HIPCHK(hipMemsetAsync(m.rep.info_d.p, 0, sizeof(double) * width * ((size_t)nevals + 1), st));
    if (noise) {
        if (m.noise_raw.alloc(RN3 * (size_t)nevals)) return fail(SGPR_E_NODEVICE, "sgpr_md_run: device allocation failed");
        HIPCHK(hipMemcpyAsync(m.noise_raw.p, noise, sizeof(double) * RN3 * (size_t)nevals, hipMemcpyHostToDevice, st));
    }
    m.run.started = true;
    m.run.rep.info.clear();
    if (!h->warm) {   // the checked pass grows capacities: over every replica
        const size_t sw = (size_t)(m.run.t % RG);
        for (int i = 0; i < R; i++)
            if (const int rc_ = run_checked(h, m.rep.X.p + RN3 * sw + N3 * i, m.cell.p, m.rep.P.p + plen * (R * sw + i), st)) return rc_;
        h->warm = true;
    }
    md_call_start(h, c);
    const unsigned step0 = c.step0; const double gate = c.gate;
    const int rc_ = md_enqueue_ahead(h, nevals, st, &c.enq, [&](int j) -> int {
        const size_t sl = (size_t)((m.run.t + j) % RG), sn = (sl + 1) % RG;
        const RepEval e = {st, j, (int)(step0 + j), final_eval && j == nevals - 1, gate, sl, sn,
                           m.rep.X.p + RN3 * sl, m.rep.P.p + plen * R * sl, m.rep.X.p + RN3 * sn, m.rep.info_d.p + width * j};
        for (int i = 0; i < R; i++) {
            if (const int rl = md_reset_lists(h, st)) return rl;
            const int re = enqueue_step(h, e.X + N3 * i, m.cell.p, e.P + plen * i, st, nullptr);
            if (re) return re;
        }
        launch(e);
        return SGPR_OK;
    });
    h->lists_valid = false;
    if (rc_) return rc_;
    MdHalt r;
    if (const int rc = md_call_close(h, c, final_eval, scalars, false, &r)) return rc;
    if (r.done > 0) {
        m.run.rep.info.assign(width * r.done, 0.0);
        HIPCHK(hipMemcpy(m.run.rep.info.data(), m.rep.info_d.p, sizeof(double) * width * (size_t)r.done, hipMemcpyDeviceToHost));
    }
    md_finish_call(h, r, scalars, true, final_eval, evals_done, halt_code);
    return SGPR_OK;
}

// ---- the nudged elastic band (sgpr_md_neb; md_neb.inc has the scheme, workloads.neb_fire is the host twin) ----
// For the run begun by sgpr_md_begin (any interior image as its positions: they bind the system; masses, velocities, dt,
// friction and kT are ignored) and, if used, sgpr_md_fix — one mask for every image —, before the first sgpr_md_run.
// positions[K + 2][N][3]: the band in caller atom order, images 0 and K + 1 the fixed ends; fire as in sgpr_md_relax.
// sgpr_md_run then evaluates the K interior images with this one handle, moves them with FIRE, and stops with halt code 3 at
// the first band whose largest |G_row|^2 over all K N rows is below fmax^2.  Constant cell, one rank.
static int md_neb_init_state(sgpr_model *h)
{
    MdState &m = h->md;
    double s[RLX_LEN] = {};
    s[RLX_DT] = m.run.relax.par.dt0; s[RLX_A] = m.run.relax.par.astart; s[RLX_NSTEPS] = 0.0; s[RLX_FRESH] = 1.0;
    HIPCHK(hipMemcpy(m.relax.state.p, s, sizeof(s), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(m.neb.V.p, 0, sizeof(double) * 3 * (size_t)m.run.N * (size_t)m.run.rep.R));
    return SGPR_OK;
}

extern "C" int sgpr_md_neb(sgpr_model *h, int K, const double *positions, double fmax, double k_spring, int climb, const double *fire)
{
#pragma clang fp contract(off)
    if (!h || !positions) return fail(SGPR_E_INVALID, "sgpr_md_neb: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_neb: call sgpr_md_begin first");
    if (K < 1 || K > NEB_MAX) return fail(SGPR_E_INVALID, "sgpr_md_neb: %d interior images; a band has 1 to %d", K, NEB_MAX);
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run was begun on %d ranks; a band runs on one", m.run.world);
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_neb: the run has started");
    if (m.run.nh.on || m.run.npt.on) return fail(SGPR_E_INVALID, "sgpr_md_neb: the run has a thermostat or a barostat");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run has a committee (sgpr_md_committee), which serves dynamics only");
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run has a bias (sgpr_md_meta), which serves dynamics only; the host loop around calculate() serves a biased band");
    if (m.run.filter.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run has a filter (sgpr_md_filter), which serves dynamics only");
    if (m.run.relax.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run is a relaxation (sgpr_md_relax); a band moves at constant cell under its own FIRE");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run is a ring polymer (sgpr_md_pimd)");
    if (m.run.rec.every) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: a frame record is armed (sgpr_md_record); a band records no frames");
    if (const MdAcc *a = md_acc_attached(m.run)) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_neb: the run accumulates %s (%s), which serve dynamics only", a->noun, a->fn);
    if (!(fmax > 0.0) || !(k_spring > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_neb: fmax > 0 and k_spring > 0");
    RelaxParams p = {};
    if (const int rf = md_fire_keywords("sgpr_md_neb", fire, p)) return rf;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N;
    const size_t N3 = (size_t)3 * N;
    NebCell cl = {};
    HIPCHK(hipMemcpy(cl.h, m.cell.p, sizeof(cl.h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) cl.pbc[k] = m.run.pbc[k] ? 1 : 0;
    const bool any_pbc = cl.pbc[0] || cl.pbc[1] || cl.pbc[2];
    if (any_pbc) {
        if (!(fabs(rlx_det(cl.h)) > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_neb: the cell is singular");
        rlx_m3_inv(cl.h, cl.hi);
    }
    // The rounding recovers a displacement only when it is well inside half a cell: no fractional component of a displacement
    // after rounding at +-1/2 (where rint may go either way from one evaluation to the next), and the displacement after
    // rounding no longer than half the smallest perpendicular width of the periodic directions (beyond it another image of
    // the atom may be the nearer one).  The initial band only: the user keeps the images closer than that.
    double wmin = 1e300;
    for (int k = 0; k < 3; k++)
        if (cl.pbc[k]) wmin = std::min(wmin, 1.0 / sqrt((cl.hi[k] * cl.hi[k] + cl.hi[3 + k] * cl.hi[3 + k]) + cl.hi[6 + k] * cl.hi[6 + k]));
    for (int i = 1; i <= K + 1; i++)
        for (int c = 0; c < N; c++) {
            const double *a = positions + N3 * (size_t)(i - 1) + 3 * (size_t)c, *b = positions + N3 * (size_t)i + 3 * (size_t)c;
            const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            double o[3];
            neb_mic(cl, d[0], d[1], d[2], o[0], o[1], o[2]);
            for (int k = 0; k < 3 && any_pbc; k++) {
                const double sfr = (o[0] * cl.hi[k] + o[1] * cl.hi[3 + k]) + o[2] * cl.hi[6 + k];
                if (cl.pbc[k] && fabs(sfr) >= 0.5 - 1e-9)
                    return fail(SGPR_E_INVALID, "sgpr_md_neb: atom %d moves half a cell (fractional %.6f along vector %d) between images %d and %d: "
                                "the minimum-image rounding cannot recover it; add images", c, sfr, k, i - 1, i);
            }
            const double len = sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
            if (any_pbc && len > 0.5 * wmin)
                return fail(SGPR_E_INVALID, "sgpr_md_neb: atom %d moves %.4f between images %d and %d, more than half the smallest perpendicular "
                            "width of the cell (%.4f): the minimum-image rounding cannot recover it; add images", c, len, i - 1, i, wmin);
        }
    for (int k = 0; k < 9; k++) p.h0[k] = cl.h[k];
    p.fmax2 = fmax * fmax;
    p.cf = (double)N; p.cell = 0;
    if (m.neb.V.alloc(N3 * (size_t)K) || m.neb.ends.alloc(2 * N3) || m.neb.sums.alloc((size_t)NEB_SUMS * K) || m.neb.coef.alloc((size_t)2 * K) ||
        m.relax.state.alloc(RLX_LEN) || m.neb.par.alloc(sizeof(NebFirePar)))
        return fail(SGPR_E_NODEVICE, "sgpr_md_neb: device allocation failed");
    HIPCHK(hipMemcpy(m.neb.ends.p, positions, sizeof(double) * N3, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.neb.ends.p + N3, positions + N3 * (size_t)(K + 1), sizeof(double) * N3, hipMemcpyHostToDevice));
    NebFirePar par = {};
    par.cell = cl; par.p = p; par.kspr = k_spring; par.climb = climb ? 1 : 0;
    HIPCHK(hipMemcpy(m.neb.par.p, &par, sizeof(par), hipMemcpyHostToDevice));
    if (const int ra = md_replica_attach(h, "sgpr_md_neb", MdRun::Rep::BAND, K, NEB_INFO, positions + N3)) return ra;
    m.run.relax.par = p;
    m.run.neb.cell = cl; m.run.neb.on = true;
    return md_neb_init_state(h);
}

// optimizer.initialize() for the band: v = 0 and dt, a, nsteps back to their start (the reference's "model updated -> restart!")
extern "C" int sgpr_md_neb_reset(sgpr_model *h)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_neb_reset: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.neb.on) return fail(SGPR_E_INVALID, "sgpr_md_neb_reset: call sgpr_md_begin and sgpr_md_neb first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return md_neb_init_state(h);
}

// The K interior images in caller atom order: positions[K][N][3] of the current band (which = 0) or the one evaluated before it
// (-1), velocities[K][N][3] FIRE's, packed[K][4N + 11] the images' results where the last sgpr_md_run evaluated that band
// (a halted or `final` call: which = 0; a call that ran through: which = -1).  Any of them NULL.
extern "C" int sgpr_md_neb_state(sgpr_model *h, double *positions, double *velocities, double *packed, int which)
{
    return md_replica_state(h, "sgpr_md_neb_state", MdRun::Rep::BAND, positions, velocities, packed, which);
}

// The band record of the last sgpr_md_run: out[count][32] = E[16] | covmax[16] (image i at entry i - 1, the rest zero) of its
// evaluations first ... first + count - 1 (0 = the call's first) among those that stand.
extern "C" int sgpr_md_neb_info(sgpr_model *h, int first, int count, double *out)
{
    return md_replica_info(h, "sgpr_md_neb_info", MdRun::Rep::BAND, first, count, out);
}

// sgpr_md_run for a band: md_replica_run over the K interior images with md_neb_sums_kernel, md_neb_fire_kernel — it decides the
// halts: covloss gate (1), capacity overflow at any image (2), convergence (3) — and md_neb_move_kernel behind them.
static int md_neb_run(sgpr_model *h, int nevals, double ediff, int final_eval, double *scalars, int *evals_done, int *halt_code)
{
    MdState &m = h->md;
    const int N = m.run.N, K = m.run.rep.R;
    const size_t plen = (size_t)sgpr_packed_len(N);
    return md_replica_run(h, nevals, nullptr, ediff, final_eval, scalars, evals_done, halt_code, [&](const RepEval &e) {
        const NebBand b = {N, K, plen, e.X, m.neb.ends.p, e.P, h->d_perm.p, m.fix()};
        hipLaunchKernelGGL(md_neb_sums_kernel, dim3(K), dim3(256), 0, e.st, b, m.run.neb.cell, m.neb.sums.p, (const int *)m.halt.p, e.step);
        hipLaunchKernelGGL(md_neb_fire_kernel, dim3(1), dim3(256), 0, e.st, b, (const NebFirePar *)m.neb.par.p, m.relax.state.p, (const double *)m.neb.V.p,
                           (const double *)m.neb.sums.p, m.neb.coef.p, e.info, e.gate, m.halt.p, m.halt_host.dev, e.step,
                           m.scal_d.p + (size_t)SGPR_MD_SCAL * e.j, m.mark.dev + e.j, e.stay ? 1 : 0);
        if (!e.stay)
            hipLaunchKernelGGL(md_neb_move_kernel, dim3((N + 63) / 64, K), dim3(256), 0, e.st, b, m.run.neb.cell, (const double *)m.relax.state.p,
                               (const double *)m.neb.coef.p, m.neb.V.p, e.Xn, (const int *)m.halt.p, e.step);
    });
}

// ---- path-integral MD (sgpr_md_pimd; md_pimd.inc has the scheme, workloads.pimd_baoab is the host twin) ----
// For the run begun by sgpr_md_begin (any bead as its positions: they bind the system; its masses and dt hold, its velocities,
// friction and kT are replaced by what is given here), before the first sgpr_md_run.  positions[P][N][3], velocities[P][N][3]
// (NULL: zeros): the beads in caller atom order; kT: the physical one — the polymer is sampled at P kT with w_P = P kT / hbar,
// hbar in the units of eV, A and amu (PIMD_HBAR); friction: the centroid's, lambda: gamma_k = 2 lambda w_k of the other modes.
// The tables of the run — C, the free ring polymer's propagator over dt / 2, c1_k and c2_k — are computed here, once, in the
// operations of workloads.pimd_tables.  sgpr_md_run then evaluates the P beads with this one handle and moves them; its noise
// is [nevals][P][N][3] (mode k, caller atom order).  Constant cell, one rank, nothing else attached.
extern "C" int sgpr_md_pimd(sgpr_model *h, int P, const double *positions, const double *velocities, double kT, double friction, double lambda)
{
#pragma clang fp contract(off)
    if (!h || !positions) return fail(SGPR_E_INVALID, "sgpr_md_pimd: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_pimd: call sgpr_md_begin first");
    if (P < 1 || P > PIMD_MAX) return fail(SGPR_E_INVALID, "sgpr_md_pimd: %d beads; a polymer has 1 to %d", P, PIMD_MAX);
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run was begun on %d ranks; a polymer runs on one", m.run.world);
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_pimd: the run has started");
    if (m.run.nh.on || m.run.npt.on) return fail(SGPR_E_INVALID, "sgpr_md_pimd: the run has a thermostat or a barostat; a polymer runs at constant cell under its own thermostat");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run has a committee (sgpr_md_committee); a polymer is evaluated by one model");
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run has a bias (sgpr_md_meta), which the polymer's loop does not apply; the host loop around calculate() serves it");
    if (m.run.filter.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run has a filter (sgpr_md_filter); a polymer integrates unfiltered forces");
    if (m.run.fix.n) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: %d components are held (sgpr_md_fix); a polymer runs without a mask", m.run.fix.n);
    if (m.run.rec.every) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: a frame record is armed (sgpr_md_record); a polymer records no frames");
    if (const MdAcc *a = md_acc_attached(m.run)) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run accumulates %s (%s); a polymer's %s not sampled", a->noun, a->fn, a->polymer);
    if (m.run.relax.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run is a relaxation (sgpr_md_relax)");
    if (m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_pimd: the run is a nudged elastic band (sgpr_md_neb)");
    if (m.run.pimd.on) return fail(SGPR_E_INVALID, "sgpr_md_pimd: the run is a polymer already");
    if (!(kT > 0.0) || friction < 0.0 || lambda < 0.0) return fail(SGPR_E_INVALID, "sgpr_md_pimd: kT > 0, friction >= 0, lambda >= 0");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N;
    const size_t N3 = (size_t)3 * N, PN3 = N3 * (size_t)P;
    const double dt = m.run.dt, hdt = m.run.hdt, dP = (double)P;
    const double kTP = dP * kT, wP = kTP / PIMD_HBAR;
    std::vector<double> tab((size_t)P * P + 5 * (size_t)P);
    for (int j = 0; j < P; j++)
        for (int k = 0; k < P; k++) {
            const double arg = (2.0 * M_PI * (double)((j * k) % P)) / dP;
            double c;
            if (k == 0) c = sqrt(1.0 / dP);
            else if (2 * k < P) c = sqrt(2.0 / dP) * cos(arg);
            else if (2 * k == P) c = (j & 1) ? -sqrt(1.0 / dP) : sqrt(1.0 / dP);
            else c = sqrt(2.0 / dP) * sin(arg);
            tab[(size_t)j * P + k] = c;
        }
    double *cs = tab.data() + (size_t)P * P, *sn = cs + P, *wsn = sn + P, *c1 = wsn + P, *c2 = c1 + P;
    for (int k = 0; k < P; k++) {
        const double wk = k ? (2.0 * wP) * sin(((double)k * M_PI) / dP) : 0.0;
        const double s = sin(wk * hdt);
        cs[k] = cos(wk * hdt);
        sn[k] = k ? s / wk : hdt;
        wsn[k] = wk * s;
        const double g = k ? (2.0 * lambda) * wk : friction;
        c1[k] = exp(-(g * dt));
        c2[k] = sqrt(1.0 - c1[k] * c1[k]);
    }
    std::vector<double> sq(N);
    for (int i = 0; i < N; i++) sq[i] = sqrt(kTP / m.run.mass_sorted[i]);
    if (m.pimd.V.alloc(PN3 * RLX_RING) || m.pimd.sums.alloc((size_t)PIMD_SUMS * P) || m.pimd.tab.alloc(tab.size()) || m.pimd.sq.alloc(N))
        return fail(SGPR_E_NODEVICE, "sgpr_md_pimd: device allocation failed");
    HIPCHK(hipMemset(m.pimd.V.p, 0, sizeof(double) * PN3 * RLX_RING));
    if (velocities) HIPCHK(hipMemcpy(m.pimd.V.p, velocities, sizeof(double) * PN3, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.pimd.tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.pimd.sq.p, sq.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    if (const int ra = md_replica_attach(h, "sgpr_md_pimd", MdRun::Rep::POLYMER, P, PIMD_INFO, positions)) return ra;
    m.run.pimd.kT = kT; m.run.pimd.wP2 = wP * wP;
    m.run.pimd.on = true;
    return SGPR_OK;
}

// The P beads in caller atom order: positions[P][N][3] of the current configuration (which = 0) or the one evaluated before it
// (-1), velocities_pre[P][N][3] BEFORE its closing half kick (due at every configuration but the start of the trajectory:
// v = v_pre + (dt/2) F / m once F is known), packed[P][4N + 11] the beads' results where the last sgpr_md_run evaluated that
// configuration (a halted or `final` call: which = 0; a call that ran through: which = -1).  Any of them NULL.
extern "C" int sgpr_md_pimd_state(sgpr_model *h, double *positions, double *velocities_pre, double *packed, int which)
{
    return md_replica_state(h, "sgpr_md_pimd_state", MdRun::Rep::POLYMER, positions, velocities_pre, packed, which);
}

// The record of the last sgpr_md_run: out[count][64] = E[32] | covmax[32] (bead j at entry j, the rest zero) of its evaluations
// first ... first + count - 1 (0 = the call's first) among those that stand.
extern "C" int sgpr_md_pimd_info(sgpr_model *h, int first, int count, double *out)
{
    return md_replica_info(h, "sgpr_md_pimd_info", MdRun::Rep::POLYMER, first, count, out);
}

// sgpr_md_run for a polymer: md_replica_run over the P beads with md_pimd_sums_kernel, md_pimd_gate_kernel — it decides the
// halts: covloss gate (1), capacity overflow at any bead (2) — and md_pimd_move_kernel behind them; the repeat of a halted
// evaluation finds x and v of its slot as they were.  noise: [nevals][P][N][3], caller atom order (the move kernel goes through
// the permutation anyway).
static int md_pimd_run(sgpr_model *h, int nevals, const double *noise, double ediff, int final_eval, double *scalars, int *evals_done, int *halt_code)
{
    MdState &m = h->md;
    const int N = m.run.N, P = m.run.rep.R;
    const size_t plen = (size_t)sgpr_packed_len(N), PN3 = (size_t)3 * N * (size_t)P;
    const bool pend0 = m.run.t > 0;   // (the closing half kick of the first configuration: due unless it is the start of the trajectory)
    const size_t lds = sizeof(double) * ((size_t)4 * P * 3 * PIMD_TILE + (size_t)P * P);
    return md_replica_run(h, nevals, noise, ediff, final_eval, scalars, evals_done, halt_code, [&](const RepEval &e) {
        const PimdRing b = {N, P, plen, e.X, m.pimd.V.p + PN3 * e.sl, e.P, h->d_perm.p, m.mass.p, m.run.hdt, (e.j > 0 || pend0) ? 1 : 0};
        hipLaunchKernelGGL(md_pimd_sums_kernel, dim3(P), dim3(256), 0, e.st, b, m.pimd.sums.p, (const int *)m.halt.p, e.step);
        hipLaunchKernelGGL(md_pimd_gate_kernel, dim3(1), dim3(64), 0, e.st, N, P, (const double *)m.pimd.sums.p, m.run.pimd.kT, m.run.pimd.wP2,
                           e.info, e.gate, m.halt.p, m.halt_host.dev, e.step, m.scal_d.p + (size_t)SGPR_MD_SCAL * e.j, m.mark.dev + e.j);
        if (!e.stay) {
            const PimdMove a = {m.pimd.sq.p, m.pimd.tab.p, noise ? m.noise_raw.p + PN3 * (size_t)e.j : nullptr, e.Xn, m.pimd.V.p + PN3 * e.sn,
                                noise ? 0ull : m.seed, m.run.t + e.j};
            hipLaunchKernelGGL(md_pimd_move_kernel, dim3((N + PIMD_TILE - 1) / PIMD_TILE), dim3(256), lds, e.st, b, a, (const int *)m.halt.p, e.step);
        }
    });
}

// Evaluates `nevals` configurations starting with the current one; after each evaluation but (with `final`) the last
// the integrator moves on with the next row of `noise` ([nevals][N][3] standard normal deviates, caller atom order; null:
// velocity Verlet).  Stops at the first evaluation whose largest covloss reaches `ediff` (<= 0: never): *evals_done
// counts the evaluations whose results stand, the halting one included; the state then IS that configuration (its
// forces are evaluated again by the next call — after the caller has updated the model).
// scalars: [nevals][SGPR_MD_SCAL] = E, virial(9), overflow, largest covloss, sum m v^2 (closed | before the closing half
// kick), 0, 0 per evaluation.
extern "C" int sgpr_md_run(sgpr_model *h, int nevals, const double *noise, double ediff, int final_eval, double *scalars,
                           int *evals_done, int *halt_code)
{
    if (!h || nevals <= 0 || !evals_done) return fail(SGPR_E_INVALID, "sgpr_md_run: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_run: call sgpr_md_begin first");
    if (!(h->m > 0 && h->has_mu)) return fail(SGPR_E_NOMODEL, "sgpr_md_run: the model has no weights");
    if (m.run.relax.on) return md_relax_run(h, nevals, ediff, final_eval, scalars, evals_done, halt_code);
    if (m.run.neb.on) return md_neb_run(h, nevals, ediff, final_eval, scalars, evals_done, halt_code);
    if (m.run.pimd.on) return md_pimd_run(h, nevals, noise, ediff, final_eval, scalars, evals_done, halt_code);
    if (!m.run.bcm.members.empty()) return md_committee_run(h, nevals, noise, ediff, final_eval, scalars, evals_done, halt_code);
    MdCall c;
    if (const int ro = md_call_open(h, ediff, evals_done, halt_code, c)) return ro;
    if (m.run.world > 1 && !(peer_on(h) && h->peer.world == m.run.world && h->peer.rank == m.run.rank))
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the run was begun on %d ranks, the exchange between them is gone", m.run.world);
    hipStream_t st = c.st;
    const int N = c.N;
    const size_t plen = c.plen;
    if (m.run.meta.on) {
        // the bias rides in the single-rank gather form of the fused last kernel: what cannot take that form is refused here, before
        // anything is enqueued (md_before_last keeps the step's own check for what only a checked pass finds out: lists beyond the gather form)
        if (!md_gather_form(h))
            return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bias (sgpr_md_meta) runs in the gather form of the fused last kernel only (one rank, no graph "
                        "replay, no side-stream fork, a skin > 0): the host loop around calculate() serves this run");
        if (const int rq = md_meta_ql_fits(h, ": the host loop around calculate() serves this run")) return rq;
        // the last configuration of the call that deposits a hill must find its row
        const long long nd = (m.run.t + nevals - 1) / m.run.meta.pace * m.run.meta.pace;
        if (nd >= m.run.t && m.run.meta_slot(nd) >= m.run.meta.cap)
            return fail(SGPR_E_INVALID, "sgpr_md_run: %d evaluations from configuration %lld deposit hills up to row %lld; the bias holds %lld "
                        "(sgpr_md_meta again, with a larger capacity and the hills of sgpr_md_meta_hills)", nevals, m.run.t, m.run.meta_slot(nd), m.run.meta.cap);
        if (m.run.meta.merge) {
            // where the table stands: merges enqueued behind a halt were discarded, the one of the speculative step in front of it was not
            int ctl[META_CTL_LEN];
            HIPCHK(hipMemcpyAsync(ctl, m.meta.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            m.run.meta.enq = ctl[META_CTL_DONE];
        }
        m.run.meta.fresh = false;
    }
    if (m.run.adf.every) {
        // the bond angles read the list that the forward pass leaves behind the fused last kernel: the forms md_meta's qlvar takes
        if (!md_gather_form(h))
            return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bond angles (sgpr_md_adf) read the step's neighbour list behind the gather form of the fused last "
                        "kernel only (one rank, no graph replay, no side-stream fork, a skin > 0): the frame record and workloads.AdfCounts serve this run");
        size_t bytes = 0;
        if (h->maxnn > 0 && !md_adf_waves(m.run.adf, h->maxnn, bytes))
            return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the bond angles (sgpr_md_adf) keep a centre's neighbours in LDS; a list of up to %d entries per atom with "
                        "%d bins and %d species does not fit %d bytes", h->maxnn, m.run.adf.bins, m.run.adf.S, ADF_LDS_BYTES);
    }
    m.run.started = true;
    MdBinIdentity guard(h);
    if (const int rp = md_prepare_call(h, nevals, st, m.run.npt.on)) return rp;   // (the cell record: a moving cell only)
    if (const int ru = md_upload_noise(h, nevals, noise, st)) return ru;
    const int RG = m.run.ring, s0 = (int)(m.run.t % RG);
    if (m.run.npt.on) md_npt_cutoffs(h);
    if (m.run.npt.on && !m.run.npt.started)
        if (const int rs = md_npt_start(h, st)) return rs;
    // (moving cell: the cell of configuration n is in the ring)
    auto cell_of = [&](long long n) -> const double * { return m.run.npt.on ? m.slot(n)->h : m.cell.p; };
    if (const int rw = md_warm(h, m.X.p + (size_t)3 * N * s0, cell_of(m.run.t), m.P.p + plen * s0, st)) return rw;
    // the continuation of the last call (nothing else ran on the handle since, no re-binding, no option touched): its candidate
    // lists stand and its last kernel has binned this call's first configuration.  Otherwise: whatever ran in between — a model
    // update evaluates other frames — may have left other lists and bin populations (a run that halted: those of a step that
    // never ran)
    const bool chain = m.run.chain.ok && h->warm && h->step_count == m.run.chain.step && h->bind_gen == m.run.chain.bind && h->opt_gen == m.run.chain.opt &&
                       m.run.t == m.run.chain.t && m.run.chain.pos == m.X.p + (size_t)3 * N * s0;
    md_call_start(h, c);
    if (chain) {
        h->lists_valid = true;
        h->pre_valid = true; h->pre_pos = m.run.chain.pos; h->pre_cell = cell_of(m.run.t); h->pre_step = h->step_count;
    } else if (const int rl = md_reset_lists(h, st))
        return rl;
    const unsigned step0 = c.step0;
    const unsigned epoch0 = h->peer.epoch;
    const bool pend0 = m.run.t > 0;   // (the closing half kick of the first configuration: due unless it is the start of the trajectory)
    const int rc_ = md_enqueue_ahead(h, nevals, st, &c.enq, [&](int j) -> int {
        const int sl = (int)((m.run.t + j) % RG), sn = (sl + 1) % RG, sp = (sl + RG - 1) % RG;
        StepNext nx;
        nx.mode = 2;
        nx.pos_next = m.X.p + (size_t)3 * N * sn;
        FinNext &x = nx.md;
        md_fill_integrator(m, j, noise ? m.noise.p : nullptr, pend0, x);
        if (m.run.npt.on) {
            md_fill_moving_cell(m, j, x);
            nx.cell_next = x.npt_next->h;
            h->step_grid = &x.npt_cur->grid;
        }
        x.fixed = m.fix();
        x.ke_prev = j > 0 ? m.KE.p + (size_t)2 * N * sp : nullptr;
        x.packed_prev = j > 0 ? m.P.p + plen * sp : nullptr;
        x.ediff = c.gate;
        x.halt_host = m.halt_host.dev;
        x.scal_cur = m.scal_d.p + (size_t)SGPR_MD_SCAL * j; x.scal_prev = m.scal_d.p + (size_t)SGPR_MD_SCAL * (j > 0 ? j - 1 : 0);
        x.mark_cur = m.mark.dev + j;
        // (the last evaluation of a `final` run integrates speculatively too: its outcome is not adopted below)
        const int re = enqueue_step(h, x.x_cur, cell_of(m.run.t + j), m.P.p + plen * sl, st, &nx);
        if (re) return re;
        h->lists_valid = true;  // (the first evaluation rebuilt the candidates; an overflow halts the run: FinNext)
        if (!h->pre_valid) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_run: the fused last kernel is not available for this model / frame (sharded "
                                        "without the library's own exchange, graph capture or a zero skin)");
        md_thermostat_launch(h, j, (int)(step0 + j), m.P.p + plen * sl, st);
        // (the frame: the last kernel has written this evaluation's results and, Nose-Hoover, its centred velocity; the slots
        // read here are written again only when the rings come round)
        if (m.run.rec.every && (m.run.t + j) % m.run.rec.every == 0) md_record_frame(h, j, (int)(step0 + j), st);
        return md_sample_due(h, j, (int)(step0 + j), st);
    });
    if (rc_) return rc_;
    const int enq = c.enq;
    if (enq > 0) {  // the lagged reductions of the last evaluation enqueued
        FinArgs f = {};
        f.N = N;
        const int sl = (int)((m.run.t + enq - 1) % RG);
        f.nx.mode = 3; f.nx.step = (int)(step0 + enq);
        f.nx.ke_prev = m.KE.p + (size_t)2 * N * sl; f.nx.packed_prev = m.P.p + plen * sl;
        f.nx.ediff = c.gate; f.nx.halt = m.halt.p; f.nx.halt_host = m.halt_host.dev;
        f.nx.scal_prev = m.scal_d.p + (size_t)SGPR_MD_SCAL * (enq - 1);
        hipLaunchKernelGGL(finalize_tail_kernel, dim3(2), dim3(256), 0, st, f);
    }
    if (const int rc = md_collect(h, enq, st, scalars, m.run.npt.on)) return rc;
    if (const int pc = peer_check(h)) return pc;
    // Where the run goes on: when every evaluation stands and the last one was integrated, the handle is left as the last kernel
    // left it — the next sgpr_md_run continues from there (chain, above).  Otherwise the last kernel enqueued has binned a step
    // that will not run — or, after a halt, the bins are those of a discarded speculative step: whoever uses the handle next
    // starts from clean bin populations.
    const bool keep_chain = md_halt_step(m) == MD_HALT_NONE && !final_eval && enq == nevals && h->pre_valid;
    const double *keep_pos = h->pre_pos;
    // (the flags md_reset_lists clears with the populations are read by nobody before this function clears them itself on its
    // way out: lists_valid below, pre_valid when `guard` goes; keep_chain and keep_pos were taken above)
    if (!keep_chain)
        if (const int rl = md_reset_lists(h, st)) return rl;
    MdHalt r;
    if (const int rd = md_decode_halt(h, step0, enq, final_eval, m.run.npt.on, &r)) return rd;
    md_record_close(m, r);
    // exchanges that took place: the ranks have enqueued different numbers of evaluations behind the halt, all of them
    // skipped on the device (peer_push_kernel): a covloss halt at evaluation k is seen by evaluation k + 1 (or by the
    // tail kernel when k is the last), an overflow by evaluation k itself — the same count on every rank
    if (r.code && peer_on(h)) {
        h->peer.epoch = epoch0 + (unsigned)(r.code == 2 ? r.k + 1 : std::min(nevals, r.k + 2));
        if (getenv("SGPR_PEER_TRACE"))
            fprintf(stderr, "[sgpr peer] rank %d md_run halt: code %d k %d enq %d nevals %d -> epoch %u\n", h->peer.rank, r.code, r.k, enq, nevals, h->peer.epoch);
    }
    if (keep_chain) {
        m.run.chain.ok = true; m.run.chain.step = h->step_count; m.run.chain.bind = h->bind_gen; m.run.chain.opt = h->opt_gen; m.run.chain.t = m.run.t;
        m.run.chain.pos = keep_pos;
    }
    md_finish_call(h, r, scalars, m.run.nh.on, final_eval, evals_done, halt_code);
    return SGPR_OK;
}

// One slot of a device ring (N rows of three, sorted order) in caller atom order — through the run's OWN permutation: the
// handle may be bound to another frame by now
static int md_fetch_rows(const MdState &m, const double *slot_dev, double *out)
{
    std::vector<double> buf((size_t)3 * m.run.N);
    HIPCHK(hipMemcpy(buf.data(), slot_dev, sizeof(double) * 3 * m.run.N, hipMemcpyDeviceToHost));
    for (int i = 0; i < m.run.N; i++)
        for (int k = 0; k < 3; k++) out[3 * (size_t)m.run.perm[i] + k] = buf[3 * (size_t)i + k];
    return SGPR_OK;
}

// State of the run in caller atom order: positions of the current configuration, its velocities BEFORE the closing half
// kick (`pending` says whether one is due: v = v_pre + (dt/2) F / m once F is known), and — when the configuration has
// been evaluated by the last sgpr_md_run (a halted or `final` run) — its packed results [F | beta | E | virial | overflow].
extern "C" int sgpr_md_state(sgpr_model *h, double *positions, double *velocities_pre, int *pending, double *packed,
                             int which /*0: the current configuration; -1: the one evaluated before it*/)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_state: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_state: call sgpr_md_begin first");
    if (m.run.neb.on) return fail(SGPR_E_INVALID, "sgpr_md_state: the run is a nudged elastic band; sgpr_md_neb_state returns its images");
    if (m.run.pimd.on) return fail(SGPR_E_INVALID, "sgpr_md_state: the run is a ring polymer; sgpr_md_pimd_state returns its beads");
    if (which != 0 && which != -1) return fail(SGPR_E_INVALID, "sgpr_md_state: which = 0 or -1");
    if (which == -1 && m.run.t == 0) return fail(SGPR_E_INVALID, "sgpr_md_state: no earlier configuration");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N;
    const int sl = (int)((m.run.t + which + m.run.ring) % m.run.ring);
    int rc_ = positions ? md_fetch_rows(m, m.X.p + (size_t)3 * N * sl, positions) : SGPR_OK;
    // (a relaxation: the optimizer's velocity of the atoms' coordinates, one slot)
    if (!rc_ && velocities_pre) rc_ = md_fetch_rows(m, m.V.p + (size_t)3 * N * (m.run.relax.on ? 0 : sl), velocities_pre);
    // Nose-Hoover: what the integrator holds when it asks for the forces of configuration n is the centred velocity of
    // configuration n - 1 (ASE sets the momenta of a step after its force call); sgpr_md_velocities has v_n itself
    if (!rc_ && m.run.nh.on && velocities_pre && (m.run.t + which) > 0) rc_ = md_fetch_rows(m, m.V.p + (size_t)3 * N * ((sl + m.run.ring - 1) % m.run.ring), velocities_pre);
    if (rc_) return rc_;
    if (pending) *pending = (!m.run.nh.on && !m.run.relax.on && (m.run.t + which) > 0) ? 1 : 0;   // (every configuration but the start of the trajectory)
    if (packed) HIPCHK(hipMemcpy(packed, m.P.p + (size_t)sgpr_packed_len(N) * sl, sizeof(double) * sgpr_packed_len(N), hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// The velocities an observer of the trajectory sees at the current configuration, which the last sgpr_md_run must have
// evaluated (it halted there, or ran with final_eval): Langevin / velocity Verlet: the closing half kick applied; Nose-Hoover:
// the centred velocity (x_(n+1) - x_(n-1)) / 2 dt.  Caller atom order.
extern "C" int sgpr_md_velocities(sgpr_model *h, double *velocities)
{
    if (!h || !velocities) return fail(SGPR_E_INVALID, "sgpr_md_velocities: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_velocities: call sgpr_md_begin first");
    if (m.run.relax.on) return fail(SGPR_E_INVALID, "sgpr_md_velocities: the run is a relaxation");
    if (m.run.neb.on) return fail(SGPR_E_INVALID, "sgpr_md_velocities: the run is a nudged elastic band; sgpr_md_neb_state returns its images and FIRE's velocity");
    if (m.run.pimd.on) return fail(SGPR_E_INVALID, "sgpr_md_velocities: the run is a ring polymer; sgpr_md_pimd_state returns its beads and their velocities");
    if (!m.run.evaluated) return fail(SGPR_E_INVALID, "sgpr_md_velocities: the current configuration has not been evaluated (run with final_eval, or after a halt)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = m.run.N, sl = (int)(m.run.t % m.run.ring);
    if (const int rc_ = md_fetch_rows(m, m.V.p + (size_t)3 * N * sl, velocities)) return rc_;
    std::vector<double> F;
    const bool kick = !m.run.nh.on && m.run.t > 0;
    if (kick) {
        F.resize((size_t)3 * N);   // (packed forces are in caller order)
        HIPCHK(hipMemcpy(F.data(), m.P.p + (size_t)sgpr_packed_len(N) * sl, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
        if (m.run.filter.on) {   // (the kick the filtered integrator gives: finalize_next_kernel<5>'s operations)
#pragma clang fp contract(off)
            std::vector<double> a((size_t)3 * N);
            if (const int rc_ = md_fetch_rows(m, m.filter.f.p + (size_t)3 * N * sl, a.data())) return rc_;
            for (size_t e = 0; e < (size_t)3 * N; e++) F[e] = F[e] - std::min(std::max(a[e] * m.run.filter.shrink, -1.0), 1.0);
        }
    }
    for (int i = 0; i < N; i++) {
        const size_t c = m.run.perm[i];
        for (int k = 0; k < 3; k++)
            if (m.run.fix.n && m.run.fix.sorted[3 * (size_t)i + k]) velocities[3 * c + k] = 0.0;   // (a held component: F = 0, v = 0)
            else if (kick) velocities[3 * c + k] = velocities[3 * c + k] + m.run.hdt * F[3 * c + k] / m.run.mass_sorted[i];
    }
    return SGPR_OK;
}

// The frame record (md_record.inc): what a trajectory writer needs of a run that is not cut for it — the reference's writers
// are attached to the host loop with `loginterval` (cl/md.py:24-26, :117-128, :155-166) and its optimizers take trajectory=
// (cl/relax.py).  every >= 1: from the next sgpr_md_run on, the evaluation of every configuration n with n % every == 0 is
// followed by one launch that copies the configuration out, in caller atom order; 0: off.  what: bit 0 the velocities the
// integrator holds (sgpr_md_state's velocities_pre), bit 1 the packed results; positions always.  Between any two calls of a
// run (the interval belongs to the writer, not to the integrator); sgpr_md_begin switches it off.
extern "C" int sgpr_md_record(sgpr_model *h, int every, int what)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_record: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_record: call sgpr_md_begin first");
    if (every < 0 || (what & ~3)) return fail(SGPR_E_INVALID, "sgpr_md_record: every >= 0, what = bit 0 (velocities) | bit 1 (results)");
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_record: the run was begun on %d ranks; frames are recorded on one", m.run.world);
    if (every && !m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_record: the run has a committee (sgpr_md_committee), which records no frames");
    if (every && m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_record: the run is a nudged elastic band (sgpr_md_neb), which records no frames; sgpr_md_neb_state behind a cut call serves trajectories");
    if (every && m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_record: the run is a ring polymer (sgpr_md_pimd), which records no frames; sgpr_md_pimd_state behind a cut call serves trajectories");
    m.run.rec.every = every;
    m.run.rec.what = every ? what : 0;
    return SGPR_OK;
}

// How many frames of the last sgpr_md_run stand (0: it recorded nothing).
extern "C" int sgpr_md_frame_count(sgpr_model *h, int *count)
{
    if (!h || !count) return fail(SGPR_E_INVALID, "sgpr_md_frame_count: bad arguments");
    if (!h->md.active) return fail(SGPR_E_INVALID, "sgpr_md_frame_count: call sgpr_md_begin first");
    *count = h->md.run.rec.call_every ? h->md.run.rec.call_count : 0;
    return SGPR_OK;
}

// Frames first ... first + count - 1 of the last call's record (valid until the next sgpr_md_run, like sgpr_md_cells): index[r]
// the trajectory index, positions[count][N][3], velocities_pre[count][N][3], packed[count][4N + 11]; any of them NULL.  One
// device-to-host copy per array: nothing is un-permuted on the host.
extern "C" int sgpr_md_frames(sgpr_model *h, int first, int count, int64_t *index, double *positions, double *velocities_pre, double *packed)
{
    if (!h || first < 0 || count <= 0) return fail(SGPR_E_INVALID, "sgpr_md_frames: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_frames: call sgpr_md_begin first");
    const int have = m.run.rec.call_every ? m.run.rec.call_count : 0;
    if ((long long)first + count > have)
        return fail(SGPR_E_INVALID, "sgpr_md_frames: frames %d ... %lld asked for, the last sgpr_md_run recorded %d", first, (long long)first + count - 1, have);
    if ((velocities_pre && !(m.run.rec.call_what & 1)) || (packed && !(m.run.rec.call_what & 2)))
        return fail(SGPR_E_INVALID, "sgpr_md_frames: %s not recorded (sgpr_md_record's `what`)", velocities_pre && !(m.run.rec.call_what & 1) ? "velocities were" : "results were");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N3 = (size_t)3 * m.run.N, plen = (size_t)sgpr_packed_len(m.run.N);
    if (index) {
        const long long ev = m.run.rec.call_every, n0 = (m.run.rec.call_t0 + ev - 1) / ev * ev;
        for (int r = 0; r < count; r++) index[r] = n0 + ((long long)first + r) * ev;
    }
    if (positions) HIPCHK(hipMemcpy(positions, m.rec.x.p + N3 * first, sizeof(double) * N3 * count, hipMemcpyDeviceToHost));
    if (velocities_pre) HIPCHK(hipMemcpy(velocities_pre, m.rec.v.p + N3 * first, sizeof(double) * N3 * count, hipMemcpyDeviceToHost));
    if (packed) HIPCHK(hipMemcpy(packed, m.rec.p.p + plen * first, sizeof(double) * plen * count, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// Mean-square displacements of the run (md_msd.inc has the definition; workloads.MsdBlocks is the host twin): every >= 1 —
// configuration n with n % every == 0 is sample n / every, and behind its evaluation two launches update a table in device
// memory: per level l < levels (lag 2^l samples, one origin, windows that do not overlap) and species of the model's table the
// sums of msd, msd^2, smd, smd^2 and the number of windows.  com: displacements relative to the frame's centre of mass.  After
// sgpr_md_begin (and _fix, _thermostat, _filter, _meta, _record), before the first sgpr_md_run; every = 0 detaches and frees.  The attach
// zeroes the table.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, beside a mask, the filter, a bias
// and the frame record; a barostat, a committee, a relaxation, a band, a polymer and several ranks: SGPR_E_UNSUPPORTED, from
// here and from their attach functions.
extern "C" int sgpr_md_msd(sgpr_model *h, int every, int levels, int com)
{
    const MdAcc &acc = MD_ACC[MD_MSD];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.msd = MdRun::Msd(); return md_release(h, m.msd); }   // (a detach gives the memory back)
    if (every < 0 || levels < 1 || levels > MSD_MAXL || (com != 0 && com != 1))
        return fail(SGPR_E_INVALID, "sgpr_md_msd: every >= 0, 1 <= levels <= %d, com = 0 or 1", MSD_MAXL);
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (const int rm = md_acc_modes(h, acc)) return rm;
    const int N = m.run.N, S = h->S;
    if (sizeof(double) * (size_t)levels * S * MSD_PART > 65536)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_msd: %d levels of %d species: the sums of a sample must fit 64 KiB of LDS", levels, S);
    MdSpecies sp;   // the chunks | a species' chunks | its atoms
    if (const int rs = md_species_chunks(h, acc.fn, MSD_CHUNK, false, sp)) return rs;
    std::vector<int> &tab = sp.tab;
    const int nch = sp.nch;
    tab.insert(tab.end(), sp.coff.begin(), sp.coff.end());
    tab.insert(tab.end(), sp.nz.begin(), sp.nz.end());
    double mtot = 0.0;
    for (int i = 0; i < N; i++) mtot += m.run.mass_sorted[i];
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (m.msd.origin.alloc((size_t)levels * 3 * N) || m.msd.part.alloc((size_t)levels * nch * MSD_PART) || m.msd.table.alloc((size_t)levels * S * 4) ||
        m.msd.ctl.alloc((size_t)1 + levels) || m.msd.tab.alloc(tab.size(), false))
        return fail(SGPR_E_NODEVICE, "sgpr_md_msd: device allocation failed");
    HIPCHK(hipMemcpy(m.msd.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    MdRun::Msd &a = m.run.msd;
    a.every = every; a.levels = levels; a.com = com; a.nch = nch; a.S = S; a.mtot = mtot;
    return SGPR_OK;
}

// The table as it stands (between two calls of a run; the stream is synchronised): table [levels][S][4] the sums of msd, msd^2,
// smd, smd^2 per level and species of the model's table, counts [levels] the windows of a level, info [2] = samples taken,
// next_due (the configuration the table waits for).  Any pointer may be NULL.
extern "C" int sgpr_md_msd_read(sgpr_model *h, double *table, int64_t *counts, int64_t *info)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_msd_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.msd.every) return fail(SGPR_E_INVALID, "sgpr_md_msd_read: call sgpr_md_begin and sgpr_md_msd first");
    const MdRun::Msd &a = m.run.msd;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<long long> ctl((size_t)1 + a.levels);
    HIPCHK(hipMemcpy(ctl.data(), m.msd.ctl.p, sizeof(long long) * ctl.size(), hipMemcpyDeviceToHost));
    if (table) HIPCHK(hipMemcpy(table, m.msd.table.p, sizeof(double) * (size_t)a.levels * a.S * 4, hipMemcpyDeviceToHost));
    if (counts) for (int l = 0; l < a.levels; l++) counts[l] = ctl[1 + l];
    if (info) { info[0] = ctl[0] / a.every; info[1] = ctl[0]; }
    return SGPR_OK;
}

// The cell of the pair sweep, on the host at the attach: the inverse by the cofactor formula of nl_make_grid (restated in
// workloads.RdfCounts, operation for operation), the volume |det|, the heights V / |cross| and the image block
// R_k = floor(rmax / height_k + 1/2) along the periodic directions.  false: no volume.
static bool md_rdf_geometry(const double *cell, const int32_t *pbc, double rmax, RdfGeom &g, double &volume, double *height)
{
#pragma clang fp contract(off)
    const double *p = cell, *q = cell + 3, *r = cell + 6;
    const double dt = p[0] * (q[1] * r[2] - q[2] * r[1]) - p[1] * (q[0] * r[2] - q[2] * r[0]) + p[2] * (q[0] * r[1] - q[1] * r[0]);
    if (!(fabs(dt) > 1e-12)) return false;
    const double bc[3] = {q[1] * r[2] - q[2] * r[1], q[2] * r[0] - q[0] * r[2], q[0] * r[1] - q[1] * r[0]};
    const double ca[3] = {r[1] * p[2] - r[2] * p[1], r[2] * p[0] - r[0] * p[2], r[0] * p[1] - r[1] * p[0]};
    const double ab[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
    for (int k = 0; k < 3; k++) {
        g.inv[3 * k + 0] = bc[k] / dt;
        g.inv[3 * k + 1] = ca[k] / dt;
        g.inv[3 * k + 2] = ab[k] / dt;
    }
    for (int k = 0; k < 9; k++) g.h[k] = cell[k];
    volume = fabs(dt);
    height[0] = volume / sqrt((bc[0] * bc[0] + bc[1] * bc[1]) + bc[2] * bc[2]);
    height[1] = volume / sqrt((ca[0] * ca[0] + ca[1] * ca[1]) + ca[2] * ca[2]);
    height[2] = volume / sqrt((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]);
    for (int k = 0; k < 3; k++) {
        g.pbc[k] = pbc[k] ? 1 : 0;
        const double f = floor(rmax / height[k] + 0.5);
        g.R[k] = pbc[k] ? (f > 1e6 ? 1000000 : (int)f) : 0;
    }
    return true;
}

// Radial distribution functions of the run (md_rdf.inc has the definition; workloads.RdfCounts is the host twin): every >= 1 —
// behind the evaluation of configuration n with n % every == 0 two launches add the configuration's pair distances in
// [rmin, rmax) to a table of integers in device memory, `bins` bins per pair of species of the model's table, periodic images
// and self-images included (rmax may exceed the model's cutoff and half the cell: up to two images either way per direction).
// After sgpr_md_begin (and _fix, _thermostat, _filter, _meta, _record, _msd), before the first sgpr_md_run; every = 0 detaches.
// The attach zeroes the table.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, beside a mask, the
// filter, a bias, the frame record and sgpr_md_msd (each keeps its own next_due); a barostat, a committee, a relaxation, a
// band, a polymer and several ranks: SGPR_E_UNSUPPORTED, from here and from their attach functions.
extern "C" int sgpr_md_rdf(sgpr_model *h, int every, double rmin, double rmax, int bins)
{
    const MdAcc &acc = MD_ACC[MD_RDF];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.rdf = MdRun::Rdf(); return md_release(h, m.rdf); }
    if (every < 0 || bins < 1 || bins > RDF_MAXBINS || !(rmin >= 0.0) || !(rmin < rmax) || !(rmax < 1e300))
        return fail(SGPR_E_INVALID, "sgpr_md_rdf: every >= 0, 1 <= bins <= %d, 0 <= rmin < rmax", RDF_MAXBINS);
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (const int rm = md_acc_modes(h, acc)) return rm;
    const int S = h->S;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    double cell[9], height[3], volume = 0.0;
    HIPCHK(hipMemcpy(cell, m.cell.p, sizeof(double) * 9, hipMemcpyDeviceToHost));
    RdfGeom g = {};
    if (!md_rdf_geometry(cell, m.run.pbc, rmax, g, volume, height)) return fail(SGPR_E_INVALID, "sgpr_md_rdf: the cell has no volume; densities need one");
    for (int k = 0; k < 3; k++)
        if (g.R[k] > RDF_MAXR)
            return fail(SGPR_E_UNSUPPORTED, "sgpr_md_rdf: rmax = %g against the cell height %g along direction %d needs images %d cells away; at most %d (125 shifts)",
                        rmax, height[k], k, g.R[k], RDF_MAXR);
    g.rmin = rmin; g.rmax = rmax; g.bins = bins;
    MdSpecies sp;   // the tile pairs I <= J | a species' atoms
    if (const int rs = md_species_chunks(h, acc.fn, 0, false, sp)) return rs;
    std::vector<int> &tab = sp.tab;
    const int npairs = md_tile_pairs(sp.nz, sp.first, false, tab);
    tab.insert(tab.end(), sp.nz.begin(), sp.nz.end());
    if (m.rdf.table.alloc((size_t)S * S * bins) || m.rdf.ctl.alloc(2) || m.rdf.tab.alloc(tab.size(), false))
        return fail(SGPR_E_NODEVICE, "sgpr_md_rdf: device allocation failed");
    HIPCHK(hipMemcpy(m.rdf.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    MdRun::Rdf &a = m.run.rdf;
    // (workgroups for every SIMD of the chip: a tile pair of a small frame is cut along J into up to 8 parts of 16 atoms or more)
    a.split = std::max(1, std::min(RDF_SPLIT_MAX, RDF_WORKGROUPS / std::max(1, npairs)));
    a.every = every; a.npairs = npairs; a.S = S; a.images = g.R[0] || g.R[1] || g.R[2]; a.g = g; a.volume = volume; a.nz = sp.nz;
    return SGPR_OK;
}

// The table as it stands (between two calls of a run; the stream is synchronised): hist [S][S][bins] the counts per ordered pair
// of species slots, symmetric and filled out; info [4 + S] = samples taken, next_due (the configuration the table waits for),
// bins, S, and the atoms of every species in the frame; geom [3] = the volume |det cell|, rmin, rmax.  Any pointer may be NULL.
extern "C" int sgpr_md_rdf_read(sgpr_model *h, uint64_t *hist, int64_t *info, double *geom)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_rdf_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.rdf.every) return fail(SGPR_E_INVALID, "sgpr_md_rdf_read: call sgpr_md_begin and sgpr_md_rdf first");
    const MdRun::Rdf &a = m.run.rdf;
    const int S = a.S, bins = a.g.bins;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hist) {
        HIPCHK(hipMemcpy(hist, m.rdf.table.p, sizeof(uint64_t) * (size_t)S * S * bins, hipMemcpyDeviceToHost));
        for (int p = 0; p < S; p++)
            for (int q = 0; q < p; q++)
                for (int k = 0; k < bins; k++) hist[((size_t)p * S + q) * bins + k] = hist[((size_t)q * S + p) * bins + k];
    }
    if (info) {
        long long ctl[2];
        HIPCHK(hipMemcpy(ctl, m.rdf.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
        info[0] = ctl[1]; info[1] = ctl[0]; info[2] = bins; info[3] = S;
        for (int z = 0; z < S; z++) info[4 + z] = a.nz[z];
    }
    if (geom) { geom[0] = a.volume; geom[1] = a.g.rmin; geom[2] = a.g.rmax; }
    return SGPR_OK;
}

// Velocity autocorrelations of the run (md_vacf.inc has the definition; workloads.VacfRing is the host twin): every >= 1 —
// configuration n with n % every == 0 is sample n / every; behind its evaluation its observer's velocity is stored in a ring of
// lags + 1 slots and the sample before it is correlated with its origins o = s - k, k < lags, o % origin_every == 0: per species
// of the model's table the tracer sums tr [lags][S], the collective block col [lags][S][S], count [lags].  com: velocities relative
// to the frame's centre of mass.  After sgpr_md_begin (and _fix, _thermostat, _record, _msd, _rdf), before the first sgpr_md_run;
// every = 0 detaches and frees.  The attach zeroes the tables.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one
// rank, beside a mask, the frame record, sgpr_md_msd and sgpr_md_rdf (each keeps its own next_due); a barostat, a committee, a
// relaxation, a band, a polymer, several ranks, the filter and a bias (there the closing kick uses a force other than the packed
// one): SGPR_E_UNSUPPORTED, from here and from their attach functions.  Limits: lags <= VACF_MAXLAGS, the ring
// (lags + 1) 24 N bytes <= VACF_MAXBYTES.
extern "C" int sgpr_md_vacf(sgpr_model *h, int every, int lags, int origin_every, int com)
{
    const MdAcc &acc = MD_ACC[MD_VACF];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.vacf = MdRun::Vacf(); return md_release(h, m.vacf); }
    if (every < 0 || lags < 1 || origin_every < 1 || (com != 0 && com != 1))
        return fail(SGPR_E_INVALID, "sgpr_md_vacf: every >= 0, lags >= 1, origin_every >= 1, com = 0 or 1");
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (const int rm = md_acc_modes(h, acc)) return rm;
    if (m.run.filter.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_vacf: the run has a filter (sgpr_md_filter): its closing kick uses the filtered force, not the packed one the sample takes");
    if (m.run.meta.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_vacf: the run has a bias (sgpr_md_meta): its closing kick uses the biased force, not the packed one the sample takes");
    const int N = m.run.N, S = h->S;
    if (lags > VACF_MAXLAGS || (unsigned long long)(lags + 1) * 24ull * (unsigned long long)N > VACF_MAXBYTES)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_vacf: %d lags of %d atoms: at most %d lags and a ring of (lags + 1) 24 N = %llu bytes",
                    lags, N, VACF_MAXLAGS, (unsigned long long)VACF_MAXBYTES);
    MdSpecies sp;   // the chunks | a species' chunks | its atoms
    if (const int rs = md_species_chunks(h, acc.fn, VACF_CHUNK, false, sp)) return rs;
    std::vector<int> &tab = sp.tab;
    const int nch = sp.nch;
    tab.insert(tab.end(), sp.coff.begin(), sp.coff.end());
    tab.insert(tab.end(), sp.nz.begin(), sp.nz.end());
    double mtot = 0.0;
    for (int i = 0; i < N; i++) mtot += m.run.mass_sorted[i];
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t slots = (size_t)lags + 1;
    // (ring slots are stored before they are read: only the tables and the control words start from zero)
    if (m.vacf.ring.alloc(slots * 3 * N, false) || m.vacf.vpart.alloc(slots * nch * 6, false) || m.vacf.part.alloc((size_t)lags * nch, false) ||
        m.vacf.jring.alloc(slots * S * 3, false) || m.vacf.cring.alloc(slots * 3, false) || m.vacf.tr.alloc((size_t)lags * S) ||
        m.vacf.col.alloc((size_t)lags * S * S) || m.vacf.ctl.alloc((size_t)2 + lags) || m.vacf.tab.alloc(tab.size(), false))
        return fail(SGPR_E_NODEVICE, "sgpr_md_vacf: device allocation failed");
    HIPCHK(hipMemcpy(m.vacf.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    MdRun::Vacf &a = m.run.vacf;
    a.every = every; a.lags = lags; a.origin_every = origin_every; a.com = com; a.nch = nch; a.S = S; a.mtot = mtot; a.nz = sp.nz;
    return SGPR_OK;
}

// The tables as they stand (between two calls of a run; the stream is synchronised): tracer [lags][S], collective [lags][S][S],
// counts [lags], info [3 + S] = samples correlated, pending (0 / 1: a stored sample waits for the next one), next_due (the
// configuration the table waits for), and the atoms of every species in the frame.  Any pointer may be NULL.
extern "C" int sgpr_md_vacf_read(sgpr_model *h, double *tracer, double *collective, int64_t *counts, int64_t *info)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_vacf_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.vacf.every) return fail(SGPR_E_INVALID, "sgpr_md_vacf_read: call sgpr_md_begin and sgpr_md_vacf first");
    const MdRun::Vacf &a = m.run.vacf;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<long long> ctl((size_t)2 + a.lags);
    HIPCHK(hipMemcpy(ctl.data(), m.vacf.ctl.p, sizeof(long long) * ctl.size(), hipMemcpyDeviceToHost));
    if (tracer) HIPCHK(hipMemcpy(tracer, m.vacf.tr.p, sizeof(double) * (size_t)a.lags * a.S, hipMemcpyDeviceToHost));
    if (collective) HIPCHK(hipMemcpy(collective, m.vacf.col.p, sizeof(double) * (size_t)a.lags * a.S * a.S, hipMemcpyDeviceToHost));
    if (counts) for (int k = 0; k < a.lags; k++) counts[k] = ctl[2 + k];
    if (info) {
        info[0] = ctl[1]; info[1] = ctl[0] > 0 ? 1 : 0; info[2] = ctl[0];
        for (int z = 0; z < a.S; z++) info[3 + z] = a.nz[z];
    }
    return SGPR_OK;
}

// Van Hove functions of the run (md_vanhove.inc has the definition; workloads.VanHoveCounts is the host twin): every >= 1 —
// configuration n with n % every == 0 is sample n / every, levels and origins as sgpr_md_msd's; behind a sampled evaluation at
// most three launches add, per due level, every atom's displacement to a histogram over (r < rmax, theta, phi) per species of
// the model's table (rbins x tbins x pbins; beyond rmax: `over`) and, with dbins > 0, every distance r < dmax between an origin
// and a present position, periodic images included, to dbins bins per ORDERED pair of species.  All entries are integers.
// After sgpr_md_begin (and _fix, _thermostat, _filter, _meta, _record, _msd, _rdf, _vacf), before the first sgpr_md_run; every =
// 0 detaches and frees.  The attach zeroes the tables and sets the angular edges with cos and sin of this library;
// sgpr_md_vanhove_edges replaces them by the caller's doubles.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one
// rank, beside a mask, the filter, a bias, the frame record and the other accumulators (each keeps its own next_due); a
// barostat, a committee, a relaxation, a band, a polymer and several ranks: SGPR_E_UNSUPPORTED, from here and from their attach
// functions.
extern "C" int sgpr_md_vanhove(sgpr_model *h, int every, int levels, double rmax, int rbins, int tbins, int pbins, double dmax, int dbins)
{
    const MdAcc &acc = MD_ACC[MD_VH];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.vh = MdRun::VanHove(); return md_release(h, m.vh); }
    if (every < 0 || levels < 1 || levels > MSD_MAXL) return fail(SGPR_E_INVALID, "sgpr_md_vanhove: every >= 0, 1 <= levels <= %d", MSD_MAXL);
    if (rbins < 1 || rbins > VH_MAXRBINS || !(rmax > 0.0) || !(rmax < 1e300))
        return fail(SGPR_E_INVALID, "sgpr_md_vanhove: rmax > 0, 1 <= rbins <= %d (rbins = %d)", VH_MAXRBINS, rbins);
    if (tbins < 1 || tbins > VH_MAXABINS || pbins < 1 || pbins > VH_MAXABINS)
        return fail(SGPR_E_INVALID, "sgpr_md_vanhove: 1 <= tbins, pbins <= %d (tbins = %d, pbins = %d)", VH_MAXABINS, tbins, pbins);
    if (dbins < 0 || dbins > RDF_MAXBINS || (dbins > 0 && (!(dmax > 0.0) || !(dmax < 1e300))))
        return fail(SGPR_E_INVALID, "sgpr_md_vanhove: 0 <= dbins <= %d (dbins = %d), dmax > 0 with dbins > 0", RDF_MAXBINS, dbins);
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (const int rm = md_acc_modes(h, acc)) return rm;
    const int N = m.run.N, S = h->S;
    const size_t zstride = (size_t)rbins * tbins * pbins;
    if ((unsigned long long)levels * S * zstride * 8ull > (1ull << 30))
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_vanhove: a self table of %d levels x %d species x %d x %d x %d bins is %llu bytes; at most 1 GiB",
                    levels, S, rbins, tbins, pbins, (unsigned long long)levels * S * zstride * 8ull);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    double cell[9], height[3] = {0.0, 0.0, 0.0}, volume = 0.0;
    HIPCHK(hipMemcpy(cell, m.cell.p, sizeof(double) * 9, hipMemcpyDeviceToHost));
    RdfGeom g = {};
    const bool has_volume = md_rdf_geometry(cell, m.run.pbc, dbins ? dmax : 0.0, g, volume, height);
    if (dbins) {
        if (!has_volume) return fail(SGPR_E_INVALID, "sgpr_md_vanhove: the cell has no volume; the distinct part needs one");
        for (int k = 0; k < 3; k++)
            if (g.R[k] > RDF_MAXR)
                return fail(SGPR_E_UNSUPPORTED, "sgpr_md_vanhove: dmax = %g against the cell height %g along direction %d needs images %d cells away; at most %d (125 shifts)",
                            dmax, height[k], k, g.R[k], RDF_MAXR);
    }
    g.rmin = 0.0; g.rmax = dbins ? dmax : 0.0; g.bins = dbins;
    // the chunks of the self part and the tiles of the distinct part: runs of consecutive sorted atoms of one species (the sort is
    // by species in table order); every ordered pair of tiles
    MdSpecies sp;
    if (const int rs = md_species_chunks(h, acc.fn, MSD_CHUNK, true, sp)) return rs;
    static_assert(VH_CHUNK == 3, "a chunk record of the self part: first atom, atoms, species");
    std::vector<int> &tab = sp.tab;
    const int nch = sp.nch, npairs = dbins ? md_tile_pairs(sp.nz, sp.first, true, tab) : 0;
    tab.insert(tab.end(), sp.nz.begin(), sp.nz.end());
    std::vector<double> edges((size_t)tbins + 2 * pbins);
    for (int k = 0; k < tbins; k++) edges[k] = cos((double)k * M_PI / (double)tbins);
    for (int k = 0; k < pbins; k++) {
        const double f = -M_PI + 2.0 * M_PI * (double)k / (double)pbins;
        edges[tbins + k] = cos(f); edges[tbins + pbins + k] = sin(f);
    }
    if (m.vh.origin.alloc((size_t)levels * 3 * N, false) || m.vh.edges.alloc(edges.size(), false) || m.vh.hs.alloc((size_t)levels * S * zstride) ||
        m.vh.over.alloc((size_t)levels * S) || m.vh.hd.alloc((size_t)levels * S * S * dbins) || m.vh.ctl.alloc((size_t)VH_CTL + levels) ||
        m.vh.tab.alloc(tab.size(), false)) {
        m.vh = MdState::VanHoveBufs();
        m.run.vh = MdRun::VanHove();   // (an earlier attach's settings go with its buffers: the run launches nothing on them)
        return fail(SGPR_E_NODEVICE, "sgpr_md_vanhove: device allocation failed");
    }
    HIPCHK(hipMemcpy(m.vh.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.vh.edges.p, edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice));
    MdRun::VanHove &a = m.run.vh;
    a = MdRun::VanHove();
    a.split = std::max(1, std::min(RDF_SPLIT_MAX, RDF_WORKGROUPS / std::max(1, npairs)));
    a.every = every; a.levels = levels; a.rbins = rbins; a.tbins = tbins; a.pbins = pbins; a.dbins = dbins; a.nch = nch; a.npairs = npairs; a.S = S;
    a.images = g.R[0] || g.R[1] || g.R[2]; a.g = g; a.rmax = rmax; a.dmax = dbins ? dmax : 0.0; a.volume = has_volume ? volume : 0.0; a.nz = sp.nz;
    return SGPR_OK;
}

// The angular edges of the self part as the caller made them: ct [tbins] = cos(k pi / tbins), cu, su [pbins] = cos, sin of
// -pi + 2 pi k / pbins (entry 0 of each is never compared).  A host twin that compares with the same doubles gives the same
// counts whatever the two libraries' cos and sin do to a last bit.  After sgpr_md_vanhove, before the first sgpr_md_run.
extern "C" int sgpr_md_vanhove_edges(sgpr_model *h, const double *ct, const double *cu, const double *su)
{
    if (!h || !ct || !cu || !su) return fail(SGPR_E_INVALID, "sgpr_md_vanhove_edges: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.vh.every) return fail(SGPR_E_INVALID, "sgpr_md_vanhove_edges: call sgpr_md_begin and sgpr_md_vanhove first");
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_vanhove_edges: the run has started");
    const MdRun::VanHove &a = m.run.vh;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(m.vh.edges.p, ct, sizeof(double) * a.tbins, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.vh.edges.p + a.tbins, cu, sizeof(double) * a.pbins, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.vh.edges.p + a.tbins + a.pbins, su, sizeof(double) * a.pbins, hipMemcpyHostToDevice));
    return SGPR_OK;
}

// The tables as they stand (between two calls of a run; the stream is synchronised): self_hist [levels][S][rbins][tbins][pbins],
// over [levels][S], distinct_hist [levels][S][S][dbins] (origin's species first), counts [levels] the windows of a level, info
// [8 + S] = samples taken, next_due (the configuration the tables wait for), levels, S, rbins, tbins, pbins, dbins, and the atoms
// of every species in the frame; geom [3] = the volume |det cell| (0: none), rmax, dmax.  Any pointer may be NULL.
extern "C" int sgpr_md_vanhove_read(sgpr_model *h, uint64_t *self_hist, uint64_t *over, uint64_t *distinct_hist, int64_t *counts, int64_t *info,
                                    double *geom)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_vanhove_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.vh.every) return fail(SGPR_E_INVALID, "sgpr_md_vanhove_read: call sgpr_md_begin and sgpr_md_vanhove first");
    const MdRun::VanHove &a = m.run.vh;
    const size_t LS = (size_t)a.levels * a.S;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<long long> ctl((size_t)VH_CTL + a.levels);
    HIPCHK(hipMemcpy(ctl.data(), m.vh.ctl.p, sizeof(long long) * ctl.size(), hipMemcpyDeviceToHost));
    if (self_hist) HIPCHK(hipMemcpy(self_hist, m.vh.hs.p, sizeof(uint64_t) * LS * a.rbins * a.tbins * a.pbins, hipMemcpyDeviceToHost));
    if (over) HIPCHK(hipMemcpy(over, m.vh.over.p, sizeof(uint64_t) * LS, hipMemcpyDeviceToHost));
    if (distinct_hist && a.dbins) HIPCHK(hipMemcpy(distinct_hist, m.vh.hd.p, sizeof(uint64_t) * LS * a.S * a.dbins, hipMemcpyDeviceToHost));
    if (counts) for (int l = 0; l < a.levels; l++) counts[l] = ctl[VH_CTL + l];
    if (info) {
        info[0] = ctl[1]; info[1] = ctl[0]; info[2] = a.levels; info[3] = a.S; info[4] = a.rbins; info[5] = a.tbins; info[6] = a.pbins; info[7] = a.dbins;
        for (int z = 0; z < a.S; z++) info[8 + z] = a.nz[z];
    }
    if (geom) { geom[0] = a.volume; geom[1] = a.rmax; geom[2] = a.dmax; }
    return SGPR_OK;
}

// Bond-angle and coordination distributions of the run (md_adf.inc has the definition; workloads.AdfCounts is the host twin):
// every >= 1 — behind the evaluation of configuration n with n % every == 0 two launches count, per centre, the angles between the
// pairs of its neighbours within cut[a][b] and its neighbours per species, from the neighbour list the step has just built.
// cut: [S][S] over the species slots of the model's table, symmetric, 0 = the pair never bonds, every entry <= rc; ct: [bins] the
// caller's cos(e pi / bins) (entry 0 is never compared; they must not increase).  After sgpr_md_begin (and _fix, _thermostat,
// _filter, _meta, _record, _msd, _rdf, _vacf, _vanhove), before the first sgpr_md_run; every = 0 detaches and frees.  The attach
// zeroes the tables.  Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, beside a mask, the filter, a bias,
// the frame record and the other accumulators (each keeps its own next_due); a barostat, a committee, a relaxation, a band, a
// polymer and several ranks: SGPR_E_UNSUPPORTED, from here and from their attach functions.
extern "C" int sgpr_md_adf(sgpr_model *h, int every, int bins, const double *cut, const double *ct)
{
    const MdAcc &acc = MD_ACC[MD_ADF];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.adf = MdRun::Adf(); return md_release(h, m.adf); }
    if (every < 0 || bins < 1 || bins > ADF_MAXBINS || !cut || !ct)
        return fail(SGPR_E_INVALID, "sgpr_md_adf: every >= 0, 1 <= bins <= %d, a cutoff table and an edge table", ADF_MAXBINS);
    const int S = h->S;
    double cmax = 0.0;
    for (int a = 0; a < S; a++)
        for (int b = 0; b < S; b++) {
            const double c = cut[a * S + b];
            if (!(c >= 0.0) || !(c < 1e300) || c != cut[b * S + a])
                return fail(SGPR_E_INVALID, "sgpr_md_adf: the cutoff table must be symmetric and >= 0 (slots %d, %d: %g against %g)", a, b, c, cut[b * S + a]);
            cmax = std::max(cmax, c);
        }
    if (!(cmax > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_adf: every cutoff is 0: no pair bonds");
    for (int e = 0; e < bins; e++)
        if (!(fabs(ct[e]) <= 1.0) || (e > 0 && ct[e] > ct[e - 1]))
            return fail(SGPR_E_INVALID, "sgpr_md_adf: the edges ct[e] = cos(e pi / bins) lie in [-1, 1] and do not increase (entry %d)", e);
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (cmax > h->rc)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_adf: a bond cutoff of %g lies beyond the model's cutoff %g; the step's neighbour list holds no further neighbours", cmax, h->rc);
    if (const int rm = md_acc_modes(h, acc)) return rm;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    MdSpecies sp;   // the chunks of centres | a species' atoms
    if (const int rs = md_species_chunks(h, acc.fn, ADF_CHUNK, true, sp)) return rs;
    std::vector<int> &tab = sp.tab;
    const int nch = sp.nch;
    tab.insert(tab.end(), sp.nz.begin(), sp.nz.end());
    std::vector<double> par(cut, cut + (size_t)S * S);
    par.insert(par.end(), ct, ct + bins);
    if (m.adf.angles.alloc((size_t)S * S * S * bins) || m.adf.coord.alloc((size_t)S * S * ADF_MAXCOORD) || m.adf.par.alloc(par.size(), false) ||
        m.adf.ctl.alloc(2) || m.adf.tab.alloc(tab.size(), false)) {
        m.adf = MdState::AdfBufs();
        m.run.adf = MdRun::Adf();   // (an earlier attach's settings go with its buffers: the run launches nothing on them)
        return fail(SGPR_E_NODEVICE, "sgpr_md_adf: device allocation failed");
    }
    HIPCHK(hipMemcpy(m.adf.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.adf.par.p, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice));
    MdRun::Adf &a = m.run.adf;
    a = MdRun::Adf();
    a.every = every; a.bins = bins; a.nch = nch; a.S = S; a.nz = sp.nz;
    a.lds = (long long)(S * (S + 1) / 2) * bins <= ADF_LDS_COUNTERS;
    return SGPR_OK;
}

// The tables as they stand (between two calls of a run; the stream is synchronised): angles [S][S][S][bins] the counts per (centre,
// end, end) of species slots, symmetric in the ends and filled out; coord [S][S][64] per (centre, neighbour) the centres with n
// neighbours (63: that many or more); info [4 + S] = samples taken, next_due (the configuration the tables wait for), bins, S,
// and the atoms of every species in the frame.  Any pointer may be NULL.
extern "C" int sgpr_md_adf_read(sgpr_model *h, uint64_t *angles, uint64_t *coord, int64_t *info)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_adf_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.adf.every) return fail(SGPR_E_INVALID, "sgpr_md_adf_read: call sgpr_md_begin and sgpr_md_adf first");
    const MdRun::Adf &a = m.run.adf;
    const int S = a.S, bins = a.bins;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (angles) {
        HIPCHK(hipMemcpy(angles, m.adf.angles.p, sizeof(uint64_t) * (size_t)S * S * S * bins, hipMemcpyDeviceToHost));
        for (int c = 0; c < S; c++)
            for (int p = 0; p < S; p++)
                for (int q = 0; q < p; q++)
                    for (int k = 0; k < bins; k++) angles[(((size_t)c * S + p) * S + q) * bins + k] = angles[(((size_t)c * S + q) * S + p) * bins + k];
    }
    if (coord) HIPCHK(hipMemcpy(coord, m.adf.coord.p, sizeof(uint64_t) * (size_t)S * S * ADF_MAXCOORD, hipMemcpyDeviceToHost));
    if (info) {
        long long ctl[2];
        HIPCHK(hipMemcpy(ctl, m.adf.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
        info[0] = ctl[1]; info[1] = ctl[0]; info[2] = bins; info[3] = S;
        for (int z = 0; z < S; z++) info[4 + z] = a.nz[z];
    }
    return SGPR_OK;
}

// Partial structure factors and coherent intermediate scattering functions of the run (md_sq.inc has the definition and the
// accuracy bound the device is held to; workloads.SqRing is the host twin): every >= 1 — configuration n with n % every == 0 is
// sample n / every; behind its evaluation three launches form, per species of the model's table and wave vector q_j = 2 pi hkl_j
// inv(cell)^T (hkl [nq][3], one of each +- pair), the density rho_z(q_j), keep it in a ring of `lags` slots, and add
// Re(rho_a(s) conj rho_b(o)) to f [lags][nq][S][S] for every lag k < lags whose origin o = s - k >= 0 has o % origin_every == 0,
// rho to mean [nq][S] and 1 to count [k] and to samples.  After sgpr_md_begin (and _fix, _thermostat, _filter, _meta, _record
// and the other accumulators), before the first sgpr_md_run; every = 0 detaches and frees.  The attach zeroes the tables.
// Langevin, velocity Verlet and Nose-Hoover at constant cell on one rank, beside a mask, the filter, a bias, the frame record
// and the other accumulators (each keeps its own next_due); a barostat, a committee, a relaxation, a band, a polymer and several
// ranks: SGPR_E_UNSUPPORTED, from here and from their attach functions.  Limits: nq <= SQ_MAXQ, |index| <= SQ_MAXH, lags <=
// SQ_MAXLAGS, f and the ring together lags nq S (8 S + 16) bytes <= SQ_MAXBYTES.
extern "C" int sgpr_md_sq(sgpr_model *h, int every, int nq, const int32_t *hkl, int lags, int origin_every)
{
    const MdAcc &acc = MD_ACC[MD_SQ];
    if (const int rr = md_acc_run(h, acc)) return rr;
    MdState &m = h->md;
    if (every == 0) { m.run.sq = MdRun::Sq(); return md_release(h, m.sq); }
    if (every < 0 || nq < 1 || nq > SQ_MAXQ || !hkl || lags < 1 || lags > SQ_MAXLAGS || origin_every < 1)
        return fail(SGPR_E_INVALID, "sgpr_md_sq: every >= 0, 1 <= nq <= %d wave vectors hkl[nq][3], 1 <= lags <= %d, origin_every >= 1", SQ_MAXQ, SQ_MAXLAGS);
    int hmax = 0;
    for (int j = 0; j < nq; j++) {
        const int32_t *v = hkl + 3 * (size_t)j;
        if (!v[0] && !v[1] && !v[2]) return fail(SGPR_E_INVALID, "sgpr_md_sq: wave vector %d is (0, 0, 0): rho(0) is the number of atoms", j);
        for (int k = 0; k < 3; k++) {
            if (v[k] > SQ_MAXH || v[k] < -SQ_MAXH)
                return fail(SGPR_E_INVALID, "sgpr_md_sq: wave vector %d has the index %d along direction %d; at most %d either way", j, (int)v[k], k, SQ_MAXH);
            if (v[k] && !m.run.pbc[k])
                return fail(SGPR_E_INVALID, "sgpr_md_sq: wave vector %d has the index %d along direction %d, which is not periodic: no reciprocal lattice there",
                            j, (int)v[k], k);
            hmax = std::max(hmax, std::abs((int)v[k]));
        }
    }
    if (const int ru = md_acc_unstarted(h, acc)) return ru;
    if (const int rm = md_acc_modes(h, acc)) return rm;
    const int S = h->S;
    const unsigned long long bytes = (unsigned long long)lags * (unsigned long long)nq * (unsigned long long)S * (8ull * S + 16ull);
    if (bytes > SQ_MAXBYTES)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_sq: %d lags of %d wave vectors and %d species: f and the ring take %llu bytes; at most %llu "
                    "(fewer lags, a larger `every`, or fewer wave vectors)", lags, nq, S, bytes, (unsigned long long)SQ_MAXBYTES);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    double cell[9], height[3], volume = 0.0;
    HIPCHK(hipMemcpy(cell, m.cell.p, sizeof(double) * 9, hipMemcpyDeviceToHost));
    RdfGeom g = {};   // (the inverse of the pair sweeps: one formula for every accumulator that scales coordinates)
    if (!md_rdf_geometry(cell, m.run.pbc, 1.0, g, volume, height)) return fail(SGPR_E_INVALID, "sgpr_md_sq: the cell has no volume; a reciprocal lattice needs one");
    const bool narrow = hmax > SQ_WIDE_H;
    MdSpecies sp;   // the chunks | a species' chunks | the wave vectors
    if (const int rs = md_species_chunks(h, acc.fn, narrow ? 32 : 64, false, sp)) return rs;
    std::vector<int> &tab = sp.tab;
    const int nch = sp.nch;
    tab.insert(tab.end(), sp.coff.begin(), sp.coff.end());
    tab.insert(tab.end(), hkl, hkl + 3 * (size_t)nq);
    const size_t LQ = (size_t)lags * nq;
    // (part and ring slots are written before they are read: only the tables and the control words start from zero)
    if (m.sq.part.alloc((size_t)std::max(nch, 1) * nq * 2, false) || m.sq.ring.alloc(LQ * S * 2, false) || m.sq.mean.alloc((size_t)nq * S * 2) ||
        m.sq.f.alloc(LQ * S * S) || m.sq.inv.alloc(9, false) || m.sq.ctl.alloc((size_t)2 + lags) || m.sq.tab.alloc(tab.size(), false)) {
        m.sq = MdState::SqBufs();
        m.run.sq = MdRun::Sq();   // (an earlier attach's settings go with its buffers: the run launches nothing on them)
        return fail(SGPR_E_NODEVICE, "sgpr_md_sq: device allocation failed");
    }
    HIPCHK(hipMemcpy(m.sq.tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.sq.inv.p, g.inv, sizeof(double) * 9, hipMemcpyHostToDevice));
    MdRun::Sq &a = m.run.sq;
    a = MdRun::Sq();
    a.every = every; a.nq = nq; a.lags = lags; a.origin_every = origin_every; a.nch = nch; a.S = S; a.narrow = narrow; a.nz = sp.nz;
    return SGPR_OK;
}

// The tables as they stand (between two calls of a run; the stream is synchronised): f [lags][nq][S][S], mean [nq][S][2] (real,
// imaginary), count [lags], info [2 + S] = samples taken, next_due (the configuration the tables wait for), and the atoms of
// every species in the frame.  Any pointer may be NULL.
extern "C" int sgpr_md_sq_read(sgpr_model *h, double *f, double *mean, int64_t *count, int64_t *info)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_sq_read: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.sq.every) return fail(SGPR_E_INVALID, "sgpr_md_sq_read: call sgpr_md_begin and sgpr_md_sq first");
    const MdRun::Sq &a = m.run.sq;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<long long> ctl((size_t)2 + a.lags);
    HIPCHK(hipMemcpy(ctl.data(), m.sq.ctl.p, sizeof(long long) * ctl.size(), hipMemcpyDeviceToHost));
    if (f) HIPCHK(hipMemcpy(f, m.sq.f.p, sizeof(double) * (size_t)a.lags * a.nq * a.S * a.S, hipMemcpyDeviceToHost));
    if (mean) HIPCHK(hipMemcpy(mean, m.sq.mean.p, sizeof(double) * (size_t)a.nq * a.S * 2, hipMemcpyDeviceToHost));
    if (count) for (int k = 0; k < a.lags; k++) count[k] = ctl[2 + k];
    if (info) {
        info[0] = ctl[1]; info[1] = ctl[0];
        for (int z = 0; z < a.S; z++) info[2 + z] = a.nz[z];
    }
    return SGPR_OK;
}

// Deviates of the integrator on the device: seed != 0 makes sgpr_md_run (called with noise = NULL) draw the standard
// normal deviate of (configuration index, atom, component) from a counter-based generator; 0 switches that off.
extern "C" int sgpr_md_seed(sgpr_model *h, uint64_t seed)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_seed: bad arguments");
    h->md.seed = seed;
    return SGPR_OK;
}

// The deviates sgpr_md_run uses to move configurations [t_first, t_first + count) on, out[count][N][3] in caller atom
// order (for a host-side twin of a seeded run).
extern "C" int sgpr_md_deviates(sgpr_model *h, int64_t t_first, int count, double *out)
{
    if (!h || count <= 0 || !out) return fail(SGPR_E_INVALID, "sgpr_md_deviates: bad arguments");
    MdState &m = h->md;
    if (!m.active || m.seed == 0) return fail(SGPR_E_INVALID, "sgpr_md_deviates: call sgpr_md_begin and sgpr_md_seed first");
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> d;
    if (d.alloc((size_t)count * 3 * m.run.N, false)) return fail(SGPR_E_NODEVICE, "sgpr_md_deviates: device allocation failed");
    hipLaunchKernelGGL(md_deviates_kernel, dim3(1024), dim3(256), 0, h->stream, m.run.N, count, m.seed, (long long)t_first, d.p);
    HIPCHK(hipMemcpy(out, d.p, sizeof(double) * (size_t)count * 3 * m.run.N, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// The filter of model-update jumps for the run begun by sgpr_md_begin: the reference's default MD wraps its atoms in FilterDeltas
// (cl/md.py:76-79, ml_filter = 0.8; calculator/active.py:47-76), which keeps a running sum of the jumps `deltas` an on-the-fly
// update puts into forces and stress, shrinks it at every call and subtracts it (forces: clamped to 1 eV/A) from what the
// integrator sees.  Here, by evaluation index, once per configuration n:
//     A_f <- (A_f + dF_n) shrink,   F_seen = F_model - min(max(A_f, -1), 1)      (then a held component sees 0 as before)
//     A_s <- (A_s + dS_n) shrink,   stress_seen = stress_model - A_s              (moving cell only: nobody else asks for a stress)
// inside the step's last kernel (finalize_next_kernel<5>, <6>, <7>) and md_npt_kernel; dF_n, dS_n: what sgpr_md_filter_push added
// to the accumulators of configuration n before its evaluation.  The accumulators live in rings indexed like X and V (slot n is
// read, slot n + 1 written): the evaluation a halt discards leaves those of its configuration as they were.  What the run
// REPORTS (packed, sgpr_md_state, the frame record, the scalar rows) stays the model's own.
// After sgpr_md_begin (and sgpr_md_fix / _thermostat / _barostat), before the first sgpr_md_run.  0 < shrink < 1; f0[3N] caller
// atom order and s0[6] Voigt: the accumulators of configuration 0 (NULL: zeros).  A relaxation, a committee, several ranks:
// SGPR_E_UNSUPPORTED; sgpr_md_relax and sgpr_md_committee refuse a run that has a filter.
extern "C" int sgpr_md_filter(sgpr_model *h, double shrink, const double *f0, const double *s0)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_filter: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_filter: call sgpr_md_begin first");
    if (m.run.t != 0 || m.run.started) return fail(SGPR_E_INVALID, "sgpr_md_filter: the run has started");
    if (!(shrink > 0.0 && shrink < 1.0)) return fail(SGPR_E_INVALID, "sgpr_md_filter: 0 < shrink < 1");
    if (m.run.relax.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run is a relaxation (sgpr_md_relax), which applies no filter");
    if (m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run is a nudged elastic band (sgpr_md_neb), which applies no filter");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run is a ring polymer (sgpr_md_pimd), which integrates unfiltered forces");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run has a committee (sgpr_md_committee), which integrates unfiltered forces");
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run was begun on %d ranks; the filter runs on one", m.run.world);
    if (m.run.vacf.every) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_filter: the run accumulates velocity correlations (sgpr_md_vacf), whose closing kick uses the packed force; the filtered integrator kicks with another");
    HIPCHK(hipSetDevice(h->device));
    const int N = m.run.N;
    const size_t N3 = (size_t)3 * N;
    if (m.filter.f.alloc(4 * N3) || m.filter.s.alloc(32) || m.filter.in.alloc(N3) || m.filter.perm.alloc(N))
        return fail(SGPR_E_NODEVICE, "sgpr_md_filter: device allocation failed");
    HIPCHK(hipMemset(m.filter.f.p, 0, sizeof(double) * 4 * N3));
    HIPCHK(hipMemset(m.filter.s.p, 0, sizeof(double) * 32));
    HIPCHK(hipMemcpy(m.filter.perm.p, m.run.perm.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    if (f0) {
        std::vector<double> fs(N3);
        for (int i = 0; i < N; i++)
            for (int k = 0; k < 3; k++) fs[3 * (size_t)i + k] = f0[3 * (size_t)m.run.perm[i] + k];
        HIPCHK(hipMemcpy(m.filter.f.p, fs.data(), sizeof(double) * N3, hipMemcpyHostToDevice));
    }
    for (int k = 0; k < 6; k++) m.run.filter.s_host[k] = s0 ? s0[k] : 0.0;
    HIPCHK(hipMemcpy(m.filter.s.p, m.run.filter.s_host, sizeof(double) * 6, hipMemcpyHostToDevice));
    m.run.filter.on = true; m.run.filter.shrink = shrink;
    return SGPR_OK;
}

// caller order -> the run's sorted order, added into the accumulators of the current configuration (one thread per component;
// the six stress jumps by thread 0)
struct MdSix { double v[6]; };
__global__ void md_filter_push_kernel(int N, const int *perm, const double *dF, double *acc, MdSix dS, double *acc_s)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)3 * N) {
        const size_t i = e / 3, k = e - 3 * i;
        acc[e] = acc[e] + dF[3 * (size_t)perm[i] + k];
    }
    if (e == 0 && acc_s)
        for (int q = 0; q < 6; q++) acc_s[q] = acc_s[q] + dS.v[q];
}

// The jump of a model update, between two sgpr_md_run calls (after the halt's calculate(), whose `deltas` these are): dF[N][3]
// caller atom order (NULL: none), dS[6] Voigt (NULL: none; ignored at constant cell), added into the accumulators of the current
// configuration — the next evaluation shrinks the sum and applies it.
extern "C" int sgpr_md_filter_push(sgpr_model *h, const double *dF, const double *dS)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_filter_push: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.filter.on) return fail(SGPR_E_INVALID, "sgpr_md_filter_push: call sgpr_md_begin and sgpr_md_filter first");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    HIPCHK(hipStreamSynchronize(st));
    const int N = m.run.N;
    const size_t N3 = (size_t)3 * N;
    MdSix six = {};
    const bool ws = m.run.npt.on && dS;
    if (ws) for (int k = 0; k < 6; k++) six.v[k] = dS[k];
    if (!dF && !ws) return SGPR_OK;
    if (dF) HIPCHK(hipMemcpy(m.filter.in.p, dF, sizeof(double) * N3, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(md_filter_push_kernel, dim3(dF ? (unsigned)((N3 + 255) / 256) : 1u), dim3(256), 0, st, dF ? N : 0, (const int *)m.filter.perm.p,
                       (const double *)m.filter.in.p, m.filter.f.p + N3 * (size_t)(m.run.t % m.run.ring), six, ws ? m.filter.s.p + 6 * (m.run.t & 3) : (double *)nullptr);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

// The accumulators of the current configuration — what its evaluation will shrink and apply; what sgpr_md_filter takes to go on
// from here in another run: f[N][3] caller atom order, s[6] (either NULL: not wanted).
extern "C" int sgpr_md_filter_state(sgpr_model *h, double *f, double *s)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_filter_state: bad arguments");
    MdState &m = h->md;
    if (!m.active || !m.run.filter.on) return fail(SGPR_E_INVALID, "sgpr_md_filter_state: call sgpr_md_begin and sgpr_md_filter first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (f)
        if (const int rc_ = md_fetch_rows(m, m.filter.f.p + (size_t)3 * m.run.N * (size_t)(m.run.t % m.run.ring), f)) return rc_;
    if (s) {
        if (m.run.npt.on) HIPCHK(hipMemcpy(s, m.filter.s.p + 6 * (m.run.t & 3), sizeof(double) * 6, hipMemcpyDeviceToHost));
        else memcpy(s, m.run.filter.s_host, sizeof(double) * 6);
    }
    return SGPR_OK;
}

// ---- metadynamics (sgpr_md_meta; md_meta.inc has the scheme, workloads.meta_bias is the host twin) ----
// The bias of the reference's calculator/meta.py for the run begun by sgpr_md_begin, attached between any two sgpr_md_run calls
// (the first included).  cvs[ncomp][3]: the components of the collective variable in the order they are concatenated — kind 0:
// distance(i = cvs[1], j = cvs[2]); kind 1: posvar(index = cvs[1], select = cvs[2]: an atomic number, or -1 for all atoms) —
// atoms in caller order; D = sum of their dimensions (1 | 3) <= 6.  sigma[D]; w; kT > 0: well-tempered with gamma = 1 / kT, 0:
// plain; pace >= 1: configuration n deposits when n % pace == 0; capacity: rows of hills; nhills rows hills_cv[nhills][D] (and
// hills_V[nhills] or NULL: zeros) are there from the start — a restart, or the hills of sgpr_md_meta_hills when a run needs a
// larger capacity: they stand for the deposits of the configurations below the current one.  ncomp = 0 detaches.
extern "C" int sgpr_md_meta(sgpr_model *h, int ncomp, const int32_t *cvs, const double *sigma, double w, double kT, int pace, int64_t capacity,
                            int64_t nhills, const double *hills_cv, const double *hills_V)
{
#pragma clang fp contract(off)
    if (!h || ncomp < 0) return fail(SGPR_E_INVALID, "sgpr_md_meta: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_meta: call sgpr_md_begin first");
    if (ncomp == 0) { m.run.meta.on = false; return SGPR_OK; }
    if (!cvs || !sigma || ncomp > META_MAXC) return fail(SGPR_E_INVALID, "sgpr_md_meta: 1 to %d components, their list and sigma", META_MAXC);
    if (m.run.npt.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run has a barostat (sgpr_md_barostat); the bias runs at constant cell, the host loop around calculate() serves a biased NPT run");
    if (m.run.relax.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run is a relaxation (sgpr_md_relax); the bias serves dynamics only, the host loop around calculate() serves a biased relaxation");
    if (m.run.neb.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run is a nudged elastic band (sgpr_md_neb); the bias serves dynamics only, the host loop around calculate() serves a biased band");
    if (m.run.pimd.on) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run is a ring polymer (sgpr_md_pimd), whose loop does not apply a bias; the host loop around calculate() serves it");
    if (!m.run.bcm.members.empty()) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run has a committee (sgpr_md_committee), whose loop does not apply a bias; the host loop around calculate() serves it");
    if (m.run.world > 1) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run was begun on %d ranks; the bias runs on one, the host loop around calculate() serves sharded runs", m.run.world);
    if (m.run.vacf.every) return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: the run accumulates velocity correlations (sgpr_md_vacf), whose closing kick uses the packed force; the biased integrator kicks with another");
    if (pace < 1 || capacity < 1 || capacity > (1 << 28) || nhills < 0 || nhills > capacity || (nhills > 0 && !hills_cv))
        return fail(SGPR_E_INVALID, "sgpr_md_meta: pace >= 1, 1 <= capacity <= 2^28, 0 <= nhills <= capacity");
    if (!(w == w) || kT < 0.0) return fail(SGPR_E_INVALID, "sgpr_md_meta: w a number, kT >= 0");
    const int N = m.run.N;
    MetaPar p = {};
    std::vector<int> inv(N);
    for (int i = 0; i < N; i++) inv[m.run.perm[i]] = i;
    std::vector<unsigned char> sel((size_t)ncomp * N, 0);
    // what sgpr_md_meta_ql staged is this call's, whatever becomes of it
    MdRun::Meta::QlStage stage[META_MAXC];
    for (int q = 0; q < META_MAXC; q++) { stage[q] = m.run.meta.stage[q]; m.run.meta.stage[q] = MdRun::Meta::QlStage(); }
    MetaQl ql = {};
    for (int d = 0; d < META_MAXD; d++) ql.dcomp[d] = -1;
    int nql = 0;
    int D = 0;
    for (int q = 0; q < ncomp; q++) {
        const int kind = cvs[3 * q], a = cvs[3 * q + 1], b = cvs[3 * q + 2];
        if (kind != 0 && kind != 1 && kind != 2) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: kind 0 (distance), 1 (posvar) or 2 (qlvar)", q);
        if (a < 0 || a >= N) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: atom %d of %d", q, a, N);
        p.kind[q] = kind; p.ia[q] = inv[a]; p.nsel[q] = 1.0;
        if (kind == 2) {
            // Q_l of atom a over its neighbours of species b inside the staged cutoff
            if (!stage[q].set) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d is a qlvar: stage its cutoff and l with sgpr_md_meta_ql first", q);
            int slot = -1;
            for (int k = 0; k < h->S; k++)
                if (h->species[k] == b) slot = k;
            bool present = false;
            for (int i = 0; i < N; i++) present = present || m.run.numbers[i] == b;
            if (slot < 0 || !present) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: no atom of species %d (an environment of nothing)", q, b);
            if (!(stage[q].cut > 0.0) || stage[q].cut > h->rc)
                return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: cutoff %g; the list reaches rc = %g and the weight is not zero there: 0 < cutoff <= rc", q,
                            stage[q].cut, h->rc);
            if (D + stage[q].nl > META_MAXD) return fail(SGPR_E_INVALID, "sgpr_md_meta: %d dimensions; at most %d", D + stage[q].nl, META_MAXD);
            ql.slot[q] = slot; ql.cut[q] = stage[q].cut; ql.nl[q] = stage[q].nl;
            for (int k = 0; k < stage[q].nl; k++) { ql.dcomp[D + k] = q; ql.dl[D + k] = stage[q].l[k]; }
            D += stage[q].nl;
            nql++;
        } else if (kind == 0) {
            if (b < 0 || b >= N || b == a) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: distance between atoms %d and %d of %d", q, a, b, N);
            p.ib[q] = inv[b];
            D += 1;
        } else {
            int n = 0;
            for (int i = 0; i < N; i++) {
                const int cidx = m.run.perm[i];
                if (b >= 0 && m.run.numbers[cidx] != b) continue;
                n++;
                if (cidx != a) sel[(size_t)q * N + i] = 1;
            }
            if (n == 0) return fail(SGPR_E_INVALID, "sgpr_md_meta: component %d: no atom of species %d (the mean of nothing)", q, b);
            p.nsel[q] = (double)n;
            D += 3;
        }
    }
    if (D > META_MAXD) return fail(SGPR_E_INVALID, "sgpr_md_meta: %d dimensions; at most %d", D, META_MAXD);
    if ((long long)nql * h->maxnn > META_QL_MAXT)
        return fail(SGPR_E_UNSUPPORTED, "sgpr_md_meta: %d qlvar component(s) and a neighbour list of up to %d entries per atom; together at most %d: the host loop "
                    "around calculate() serves this model", nql, h->maxnn, META_QL_MAXT);
    p.D = D; p.ncomp = ncomp; p.wt = kT > 0.0 ? 1 : 0;
    p.w = w; p.gamma = kT > 0.0 ? 1.0 / kT : 0.0;
    p.norm = 1.0;
    const double sq2pi = sqrt(2.0 * M_PI);
    for (int d = 0; d < META_MAXD; d++) {
        p.sigma[d] = d < D ? sigma[d] : 1.0;
        if (!(p.sigma[d] > 0.0)) return fail(SGPR_E_INVALID, "sgpr_md_meta: sigma[%d] > 0", d);
        p.sigma5[d] = 5.0 * p.sigma[d];
        if (d < D) p.norm = p.norm * sq2pi;
    }
    std::vector<double> ce((size_t)D * nhills, 0.0), rows((size_t)(META_MAXD + 1) * nhills, 0.0);
    std::vector<int> ke((size_t)D * nhills, 0);   // (centres and keys in rows of D)
    for (int64_t r = 0; r < nhills; r++)
        for (int d = 0; d < D; d++) {
            const double c = hills_cv[(size_t)D * r + d];
            if (!(c == c)) return fail(SGPR_E_INVALID, "sgpr_md_meta: hill %lld, dimension %d is not a number", (long long)r, d);
            const double kb = std::min(std::max(floor(c / p.sigma5[d]), -1e9), 1e9);   // (clamped as md_meta_kernel clamps the live key)
            ce[(size_t)D * r + d] = (floor(c / p.sigma[d]) + 0.5) * p.sigma[d];
            ke[(size_t)D * r + d] = (int)kb;
            rows[(size_t)(META_MAXD + 1) * r + d] = c;
            rows[(size_t)(META_MAXD + 1) * r + META_MAXD] = hills_V ? hills_V[r] : 0.0;
        }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t cap = (size_t)capacity;
    if (m.meta.centre.alloc(cap * META_MAXD) || m.meta.rows.alloc(cap * (META_MAXD + 1)) || m.meta.key.alloc(cap * META_MAXD) ||
        m.meta.sel.alloc((size_t)ncomp * N))
        return fail(SGPR_E_NODEVICE, "sgpr_md_meta: device allocation failed");
    if (nhills) {
        HIPCHK(hipMemcpy(m.meta.centre.p, ce.data(), sizeof(double) * ce.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m.meta.rows.p, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m.meta.key.p, ke.data(), sizeof(int) * ke.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(m.meta.sel.p, sel.data(), sel.size(), hipMemcpyHostToDevice));
    m.run.meta.par = p; m.run.meta.pace = pace; m.run.meta.base = m.run.t; m.run.meta.pre = nhills; m.run.meta.cap = capacity;
    m.run.meta.on = true; m.run.meta.fresh = true;
    m.run.meta.merge = 0; m.run.meta.enq = 0;   // (every hill on its own until sgpr_md_meta_merge says otherwise)
    m.run.meta.ql = ql; m.run.meta.nql = nql;
    return SGPR_OK;
}

// Stages the parameters of component `comp` of the NEXT sgpr_md_meta, whose cvs triple (2, index, Zj) consumes them: the
// Steinhardt Q_l (md_meta.inc, kind 2) of atom `index` over its neighbours of species Zj with r < cutoff <= rc, one dimension per
// l[k], 0 <= l <= 12, 1 <= n_l <= 6.  After sgpr_md_begin; sgpr_md_meta takes what is staged and clears it, whether it succeeds or not.
extern "C" int sgpr_md_meta_ql(sgpr_model *h, int comp, double cutoff, int n_l, const int32_t *l)
{
    if (!h || !l) return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: bad arguments");
    MdState &m = h->md;
    if (!m.active) return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: call sgpr_md_begin first");
    if (comp < 0 || comp >= META_MAXC) return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: component %d; 0 ... %d", comp, META_MAXC - 1);
    if (n_l < 1 || n_l > META_MAXD) return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: %d values of l; 1 ... %d (one dimension each)", n_l, META_MAXD);
    for (int k = 0; k < n_l; k++)
        if (l[k] < 0 || l[k] > META_QL_MAXL) return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: l = %d; 0 ... %d", l[k], META_QL_MAXL);
    if (!(cutoff > 0.0) || cutoff > h->rc)
        return fail(SGPR_E_INVALID, "sgpr_md_meta_ql: cutoff %g; the list reaches rc = %g and the weight is not zero there: 0 < cutoff <= rc", cutoff, h->rc);
    MdRun::Meta::QlStage &s = m.run.meta.stage[comp];
    s = MdRun::Meta::QlStage();
    s.set = true; s.cut = cutoff; s.nl = n_l;
    for (int k = 0; k < n_l; k++) s.l[k] = l[k];
    return SGPR_OK;
}

// The merged form of the bias (md_meta.inc; workloads.meta_density(merge=) is the definition): from the next sgpr_md_run on the
// hills are merged by bin, chunk after chunk of `chunk` rows, and an evaluation sums one entry per occupied bin and the rows
// behind the last whole chunk.  Valid after sgpr_md_meta and before the next sgpr_md_run; chunk = 0 switches merging off again.
// The chunks of the uploaded hills are merged here, synchronously, through the kernel the loop enqueues: a run that goes on
// from the rows of sgpr_md_meta_hills with the same chunk has the bits of the run that was never interrupted.
extern "C" int sgpr_md_meta_merge(sgpr_model *h, int64_t chunk)
{
    if (!h || chunk < 0 || chunk > (1 << 28)) return fail(SGPR_E_INVALID, "sgpr_md_meta_merge: 0 <= chunk <= 2^28");
    MdState &m = h->md;
    if (!m.active || !m.run.meta.on || !m.run.meta.fresh)
        return fail(SGPR_E_INVALID, "sgpr_md_meta_merge: call sgpr_md_meta first, and this before the next sgpr_md_run");
    m.run.meta.merge = 0; m.run.meta.enq = 0;
    if (chunk == 0) return SGPR_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t cap = (size_t)m.run.meta.cap, D = (size_t)m.run.meta.par.D;
    if (m.meta.tcentre.alloc(cap * D) || m.meta.tkey.alloc(cap * D) || m.meta.tcnt.alloc(cap) || m.meta.tlast.alloc(cap) || m.meta.tstamp.alloc(cap) ||
        m.meta.ctl.alloc(META_CTL_LEN))
        return fail(SGPR_E_NODEVICE, "sgpr_md_meta_merge: device allocation failed");
    const int ctl[META_CTL_LEN] = {0, 0, 0, INT_MAX};
    HIPCHK(hipMemcpy(m.meta.ctl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice));
    m.run.meta.merge = (int)chunk;
    const long long pre = m.run.meta.pre / chunk;
    for (long long j = 0; j < pre; j++)
        hipLaunchKernelGGL(md_meta_merge_kernel, dim3(1), dim3(256), 0, h->stream, m.run.meta.par.D, m.run.meta.merge, (int)j, (const double *)m.meta.centre.p,
                           (const int *)m.meta.key.p, m.meta_tab(pre), (const int *)(m.meta.ctl.p + META_CTL_RUN), 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    m.run.meta.enq = pre;
    return SGPR_OK;
}

// The table of the merged form as the current configuration sees it (the reference's Gaussian_kde.histogram()): *n_entries
// entries in the order of the first row that occupied each, centres[*n_entries][D] and counts[*n_entries], merged from the
// first *rows_merged rows.  Any of them NULL (call once for *n_entries, then with room).
extern "C" int sgpr_md_meta_table(sgpr_model *h, double *centres, double *counts, int64_t *n_entries, int64_t *rows_merged)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_meta_table: bad arguments");
    const MdState &m = h->md;
    if (!m.active || !m.run.meta.on || !m.run.meta.merge) return fail(SGPR_E_INVALID, "sgpr_md_meta_table: call sgpr_md_begin, sgpr_md_meta and sgpr_md_meta_merge first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    int ctl[META_CTL_LEN];
    HIPCHK(hipMemcpy(ctl, m.meta.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    // (behind a halt the table may be one chunk ahead of the current configuration: that chunk is taken off, as its evaluation does)
    const long long want = std::min<long long>(m.run.meta_slot(m.run.t) / m.run.meta.merge, ctl[META_CTL_DONE]);
    const bool ahead = ctl[META_CTL_DONE] != want;
    const size_t T = (size_t)(ahead ? ctl[META_CTL_TPREV] : ctl[META_CTL_T]), D = (size_t)m.run.meta.par.D;
    if (n_entries) *n_entries = (int64_t)T;
    if (rows_merged) *rows_merged = (int64_t)(want * m.run.meta.merge);
    if (centres && T) HIPCHK(hipMemcpy(centres, m.meta.tcentre.p, sizeof(double) * T * D, hipMemcpyDeviceToHost));
    if (counts && T) {
        HIPCHK(hipMemcpy(counts, m.meta.tcnt.p, sizeof(double) * T, hipMemcpyDeviceToHost));
        if (ahead) {
            std::vector<double> last(T);
            std::vector<int> stamp(T);
            HIPCHK(hipMemcpy(last.data(), m.meta.tlast.p, sizeof(double) * T, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(stamp.data(), m.meta.tstamp.p, sizeof(int) * T, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < T; k++)
                if (stamp[k] == ctl[META_CTL_DONE] - 1) counts[k] -= last[k];
        }
    }
    return SGPR_OK;
}

// D; `below`: the hills below the current configuration — the rows uploaded at the attach and the deposits of the configurations
// before it: what sgpr_md_meta takes to go on from here —; `held`: those and the current configuration's own row where the last
// sgpr_md_run evaluated it (a halted or `final` call): what sgpr_md_meta_hills serves; the capacity.  Any of them NULL.
// (meta.fresh: no sgpr_md_run since the attach — the current configuration's own row is not in these buffers, whatever an earlier
// call evaluated)
static long long md_meta_held(const MdState &m) { return m.run.meta_slot(m.run.t) + ((m.run.evaluated && !m.run.meta.fresh && m.run.t % m.run.meta.pace == 0) ? 1 : 0); }
extern "C" int sgpr_md_meta_info(sgpr_model *h, int *D, int64_t *below, int64_t *held, int64_t *capacity)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_meta_info: bad arguments");
    const MdState &m = h->md;
    if (!m.active || !m.run.meta.on) return fail(SGPR_E_INVALID, "sgpr_md_meta_info: call sgpr_md_begin and sgpr_md_meta first");
    if (D) *D = m.run.meta.par.D;
    if (below) *below = m.run.meta_slot(m.run.t);
    if (held) *held = md_meta_held(m);
    if (capacity) *capacity = m.run.meta.cap;
    return SGPR_OK;
}

// Rows first ... first + count - 1 of the hills that stand: cv[count][D] where each was deposited and V[count], the bias its
// configuration saw (either NULL: not wanted).
extern "C" int sgpr_md_meta_hills(sgpr_model *h, int64_t first, int64_t count, double *cv, double *V)
{
    if (!h || first < 0 || count <= 0) return fail(SGPR_E_INVALID, "sgpr_md_meta_hills: bad arguments");
    const MdState &m = h->md;
    if (!m.active || !m.run.meta.on) return fail(SGPR_E_INVALID, "sgpr_md_meta_hills: call sgpr_md_begin and sgpr_md_meta first");
    const long long held = md_meta_held(m);
    if (first + count > held) return fail(SGPR_E_INVALID, "sgpr_md_meta_hills: rows %lld ... %lld asked for, %lld stand", (long long)first, (long long)(first + count - 1), held);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int D = m.run.meta.par.D;
    std::vector<double> rows((size_t)(META_MAXD + 1) * count);
    HIPCHK(hipMemcpy(rows.data(), m.meta.rows.p + (size_t)(META_MAXD + 1) * first, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < count; r++) {
        if (cv) for (int d = 0; d < D; d++) cv[(size_t)D * r + d] = rows[(size_t)(META_MAXD + 1) * r + d];
        if (V) V[r] = rows[(size_t)(META_MAXD + 1) * r + META_MAXD];
    }
    return SGPR_OK;
}

extern "C" int sgpr_md_end(sgpr_model *h)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_md_end: bad arguments");
    MdState &m = h->md;
    m.active = false;
    // what the run's modes and accumulators hold on the device is the run's: given back with it (the hills of a bias, the history
    // of L-BFGS, the origins, rings and tables of the accumulators).  The run ends whatever the waits say.
    (void)md_release(h, m.meta);
    (void)md_release(h, m.lbfgs);
    (void)md_release(h, m.msd);
    (void)md_release(h, m.rdf);
    (void)md_release(h, m.vacf);
    (void)md_release(h, m.vh);
    (void)md_release(h, m.adf);
    (void)md_release(h, m.sq);
    m.run = MdRun();   // (the borrowed members are let go with everything else the run was)
    return SGPR_OK;
}
