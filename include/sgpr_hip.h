/*
 * sgpr_hip.h — C ABI of libsgpr_hip.so: MI355X-native (gfx950) SGPR force-field evaluator.
 *
 * Drop-in boundary for AutoForce's predict hot path.  The reference has no
 * FFI for this path (it is pure Python/torch); each entry point below names the reference
 * interface it replaces (file:line under /root/reference/theforce).  A Python `Calculator`
 * binds these with ctypes (autoforce_amd/_lib.py; INTEGRATION.md shows the reference-side
 * stub).  Conventions:
 *   - every function returns an int status: 0 = ok, <0 = error (SGPR_E_*);
 *     sgpr_last_error() returns a static message for the calling thread's last failure;
 *   - all arrays are caller-allocated, row-major, fp64 / int32 unless stated;
 *   - `*_dev` variants take DEVICE pointers and a HIP stream and never synchronise;
 *     the plain variants take HOST pointers, copy, and synchronise before returning;
 *   - a handle is thread-compatible (one thread at a time), not re-entrant;
 *   - units: Angstrom, eV (as ASE), stress in eV/A^3, Voigt order xx,yy,zz,yz,xz,xy.
 * There is no CPU fallback: every entry point fails with SGPR_E_NODEVICE if no gfx950
 * device is usable.
 */
#ifndef SGPR_HIP_H
#define SGPR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgpr_model sgpr_model;

enum {
    SGPR_OK = 0,
    SGPR_E_INVALID = -1,   /* bad argument */
    SGPR_E_NODEVICE = -2,  /* no usable HIP device / HIP runtime error */
    SGPR_E_NOMODEL = -3,   /* inducing set / weights not set ("you forgot to assign a DFT calculator!", calculator/active.py:429-430) */
    SGPR_E_SPECIES = -4,   /* an atomic number is missing from the model's species table */
    SGPR_E_NOT_PD = -5,    /* "cholesky was not successful!" (regression/algebra.py:45-46) */
    SGPR_E_UNSUPPORTED = -6, /* (lmax,nmax,S) not compiled in: lmax, nmax in 2..4, S <= 8 (<= 16 for lmax = nmax = 3); least squares beyond m = 8192 */
    SGPR_E_OVERFLOW = -7   /* internal capacity exceeded after retry */
};

/* Static description of the last error on this thread. */
const char *sgpr_last_error(void);

/* Library/ABI version (major*1000+minor). */
int sgpr_version(void);

/* Number of usable gfx950 devices (0 if none; never initialises a context). */
int sgpr_device_count(void);

/* Device memory this process holds through the library's buffers, over all handles: bytes as allocated and the number of
 * allocations (either pointer may be NULL).  Page-locked host memory and the exchange buffer of sgpr_peer_export are not
 * counted.  After sgpr_destroy of every handle both are zero: a test of "nothing leaks" is a difference of two calls. */
void sgpr_live_device_memory(int64_t *bytes, int64_t *buffers);

/*
 * Create a model = kernel hyper-parameters + species table.
 * Replaces: calculator/active.py:28-38 default_kernel(lmax,nmax,exponent,cutoff) ->
 *   similarity/sesoap.py:10-24 SeSoapKernel(lmax,nmax,exponent,cutoff,radii=DefaultRadii())
 *   and descriptor/sesoap.py:102-135 SeSoap.__init__ (nnl table, radii).
 * species_z[S]: atomic numbers the model knows (the reference's 120-wide wildcard table,
 *   sesoap.py:134, restricted to those that occur); radii[S]: length unit per species
 *   (sesoap.py:84-99; DefaultRadii = 0.5 for H, 1.0 otherwise).
 * eta > 0: the exponent of k(i, q) = [Z_i == Z_q] (p_i . p_q)^eta.  4 has a branch of its own, the other integers 1 ... 64 a
 *   multiply loop, everything else (non-integers, integers above 64) pow(); an orthogonal pair (p_i . p_q = 0) has k = 0 at
 *   every exponent, and below 1 its derivative eta v^(eta - 1) is unbounded there, as in the reference.
 */
int sgpr_create(int lmax, int nmax, double eta, double rc, int S, const int32_t *species_z,
                const double *radii, int device, sgpr_model **out);
void sgpr_destroy(sgpr_model *h);

/*
 * Set the inducing set X (m local chemical environments) and build their descriptors on
 * the device, plus K_mm.
 * Replaces: descriptor/atoms.py:36-59 Local(...).stage -> similarity/universal.py:100-107
 *   precalculate for every x in model.X, and regression/gppotential.py:506 / :764-768
 *   M = kern(X, X).
 * zc[m] central atomic numbers; nbr_ptr[m+1] CSR offsets into nbr_z[] / nbr_r[][3]
 * (neighbour atomic numbers and displacement vectors r_j - r_i, as Local._b / Local._r).
 * The library sorts X by species internally; all m-sized inputs/outputs of this API stay in
 * the CALLER's order.
 */
int sgpr_set_inducing(sgpr_model *h, int m, const int32_t *zc, const int64_t *nbr_ptr,
                      const int32_t *nbr_z, const double *nbr_r);

/* K_mm in caller order, [m][m] (regression/gppotential.py:506 self.M). */
int sgpr_get_kmm(sgpr_model *h, double *M);

/* Dense p-hat of the inducing LCEs in the reference's layout [m][S][S][D],
 * D=(nmax+1)^2(lmax+1), block [sb][sa] flattened [n][n'][l] (descriptor/sesoap.py:195-203,
 * :254-258 COO block (species[b], species[a])). Test/inspection export. */
int sgpr_get_inducing_descriptors(sgpr_model *h, double *P);
/* diag(K_mm)[m], caller order. */
int sgpr_get_kmm_diag(sgpr_model *h, double *diag);
/* Row sums of K_mm [m], caller order — `self.M.sum(dim=1)` of the downsizing rule (regression/gppotential.py:815-842,
 * lii=True) without the m x m matrix crossing the bus; summed in numpy's pairwise order over the caller's column order,
 * so the values are the bits numpy gives for sgpr_get_kmm's matrix. */
int sgpr_get_kmm_rowsum(sgpr_model *h, double *sums);

/*
 * Set the regression state used by prediction.
 * Replaces: regression/gppotential.py:548-605 make_munu outputs (mu, choli),
 *   :219-227 AutoMean weights, :644-649 _vscale.
 * mu[m]; mean_w[S] per-species constant energy (may be NULL = 0); vscale[S] (may be NULL =
 * 1; use +inf for species with no inducing point, calculator/active.py:795-800);
 * choli[m][m] = L^-1 lower-triangular, caller order (may be NULL: beta is then not computed).  Entries inside a species
 * block may take any value (upper ones give up the triangular trimming of the covloss product); an entry that couples two
 * species must be zero, as in every L^-1 of the block-diagonal K_mm: otherwise SGPR_E_INVALID and nothing is changed.
 */
int sgpr_set_weights(sgpr_model *h, const double *mu, const double *mean_w, const double *vscale,
                     const double *choli);

/*
 * After a device solve (sgpr_solve / sgpr_data_solve / sgpr_resolve) mu and choli are already where prediction
 * reads them: sgpr_set_mean installs the remaining outputs of make_munu — the AutoMean weights
 * (regression/gppotential.py:219-227) and, optionally, _vscale (NULL: keep the one sgpr_make_vscale computed) —
 * without moving the m x m choli over PCIe and back.  sgpr_get_choli downloads choli[m][m] (caller's order) for the
 * callers that still want it on the host (leakage, gppotential.py:706-713; model files).
 */
int sgpr_set_mean(sgpr_model *h, const double *mean_w, const double *vscale);
int sgpr_get_choli(sgpr_model *h, double *choli);
/* The end of a rejected trial (add_1inducing / add_1atoms_fast, gppotential.py:898-982: edit, refit, measure, pop,
 * refit): after the pop the model is the one the trial started from, so the caller hands back the mu it saved instead
 * of asking for the same fit again.  The K_mm factor (hence choli) of the restored inducing set is the cached one or
 * is recomputed here; follow with sgpr_set_mean for the mean / _vscale. */
int sgpr_restore_weights(sgpr_model *h, const double *mu);

/*
 * Solve side on the device (regression/gppotential.py:1204-1339 _regression with
 * optimize=False; regression/algebra.py:29-47 jitcholesky):
 *   L, ridge = jitcholesky(K_mm); choli = L^-1; sigma = noise0*0.99*mean(diag K_mm);
 *   mu = argmin |[K; sigma L^T] mu - [Y; 0]|, K = [Ke;Kf;Kv] (rows x m, caller order).
 * On success installs mu/choli in the handle (as sgpr_set_weights) and returns them.
 * Returns SGPR_E_NOT_PD when the jitter ladder is exhausted.
 */
int sgpr_solve(sgpr_model *h, int rows, const double *K, const double *Y, double noise0,
               double *mu_out, double *choli_out, double *ridge_out, double *sigma_out);

/*
 * jitcholesky of a matrix the caller holds (regression/algebra.py:29-47): L L^T = A + ridge I with the reference's
 * ladder — ridge 0 first, then 1e-6 * mean(diag A) doubled until the factorisation succeeds; SGPR_E_NOT_PD
 * ("cholesky was not successful!", :45-46) once the ridge exceeds mean(diag A).  A: host, row-major n x n
 * (symmetric; the lower triangle is read).  L_out (may be NULL): row-major n x n, upper triangle zero.
 */
int sgpr_jitcholesky(sgpr_model *h, int n, const double *A, double *L_out, double *ridge_out);

/* The same regression for another noise value, with the design matrix of the last sgpr_solve:
 * the QR of [K | Y] is kept on the device (R, Q^T Y), the noise only enters a 2m x m second stage.
 * This is what _regression(optimize=True) evaluates repeatedly (gppotential.py:1265-1300). */
int sgpr_resolve(sgpr_model *h, double noise0, double *mu, double *choli, double *ridge, double *sigma);
/* The same for `count` (<= 64) noise values in one go, mu_out[count][m]: the grid scan of the noise search
 * (gppotential.py:1283-1296 describes it) as ONE batch of independent second-stage problems sharing every kernel
 * launch.  Evaluation only: the weights installed for prediction stay those of the last sgpr_solve / sgpr_resolve. */
int sgpr_resolve_batch(sgpr_model *h, int count, const double *noise, double *mu_out);

/*
 * Training rows of one data frame against the inducing set, on the device
 * (regression/gppotential.py:63-84 energy_energy / forces_energy / virial_energy through
 * similarity/universal.py:109-183 get_func / get_leftgrad / get_virial; used by set_data :495-497
 * and add_data :728-737):
 *   Ke[m]     = sum_i k(i,q)
 *   Kf[3N][m] = -d(sum_i k(i,q))/dx   (row 3*atom+component, caller atom order)
 *   Kv[6][m]  = sum_pairs r (x) dk/dr, Voigt xx,yy,zz,yz,xz,xy (pairs with stress * volume)
 * computed as m reverse passes with mu = e_q (exact derivative; the reference's analytic path
 * carries an fp32-rounded table and agrees to ~1e-6).  Any output may be NULL.
 */
int sgpr_kernel_rows(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                     const double *cell, const int32_t *pbc, double *Ke, double *Kf, double *Kv);

/* The same for the inducing columns [q_first, q_first + q_count) only: outputs are Ke[q_count],
 * Kf[3N][q_count], Kv[6][q_count].  This is the bordering step of add_inducing
 * (gppotential.py:745-772: one new column of K_e, K_f, K_v per data frame). */
int sgpr_kernel_columns(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                        const double *cell, const int32_t *pbc, int q_first, int q_count, double *Ke,
                        double *Kf, double *Kv);

/*
 * Resident training set: the regression's design matrix K = [K_e; K_f; K_v] of the stored data frames, kept in
 * device memory for the life of the model (the reference keeps it as torch tensors next to the model:
 * PosteriorPotential.set_data / add_data / pop_1data / popfirst_1data, regression/gppotential.py:484-509,
 * :730-743, :793-813).  Rows are frame-major: frame f owns 1 + 3N_f + nv_f consecutive rows (its energy row, its
 * force rows in the caller's atom order, then nv = 0 or 6 virial rows in Voigt order); columns are the inducing LCEs
 * in the caller's order.  The inducing-set entry points below keep the columns in step (sgpr_add_inducing computes
 * ONE new column per stored frame on the device, gppotential.py:745-772; remove / select re-index; sgpr_set_inducing
 * recomputes), so after any sequence of edits the matrix equals what sgpr_kernel_rows would return for every frame.
 *
 *   sgpr_data_push    append a frame (its rows are computed on the device and stay there)
 *   sgpr_data_pop     drop frame `index` (-1 = last: pop_1data; 0: popfirst_1data)
 *   sgpr_data_clear   drop all frames
 *   sgpr_data_info    number of frames / rows
 *   sgpr_data_matvec  out[rows] = K v   (v[m] in the caller's column order): fit residuals, k·mu of a stored frame
 *   sgpr_data_fit_stats  make_stats (gppotential.py:610-649) without the residual vector: e_pred[frames] = the
 *                     energy rows of K v, stats[7] = {sum d, sum |d|, sum d^2, sum y, sum y^2, max |y|, count} of
 *                     d = K v - Y over the force and virial rows
 *   sgpr_data_get     K[rows][m] row-major (diagnostics and tests; the product path never needs it)
 *   sgpr_data_solve   sgpr_solve on the resident matrix: Y[rows] in the same row order; with_energies = 0 drops
 *                     the energy rows (the force-only fit of _regression(optimize=True), gppotential.py:1265-1300);
 *                     sgpr_resolve re-solves it for another noise as after sgpr_solve.
 *   sgpr_data_factor  the first stage of sgpr_data_solve alone (K_mm factor, R1 and z kept on the device for
 *                     sgpr_resolve / sgpr_resolve_batch); no weights are produced or installed.
 */
int sgpr_data_push(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                   const int32_t *pbc, int nv);
int sgpr_data_pop(sgpr_model *h, int index);
int sgpr_data_clear(sgpr_model *h);
int sgpr_data_info(sgpr_model *h, int32_t *frames, int64_t *rows);
int sgpr_data_matvec(sgpr_model *h, const double *v, double *out);
int sgpr_data_fit_stats(sgpr_model *h, const double *v, const double *Y, double *e_pred, double *stats);
/* mae_out[b] = mean |K_f V[b] - Y_f| over the force rows of the resident matrix, for `count` weight vectors V[count][m]
 * against the targets Y[rows] (store order): the objective of the noise search of _regression(optimize=True)
 * (regression/gppotential.py:1265-1300), reduced on the device in a fixed order, sixteen vectors per pass over the matrix. */
int sgpr_data_force_mae(sgpr_model *h, int count, const double *V, const double *Y, double *mae_out);
int sgpr_data_get(sgpr_model *h, double *K);
int sgpr_data_solve(sgpr_model *h, const double *Y, int with_energies, double noise, double *mu_out,
                    double *choli_out, double *ridge_out, double *sigma_out);
int sgpr_data_factor(sgpr_model *h, const double *Y, int with_energies);
/* Diagnostics of the last sgpr_data_solve / sgpr_data_factor: which route the first stage took ("full factorisation",
 * "columns appended / popped through the kept reflectors", "kept", "rows of the new frame appended to the kept
 * factor", "found in the cache", "from scratch") and how many species blocks of K_mm were factored, as text
 * ("stage1=...; stage2=...; kmm_blocks=a/b; step=...; rows=...", rows= last: stage2 = "factorisation" or, for the model a kept second stage was
 * made for asked again / with one appended column, "kept reflectors, ...").  The reference always refits from scratch (gppotential.py:548-605); tests use
 * this to assert that an edit (append, pop, select / downsize) was followed incrementally.  "rows=" names the kernel
 * form of the last rows / columns call: "sixteen columns per workgroup pass" (lmax and nmax <= 3, <= 4 species, lists of
 * <= 64 neighbours) or "one column per wave".  "step=knmA wcovB chainC cov=D" names the GEMM tile forms of the last
 * step: A and B the row heights (16, 32 or 64) of the K_nm and the W + covloss tiles, C the number of W + covloss tiles
 * chained behind another one in the grouped launch (0: none, or covloss not grouped), D where the covloss product ran:
 * "grouped" (one launch with W), "alone" (no W: no weights), "rev" (in the reverse kernel's launch), "fused" (one launch
 * with K_nm and W), "forked" (side stream) or "none". */
int sgpr_solve_info(sgpr_model *h, char *buf, int cap);

/*
 * Inducing-set edits (PosteriorPotential.add_inducing / pop_1inducing / popfirst_1inducing /
 * select_inducing, gppotential.py:745-842, :1037-1046).  The caller's order is kept: a new LCE is
 * appended as index m; `remove` deletes one index (-1 = last); `select` keeps `indices` in the
 * given order (downsize(lii=True), gppotential.py:829-832, selects the max_inducing LCEs with the smallest K_mm
 * row sums in argsort order).  All three are incremental on the device: descriptors, K_mm and the resident design
 * matrix are re-indexed (one new row / column for an appended LCE), the cached K_mm factor is bordered (append),
 * trimmed (pop) or re-factored per species block (select), and the kept first-stage QR of [K | Y] follows
 * through its reflectors; weights are invalidated (call sgpr_solve / sgpr_data_solve / sgpr_set_weights next, as
 * the reference calls make_munu).
 */
int sgpr_add_inducing(sgpr_model *h, int32_t zc, int nn, const int32_t *nbr_z, const double *nbr_r);
int sgpr_remove_inducing(sgpr_model *h, int index);
int sgpr_select_inducing(sgpr_model *h, int count, const int32_t *indices);

/* k(loc, X)[m] and k(loc, loc) for one LCE that is not (yet) in the inducing set
 * (gp.kern(loc, X) in ActiveCalculator.update_lce, active.py:806-818, and
 * PosteriorPotential.leakage, gppotential.py:706-713).  Either output may be NULL. */
int sgpr_kernel_local(sgpr_model *h, int32_t zc, int nn, const int32_t *nbr_z, const double *nbr_r,
                      double *k_out, double *kxx_out);

/* vscale[S] = mean_{q: Z_q = z} mu_q (K_mm mu)_q (regression/gppotential.py:644-649);
 * +inf where a species has no inducing point. Installs it in the handle as well. */
int sgpr_make_vscale(sgpr_model *h, double *vscale_out);

/*
 * One prediction = one MD step of the hot path.
 * Replaces: calculator/active.py:425-502 ActiveCalculator.calculate ->
 *   descriptor/atoms.py:384-413 TorchAtoms.update (neighbour list :348-363, Local :365-382,
 *   descriptors sesoap.py:161-260), regression/gppotential.py:63-84 K_nm,
 *   calculator/active.py:548-611 energy / autograd forces / stress, :781-804 covloss.
 * Inputs (host): numbers[N], positions[N][3], cell[3][3] (rows = lattice vectors), pbc[3].
 * shard: atoms are dealt to `world` ranks; this call evaluates rank `rank`'s share only and
 *   returns PARTIAL sums (energy without the mean term on rank != 0, forces on all N atoms
 *   from this rank's LCEs, beta zero outside the share) to be summed over ranks
 *   (calculator/active.py:562,600-602,770-777).  world = 1 for a single process.
 * Outputs (host, any may be NULL): energy[1]; forces[N][3]; stress[6]; beta[N] =
 *   covloss (already scaled by sqrt(vscale)); cov[N][m] = K_nm rows in caller order (zero
 *   rows outside the share).
 */
int sgpr_compute(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                 const double *cell, const int32_t *pbc, int rank, int world, double *energy,
                 double *forces, double *stress, double *beta, double *cov);

/* sgpr_compute without the copies out: *packed_out points at this call's results where the device wrote them — page-locked
 * host memory owned by the handle, [F 3N | beta N | E | virial 9 (row-major) | overflow word | stress 6 (Voigt)], caller atom
 * order — valid until the call AFTER THE NEXT on this handle (two buffers alternate: the previous call's results stay
 * intact while this one runs; a buffer that a larger frame replaces is kept for one more generation).  N >= 1 (an empty
 * frame has nothing to point at: sgpr_compute returns its zeros).  What ActiveCalculator.results hands out as views (the reference's results are views of
 * tensors the calculator owns, calculator/active.py:572-574; ASE copies what it passes on). */
int sgpr_compute_view(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                      const int32_t *pbc, int rank, int world, const double **packed_out);

/*
 * Device-resident form for MD loops and benchmarks: no host copies, no synchronisation.
 * sgpr_bind_system fixes N, numbers, pbc and the sharding (host arrays; may be called again
 * when they change); sgpr_step_dev consumes DEVICE positions[N][3] + cell[9] and fills the
 * DEVICE buffer `packed` (length sgpr_packed_len(N) doubles):
 *   packed[0..3N)      forces (partial over ranks)
 *   packed[3N..4N)     beta   (this rank's share, 0 elsewhere)
 *   packed[4N]         energy (partial; mean term added on rank 0 only)
 *   packed[4N+1..+9)   virial sum_pairs r (x) dE/dr (partial), row-major 3x3
 *   packed[4N+10]      1 if this rank's step overflowed a capacity (results invalid), else 0
 * (Sharded steps accumulate the forces neighbours receive as 64-bit fixed-point integers, 2^-46 eV/A per unit, so that a
 * rank's partial sums do not depend on the order the atomics land in: a single pair force beyond 1024 eV/A — two atoms
 * unphysically close — is outside that format and fails the step with SGPR_E_OVERFLOW; the unsharded path has no such limit.)
 * i.e. exactly what one all-reduce(SUM) over ranks must combine (the reference's four
 * collectives calculator/active.py:562,601,602,777 fused into one buffer).  With a communicator
 * attached (sgpr_comm_init) the step ends with that all-reduce, enqueued on the same stream: the
 * buffer then holds the TOTALS on every rank, and packed[4N+10] > 0 tells every rank alike that some
 * rank must repeat the step (sgpr_sync_check on each rank, then the step again).
 * `stream` is a hipStream_t passed as void*.  With option "graph" the step is captured into a HIP graph on first
 * use and replayed afterwards.
 */
int sgpr_bind_system(sgpr_model *h, int N, const int32_t *numbers, const int32_t *pbc, int rank,
                     int world);
int64_t sgpr_packed_len(int N);
int sgpr_step_dev(sgpr_model *h, const double *positions_dev, const double *cell_dev,
                  double *packed_dev, void *stream);
/*
 * sgpr_step_dev with the DEVICE positions of the step that follows named (same cell buffer): the last kernel of this
 * step bins them and takes the rebuild decision of the next step's neighbour candidates, so the next call — which must
 * pass exactly `positions_next_dev` — starts with the list filter instead of a binning launch (6 -> 5 launches per
 * step).  A call that passes anything else is served as usual.  positions_next_dev = NULL: sgpr_step_dev.
 * The next step is binned with the cell AS IT IS NOW: a driver that changes the contents of `cell_dev` between two steps
 * (NPT) passes NULL for the step in front of the change — every step of such a run bins for itself.  (A chain that runs in
 * another cell than the one its candidate lists were built in notices — the last kernel compares the two — and rebuilds
 * them at its next step.)
 * (The reference asks ASE for a fresh list inside every calculate(), descriptor/atoms.py:348-363, :402.)
 */
int sgpr_step_dev_next(sgpr_model *h, const double *positions_dev, const double *cell_dev,
                       double *packed_dev, const double *positions_next_dev, void *stream);

/*
 * Device-resident molecular dynamics.  The reference integrates in ASE — ase.md.langevin.Langevin around the
 * calculator (cl/md.py:117-128), velocities from util/aseutil.py:11-20 — and crosses into calculate() once per step,
 * whose covloss gate (calculator/active.py:492-499, :842-885: update when the largest covloss reaches ediff) decides
 * whether the model is edited.  Here positions and velocities live in device memory, the integrator (BAOAB Langevin;
 * friction = 0: velocity Verlet) is part of the step's last kernel, and the gate halts the run on the device.
 *
 * sgpr_md_begin   binds the system (single process), uploads positions[N][3], velocities[N][3] (NULL: zero) and
 *                 masses[N] (caller atom order), fixes dt, friction (per unit time) and kT (energy units):
 *                 c1 = exp(-friction dt), sigma_i = sqrt(1 - c1^2) sqrt(kT / m_i).
 * sgpr_md_run     evaluates `nevals` configurations starting with the current one.  After every evaluation (with
 *                 final_eval != 0: every one but the last) the state moves on:
 *                     v += (dt/2) F/m;  x += (dt/2) v;  v = c1 v + sigma xi;  x += (dt/2) v;  [evaluate]  v += (dt/2) F/m
 *                 with xi the next row of noise[nevals][N][3] (standard normal deviates, caller atom order; NULL: none).
 *                 scalars[nevals][16] (may be NULL) receives per evaluation: E, virial[9] (row-major), the capacity
 *                 overflow word, the largest covloss, sum_i m_i v_i^2 with the velocities AFTER the closing half kick and
 *                 BEFORE it (what a calculator inside the integrator's step is handed, cl/md.py:117-128), 0, 0.
 *                 The run stops at the first evaluation whose largest covloss is >= ediff (ediff <= 0: never):
 *                 *evals_done then counts that evaluation as the last one, *halt_code = 1, and the state IS that
 *                 configuration — the next sgpr_md_run evaluates it again, with whatever model the caller has installed
 *                 meanwhile, exactly as the reference recomputes the results after an update
 *                 (calculator/active.py:477-484).  *halt_code = 2: a neighbour capacity overflowed at evaluation
 *                 *evals_done (not counted); the next call re-sizes and repeats it.
 * sgpr_md_state   positions[N][3], velocities_pre[N][3] (before the closing half kick; *pending says whether one is
 *                 due) of the current configuration (which = 0) or of the one before it (which = -1), and the packed
 *                 results (sgpr_step_dev layout, length sgpr_packed_len(N)) of that configuration's last evaluation;
 *                 any pointer may be NULL.
 * Same-seed runs are bit-reproducible; with the same noise rows the trajectory equals the host-side loop around
 * sgpr_compute bit for bit (tests/test_hip_md.py).
 */
int sgpr_md_begin(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                  const int32_t *pbc, const double *masses, const double *velocities, double dt, double friction,
                  double kT);
int sgpr_md_run(sgpr_model *h, int nevals, const double *noise, double ediff, int final_eval, double *scalars,
                int *evals_done, int *halt_code);
int sgpr_md_state(sgpr_model *h, double *positions, double *velocities_pre, int *pending, double *packed, int which);
/* The velocities an observer sees at the current configuration (evaluated by the last sgpr_md_run: a halt, or final_eval):
 * the closing half kick applied (Langevin / velocity Verlet), or the centred velocity (Nose-Hoover, sgpr_md_thermostat — there
 * sgpr_md_state's velocities_pre of configuration n is v_(n-1): what the integrator holds when it asks for F_n). */
int sgpr_md_velocities(sgpr_model *h, double *velocities);
int sgpr_md_end(sgpr_model *h);
/* Deviates drawn on the device: with a seed != 0, sgpr_md_run called with noise = NULL draws xi itself — deviate
 * (configuration index, atom, component) of a counter-based generator (Philox4x32-10, Box-Muller), so a run does not
 * depend on how it is cut into calls and an evaluation repeated after a halt draws the same numbers; no host generator
 * and no upload on the step's path (the reference draws from numpy inside ase.md.langevin, cl/md.py:117-128).
 * sgpr_md_deviates returns the rows of configurations [t_first, t_first + count): out[count][N][3], caller atom order. */
int sgpr_md_seed(sgpr_model *h, uint64_t seed);
/* Nose-Hoover NVT instead of the Langevin / velocity-Verlet step (kind = 1; 0 = back): the reference's DEFAULT dynamics,
 * md(dynamics="NPT", bulk_modulus=None) = ase.md.npt.NPT with pfactor = None, ttime = tdamp fs (cl/md.py:17, :131-166;
 * Melchionna, Ciccotti, Holian 1993 as ASE integrates it):
 *     x_(n+1) = (2 x_n - x_(n-1) (1 - b) + dt^2 F_n / m) / (1 + b),  b = dt zeta_n / 2,  v_n = (x_(n+1) - x_(n-1)) / 2 dt,
 *     zeta_(n+1) = zeta_(n-1) + 2 dt tfact (KE_n - 1.5 (N - 1) kT),  tfact = 2 / (3 N kT ttime^2),
 * started with x_(-1) = x_0 - dt v_0 + dt^2 F_0 / 2m, zeta_0 = 0, zeta_(-1) = -dt tfact (KE_0 - ...).  The integrator stays
 * in the step's last kernel; zeta_(n+1) needs the kinetic energy of ALL atoms at step n, reduced by one small launch
 * behind each evaluation.  Call between sgpr_md_begin and the first sgpr_md_run.  scalars[.][12] = [13] = sum m v_n^2 with
 * the centred velocities, [14] = zeta_n, [15] = its time integral (the conserved quantity is
 * E + KE + 1.5 N kT (ttime zeta)^2 + 3 (N - 1) kT int zeta dt, ASE's get_gibbs_free_energy).  sgpr_md_state returns the
 * centred velocities (pending = 0). */
int sgpr_md_thermostat(sgpr_model *h, int kind, double ttime, double kT);
int sgpr_md_deviates(sgpr_model *h, int64_t t_first, int count, double *out);
/* A barostat on top of the Nose-Hoover thermostat (between sgpr_md_thermostat(kind = 1) and the first sgpr_md_run): the
 * combined Nose-Hoover / Parrinello-Rahman dynamics of ase.md.npt.NPT with a pfactor — the moving cell the reference's command
 * line runs when a bulk modulus is given (cl/md.py:131-166) — inside the device loop: cell, strain rate eta and scaled
 * coordinates live in rings on the device, one small launch behind each evaluation advances them, and the step's last kernel
 * moves the atoms into the NEXT cell, bins them there and keeps the candidate lists while the strain since their build
 * allows it.  pfactor = ptime^2 x bulk modulus; externalstress[6] (Voigt xx yy zz yz xz xy; a pressure P is -P, -P, -P, 0, 0, 0);
 * mask[9] zeros and ones: the cell components that may move (NULL: all); frac_traceless: 1 = the whole strain rate (masked),
 * 0 = its trace only (an isotropic cell; ASE applies no mask then).  Units as given to sgpr_md_begin.
 * SGPR_E_INVALID: a cell that is not upper triangular (h[1][0] = h[2][0] = h[2][1] = 0 exactly), a direction that is not
 * periodic, pfactor <= 0, no Nose-Hoover thermostat, a run that has started.  SGPR_E_UNSUPPORTED: a run begun on more than one
 * rank (the sharded last kernel integrates at constant cell), held components, a bias.  The handle goes on working after any of
 * them.  A run with a committee (sgpr_md_committee before or after this call) is refused likewise unless the run's option
 * "md_committee_cell" is set (sgpr_set_option, after sgpr_md_begin); with it it is accepted: every member is evaluated in the cell
 * of the configuration and the barostat integrates the committee's combined stress.
 * scalars of sgpr_md_run as for Nose-Hoover (14 / 15: zeta and its integral).  sgpr_md_state returns the positions of the
 * current configuration in ITS cell:
 * sgpr_md_cells   out[count][18] = cell h[9] (rows = cell vectors) and strain rate eta[9] of the configurations first ...
 *                 first + count - 1 (index in the trajectory, 0 = the configuration of sgpr_md_begin): any evaluated by the
 *                 last sgpr_md_run, and the current one. */
int sgpr_md_barostat(sgpr_model *h, double pfactor, const double *externalstress, const double *mask, double frac_traceless);
int sgpr_md_cells(sgpr_model *h, int64_t first, int count, double *out);
/* A relaxation instead of dynamics (between sgpr_md_begin and the first sgpr_md_run; no thermostat, no barostat): FIRE
 * (ase/optimize/fire.py, ASE 3.22) on the positions and, with move_cell, on the cell through the generalised coordinates of
 * ase.constraints.UnitCellFilter(atoms, mask) — what the reference's relax(cell=True) minimises (cl/relax.py:45-48) — with the
 * state in device memory between model updates.  With h0 the cell of sgpr_md_begin, D the deformation gradient, c = N:
 *     h = h0 D^T,  x = r D^T,  X = [ r ; c D ],  G = [ F D ; (W D^-T o M) / c ],  W = -V stress
 * and FIRE acting on (X, G) over all 3N (+ 9) components.  sgpr_md_begin's masses (NULL is accepted), velocities, dt, friction
 * and kT are ignored.  fire[8] = dt, maxstep, dtmax, nmin, finc, fdec, astart, fa (NULL: ASE's 0.1, 0.2, 1.0, 5, 1.1, 0.5, 0.1,
 * 0.99); mask6: zeros and ones for the Voigt components xx yy zz yz xz xy of the cell (NULL: all ones).
 * sgpr_md_run (its noise is ignored) evaluates and moves; the covloss gate (halt code 1) and a capacity overflow (2) work as in
 * an MD run, and convergence — max over the N (+ 3) rows of |G_row|^2 < fmax^2 — is halt code 3: *evals_done counts the
 * converged evaluation as the last one and the state IS that configuration, nothing moved.  final_eval: the last evaluation
 * of the call moves nothing and leaves the optimizer as it was.
 * scalars[.][0..11] as in an MD run; [12] = max |G_row|^2, [13] = G.v (0 for the optimizer's first evaluation), [14] = dt and
 * [15] = a as used for the move out of this evaluation (as they stand when nothing moves).
 * sgpr_md_cells returns h[9] and, in the place of eta, D[9] per configuration; sgpr_md_state the positions in the
 * configuration's own cell and, as velocities_pre, the optimizer's velocity of the atoms' coordinates (pending = 0).
 * SGPR_E_INVALID: a thermostat or barostat set, a run that has started, fmax <= 0, a FIRE parameter out of range, move_cell
 * with a direction that is not periodic or a singular cell.  SGPR_E_UNSUPPORTED: a run begun on more than one rank.  The handle
 * goes on working after any of them.
 * sgpr_md_relax_reset  optimizer.initialize(): v = 0 and dt, a, nsteps back to their start (between two sgpr_md_run calls). */
int sgpr_md_relax(sgpr_model *h, double fmax, const double *fire, int move_cell, const double *mask6);
int sgpr_md_relax_reset(sgpr_model *h);
/* L-BFGS without line search in the place of FIRE (md_lbfgs.inc; ase/optimize/lbfgs.py, ASE 3.22, restated): between sgpr_md_relax
 * — whose fmax, move_cell and mask6 hold, whose refusals apply as they are and whose FIRE keywords go unused — and the first
 * sgpr_md_run.  memory: pairs (s, y) kept at most, 1 ... 128; maxstep, alpha (H0 = 1 / alpha), damping: ASE's keywords
 * (defaults 100, 0.2, 70, 1).  p = H G is formed in the compact representation of Byrd, Nocedal and Schnabel (1994) from one
 * pass of sums over the history; a pair whose s.y is zero or not finite is left out (ASE would divide by it).  The history,
 * 2 memory (3N + 9) doubles of device memory, is indexed by evaluation: a cut run gives the bits of an uncut one, and an
 * evaluation repeated behind a covloss halt writes its own pair again.  sgpr_md_relax_reset empties it; sgpr_md_end gives it back.
 * The columns 12..15 of a row of sgpr_md_run: [12] = largest |G_row|^2, [13] = p.G, [14] = the scale applied to the step
 * (maxstep / longest, or 1), [15] = valid pairs in use; [13] and [14] are 0 where nothing moves.
 * SGPR_E_INVALID: no relaxation set up, a run that has started, memory outside 1 ... 128, a keyword <= 0.  SGPR_E_NODEVICE: no
 * room for the history.  The handle goes on working after any of them. */
int sgpr_md_relax_lbfgs(sgpr_model *h, int memory, double maxstep, double alpha, double damping);
/* Nudged elastic band with FIRE inside the device loop (md_neb.inc; the reference's cl/neb.py drives ase.neb.NEB under an
 * ase.optimize optimizer and crosses into the calculator once per image per step).  ASE's default `aseneb` method, restated:
 * images 0 ... K + 1 share numbers, cell (constant) and pbc; the ends never move and are never evaluated; with the model's
 * forces F_i (zero on held components) and energies E_i of the interior images i = 1 ... K and one spring constant k
 *     t_i = mic(R_i - R_(i-1)),  i = 1 ... K + 1      per atom d - rint(d h^-1) h in the periodic directions
 *     imax = the interior image of highest energy (the later one on a tie)
 *     tau_i = t_(i+1) for i < imax,  t_i for i > imax,  t_i + t_(i+1) for i = imax
 *     G_i = F_i - (F_i.tau_i / tau_i^2) tau_i - (((k t_i - k t_(i+1)).tau_i) / tau_i^2) tau_i
 *     climb, i = imax:  G_i = F_i - 2 (F_i.tau_i / tau_i^2) tau_i
 * and FIRE (sgpr_md_relax's recurrence at constant cell) on the concatenated K N rows: ONE dt, a, nsteps and step limit for the
 * band, G.v, G.G, v.v summed over all interior images, converged when max over all K N rows of |G_row|^2 < fmax^2.
 * sgpr_md_neb        after sgpr_md_begin (positions: any interior image — they bind the system; masses, velocities, dt, friction
 *                    and kT are ignored) and, if used, sgpr_md_fix (one mask for every image; a held component's velocity is 0
 *                    and its coordinate keeps its bits), before the first sgpr_md_run.  positions[K + 2][N][3] caller atom order;
 *                    fire[8] as in sgpr_md_relax (NULL: ASE's defaults).  SGPR_E_INVALID: K < 1 or K > 16, a thermostat or
 *                    barostat, a run that has started, fmax <= 0, k_spring <= 0, a singular cell with a periodic direction, and an
 *                    initial band the rounding cannot recover: a fractional component of a displacement between neighbouring
 *                    images, after rounding, within 1e-9 of +-1/2, or such a displacement longer than half the smallest
 *                    perpendicular width of the cell — the caller keeps neighbouring images closer than that for the whole run
 *                    (only the initial band is checked).  SGPR_E_UNSUPPORTED: more than one rank, a committee, a filter, a
 *                    relaxation (sgpr_md_relax), an armed frame record.
 * sgpr_md_run        evaluates the band (K plain steps of this handle, each rebuilding its candidate lists) and moves it;
 *                    halt code 1: the largest covloss over all images reached ediff (nothing moved), 2: a capacity overflowed at
 *                    some image, 3: converged.  scalars[.][0] = E of imax, [1] = imax, [2] = the image that carried the largest
 *                    covloss (both 1 ... K), [10] overflow, [11] largest covloss, [12] max |G_row|^2, [13] G.v, [14] dt, [15] a
 *                    as used for the move out of the evaluation; the others zero.
 * sgpr_md_neb_reset  optimizer.initialize(): v = 0 and dt, a, nsteps back to their start (between two sgpr_md_run calls).
 * sgpr_md_neb_state  the K interior images, caller atom order: positions[K][N][3] of the current band (which = 0) or the one
 *                    before it (-1), velocities[K][N][3] (FIRE's), packed[K][4N + 11] the images' results where the last
 *                    sgpr_md_run evaluated that band; any of them NULL.  sgpr_md_state refuses a band.
 * sgpr_md_neb_info   out[count][32] = E[16] | covmax[16] per evaluation first ... first + count - 1 of the last sgpr_md_run
 *                    (0 = its first) among those that stand; kept on the device during the call, fetched behind its one wait.
 * sgpr_md_record, sgpr_md_committee, sgpr_md_filter, sgpr_md_thermostat, sgpr_md_relax and sgpr_md_fix behind sgpr_md_neb are
 * refused. */
int sgpr_md_neb(sgpr_model *h, int K, const double *positions, double fmax, double k_spring, int climb, const double *fire);
int sgpr_md_neb_reset(sgpr_model *h);
int sgpr_md_neb_state(sgpr_model *h, double *positions, double *velocities, double *packed, int which);
int sgpr_md_neb_info(sgpr_model *h, int first, int count, double *out);
/* Path-integral molecular dynamics inside the device loop (md_pimd.inc; the reference's calculators declare the mode —
 * ActiveCalculator(nbeads=P) — and are driven bead by bead from outside).  A ring polymer of P beads, 1 <= P <= 32, all
 * evaluated by this one handle; physical temperature T, the polymer sampled at kT_P = P kT with w_P = kT_P / hbar (the RPMD
 * convention; hbar = 0.06465415105180661 in eV, A, amu: the units of the run):
 *     H_P = sum_j sum_i [ m_i v_ij^2 / 2 + m_i w_P^2 / 2 |x_ij - x_i,j+1|^2 ] + sum_j V(x_j)       (raw coordinates, no minimum image)
 * integrated by BAOAB with the PILE-L thermostat (Ceriotti et al., J. Chem. Phys. 133, 124104; Liu, Li, Liu, J. Chem. Phys.
 * 145, 024103): behind the forces of evaluation n the closing half kick of step n - 1, the opening half kick, then in the normal
 * modes of the free ring polymer (x~_k = sum_j C[j][k] x_j, w_k = 2 w_P sin(k pi / P)) the exact free propagation over dt / 2,
 * v~_k <- c1_k v~_k + c2_k sqrt(kT_P / m) xi with c1_k = exp(-gamma_k dt), gamma_0 = friction, gamma_k = 2 lambda w_k, and the
 * free propagation over dt / 2 again.  friction = 0, lambda = 1/2: TRPMD; friction = lambda = 0: microcanonical RPMD.  At P = 1
 * the scheme is sgpr_md_begin's Langevin step, operation for operation.
 * sgpr_md_pimd        after sgpr_md_begin (positions: any bead — they bind the system; its masses and dt hold; its velocities,
 *                     friction and kT are replaced by this call's), before the first sgpr_md_run.  positions[P][N][3],
 *                     velocities[P][N][3] (NULL: zeros), caller atom order.  SGPR_E_INVALID: P < 1 or P > 32, a thermostat or
 *                     barostat, a run that has started, kT <= 0, friction < 0, lambda < 0.  SGPR_E_UNSUPPORTED: more than one
 *                     rank, a committee, a bias, a filter, held components, an armed frame record, a relaxation, a band.
 * sgpr_md_run         evaluates the polymer (P plain steps of this handle, each rebuilding its candidate lists) and moves it;
 *                     noise[nevals][P][N][3]: the deviates of mode k, caller atom order (NULL: none, or — sgpr_md_seed — those
 *                     sgpr_md_deviates returns for t = n P + k).  Halt code 1: the largest covloss over all beads reached ediff
 *                     (nothing moved), 2: a capacity overflowed at some bead.  scalars[.][0] = the mean of the beads' energies,
 *                     [1] = the bead (1 ... P) that carried the largest covloss, [10] overflow, [11] largest covloss, [12] | [13]
 *                     sum m v^2 over all beads after | before the closing half kick, [14] the centroid-virial kinetic energy
 *                     3 N kT / 2 - (1 / 2P) sum_j sum_i (x_ij - xbar_i).F_ij, [15] the spring energy; the others zero.
 * sgpr_md_pimd_state  the P beads, caller atom order: positions[P][N][3] of the current configuration (which = 0) or the one
 *                     before it (-1), velocities_pre[P][N][3] before its closing half kick, packed[P][4N + 11] the beads'
 *                     results where the last sgpr_md_run evaluated that configuration; any of them NULL.  sgpr_md_state and
 *                     sgpr_md_velocities refuse a polymer.
 * sgpr_md_pimd_info   out[count][64] = E[32] | covmax[32] per evaluation first ... first + count - 1 of the last sgpr_md_run
 *                     (0 = its first) among those that stand.
 * sgpr_md_fix, sgpr_md_thermostat, sgpr_md_barostat, sgpr_md_relax, sgpr_md_neb, sgpr_md_committee, sgpr_md_filter, sgpr_md_meta
 * and sgpr_md_record behind sgpr_md_pimd are refused. */
int sgpr_md_pimd(sgpr_model *h, int P, const double *positions, const double *velocities, double kT, double friction, double lambda);
int sgpr_md_pimd_state(sgpr_model *h, double *positions, double *velocities_pre, double *packed, int which);
int sgpr_md_pimd_info(sgpr_model *h, int first, int count, double *out);
/* Held atoms and components (after sgpr_md_begin; before sgpr_md_thermostat, sgpr_md_relax and the first sgpr_md_run):
 * fixed3N[N][3] in caller atom order, nonzero = that Cartesian component of that atom is held — all three of an atom for
 * ase.constraints.FixAtoms, the chosen ones for FixCartesian.  NULL or all zeros: nothing is held, and the run launches what a
 * run without this call launches.  Honoured inside the device loops — BAOAB Langevin, velocity Verlet, Nose-Hoover NVT (sharded
 * runs too), FIRE with and without a moving cell —, where a held component
 *   - is moved with F = 0: the forces the library REPORTS (packed results, sgpr_md_state) stay the model's own, and energy,
 *     virial and covloss are untouched;
 *   - has velocity exactly 0 from this call on (the value given to sgpr_md_begin is dropped), in the closing half kick of
 *     sgpr_md_velocities, in the Nose-Hoover centred velocity and in FIRE's velocity alike;
 *   - receives no Langevin noise: the device's deviates are counter-based on (seed; configuration, atom, component), so the
 *     free components draw exactly what they draw in a run without a mask; uploaded rows are read as before, held entries unused;
 *   - keeps its coordinate by selection, not by arithmetic that should cancel: at constant cell the bits uploaded by
 *     sgpr_md_begin for the whole run; in a relaxation with move_cell the undeformed coordinate r is what is held and
 *     x = r D^T follows the cell (FixAtoms inside UnitCellFilter).  The entries of G = F D of held components are zero in FIRE's
 *     three sums and in max |G_row|^2: convergence is judged on the free components; the cell rows are unchanged.
 * Degrees of freedom g = 3N - (held components).  With a non-empty mask sgpr_md_thermostat uses tfact = 2 / (g kT ttime^2) and
 * K0 = g kT / 2 — no centre-of-mass degree is removed, momentum is not conserved beside a held atom — and the conserved quantity
 * is E + KE + zeta^2 / tfact + 2 K0 int zeta dt, which is the expression above when nothing is held.  (The project's own
 * definition: ase.md.npt.NPT takes no constraints.)  scalars[.][12] / [13] are sums over all atoms as before: the temperature is
 * sum m v^2 / (g kB).
 * SGPR_E_INVALID: no run begun, a thermostat or a relaxation already set, a run that has started, every component held.
 * SGPR_E_UNSUPPORTED: from sgpr_md_barostat behind a non-empty mask (the moving-cell dynamics run without one).  The handle
 * goes on working after any of them. */
int sgpr_md_fix(sgpr_model *h, const uint8_t *fixed3N);
/* The frame record: a trajectory out of a run that is NOT cut for it.  The reference attaches its writers to the host loop
 * (theforce/cl/md.py:24-26: `loginterval`, default 1; :117-128 and :155-166: dyn.attach(traj.write, interval=loginterval)) and
 * its optimizers take trajectory= (theforce/cl/relax.py); each step there crosses into the calculator anyway.  Here a call of
 * sgpr_md_run stays on the device for all its evaluations, and sgpr_md_state shows only where it ended.
 *
 * sgpr_md_record       every >= 1: from the next sgpr_md_run on, the evaluation of every configuration n (index in the
 *                      trajectory) with n % every == 0 is followed by ONE extra launch that copies that configuration into a
 *                      record in device memory, in caller atom order; every = 0 switches recording off.  what: bit 0 the
 *                      velocities the integrator holds, bit 1 the packed results [F | beta | E | virial | overflow];
 *                      positions are always recorded.  A frame holds exactly what sgpr_md_state(which = -1) would return for
 *                      configuration n had the call ended with that evaluation — the same bits (Nose-Hoover / NPT:
 *                      velocities_pre of frame n is the centred v_(n-1); a relaxation: FIRE's velocity as it stands behind
 *                      the move out of n).  After sgpr_md_begin (which switches it off), between any two sgpr_md_run calls.
 *                      SGPR_E_INVALID: before sgpr_md_begin, every < 0, unknown bits.  SGPR_E_UNSUPPORTED: the run was begun
 *                      on more than one rank.  A run that records nothing launches exactly what it launched before.
 * sgpr_md_frame_count  frames of the LAST sgpr_md_run that stand: those of the evaluations whose results stand (*evals_done),
 *                      less the halting one when the covloss gate fired (halt code 1: the next call evaluates and records
 *                      that configuration again, with the model the caller has installed by then); a converged relaxation
 *                      (code 3) keeps the frame of its last evaluation.
 * sgpr_md_frames       frames first ... first + count - 1 of that record (valid until the next sgpr_md_run): index[count] the
 *                      trajectory indices, positions[count][N][3], velocities_pre[count][N][3], packed[count][4N + 11].  Any
 *                      pointer may be NULL; a non-NULL pointer for an array that was not recorded, or frames beyond
 *                      sgpr_md_frame_count: SGPR_E_INVALID.  One device-to-host copy per array.  Cell and strain rate (or D)
 *                      of the same evaluations: sgpr_md_cells.
 * The handle stays usable after every error above. */
int sgpr_md_record(sgpr_model *h, int every, int what);
int sgpr_md_frame_count(sgpr_model *h, int *count);
int sgpr_md_frames(sgpr_model *h, int first, int count, int64_t *index, double *positions, double *velocities_pre, double *packed);
/* Mean-square displacements accumulated inside the loop: what the reference computes from a stored trajectory
 * (theforce/analysis/analysis.py:109-176 `correlator`, :296-338 `diffusion_constants`) without the trajectory leaving the device.
 * Sample s is configuration n = s every.  Level l < levels has the lag 2^l samples and ONE origin O_l; at sample s every level
 * with s mod 2^l == 0 measures, if s >= 2^l, d_i = x_i - O_l,i (the positions of the run are never wrapped; a held component
 * has d = 0) and then sets O_l <- x.  With c = sum m_i d_i / sum m_i over all atoms (com = 1; else 0), per species z of the
 * model's table with n_z atoms in the frame, A = sum |d_i|^2 and B = sum d_i:
 *     msd = (A - 2 c.B + n_z |c|^2) / n_z  (= mean |d_i - c|^2),     smd = |B - n_z c|^2 / n_z
 * and the row (l, z) of the table gains msd, msd^2, smd, smd^2, count[l] gains 1.  The windows of a level do not overlap, so
 * sqrt(var / count) is an error bar.  A species absent from the frame keeps zeros.  Fixed summation order, no float atomics:
 * two runs give the same bits, however the run is cut into calls; a configuration evaluated twice (the repeat behind a covloss
 * halt or an overflow) counts once, the speculative evaluation behind a halt not at all.
 *
 * sgpr_md_msd       every >= 1, 1 <= levels <= 32, com 0 / 1: after sgpr_md_begin (and sgpr_md_fix, _thermostat, _filter, _meta,
 *                   _record, if used), before the first sgpr_md_run; zeroes the table.  every = 0 detaches and frees: the run
 *                   launches what it launched before.  Two small launches behind a sampled evaluation, levels x 3N doubles of device memory.
 *                   SGPR_E_INVALID: no run begun, a run that has started, values out of range.  SGPR_E_UNSUPPORTED: several
 *                   ranks, a barostat, a committee, a relaxation, a band, a polymer — and from sgpr_md_barostat, _committee,
 *                   _relax, _neb and _pimd on a run that has the accumulator.
 * sgpr_md_msd_read  between two calls of the run (synchronises the stream): table[levels][S][4] (S: the model's species),
 *                   counts[levels], info[2] = samples taken, the configuration the table waits for next.  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_msd(sgpr_model *h, int every, int levels, int com);
int sgpr_md_msd_read(sgpr_model *h, double *table, int64_t *counts, int64_t *info);
/* Radial distribution functions accumulated inside the loop: the pair-distance histograms the reference takes from a stored
 * trajectory (theforce/analysis/rdf.py `rdf`), as integers in device memory.  Behind the evaluation of every configuration n
 * with n % every == 0, for the species slots a, b of the model's table and k < bins, H[a][b][k] gains the number of triples
 * (i of species a, j of species b, s in Z^3) with (j, s) != (i, 0) — periodic self-images count — and
 *     d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),  r = sqrt((d0 d0 + d1 d1) + d2 d2),  rmin <= r < rmax,
 *     k = (int)(((r - rmin) / (rmax - rmin)) bins)     (a quotient that rounds up to `bins` stays in the last bin),
 * h0, h1, h2 the cell vectors, s = 0 along an open direction.  rmax may exceed the model's cutoff and half the cell: every
 * image within rmax is enumerated, up to two cells either way per direction.  Integer counts: the table is the same bits
 * however the atoms were wrapped and however the run is cut; a configuration evaluated twice (the repeat behind a covloss halt
 * or an overflow) counts once, the speculative evaluation behind a halt not at all.  g(r) is formed by the caller:
 *     g_ab(k) = H[a][b][k] / (samples n_a shell_k n_b / V).
 *
 * sgpr_md_rdf       every >= 1, 0 <= rmin < rmax, 1 <= bins <= 2048: after sgpr_md_begin (and sgpr_md_fix, _thermostat, _filter,
 *                   _meta, _record, _msd, if used), before the first sgpr_md_run; zeroes the table.  every = 0 detaches and
 *                   frees the table: the run launches what it launched before.  Two launches behind a sampled evaluation, one
 *                   workgroup per pair of 128-atom tiles: O(N^2) per sample.  SGPR_E_INVALID: no run begun, a run that has
 *                   started, values out of range, a cell without volume, atoms not sorted by the model's species.
 *                   SGPR_E_UNSUPPORTED: rmax beyond 2.5 heights of the cell along a periodic direction (the message names the
 *                   height), several ranks, a barostat, a committee, a relaxation, a band, a polymer — and from
 *                   sgpr_md_barostat, _committee, _relax, _neb and _pimd on a run that has the accumulator.
 * sgpr_md_rdf_read  between two calls of the run (synchronises the stream): hist[S][S][bins] (S: the model's species; symmetric,
 *                   filled out), info[4 + S] = samples taken, the configuration the table waits for next, bins, S, the atoms
 *                   of every species in the frame; geom[3] = the volume |det cell|, rmin, rmax (bin k is
 *                   [rmin + k w, rmin + (k + 1) w), w = (rmax - rmin) / bins).  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_rdf(sgpr_model *h, int every, double rmin, double rmax, int bins);
int sgpr_md_rdf_read(sgpr_model *h, uint64_t *hist, int64_t *info, double *geom);
/* Velocity autocorrelations accumulated inside the loop.  The reference has none (theforce/analysis correlates displacements
 * only): the definition is this library's, workloads.VacfRing is its host twin, and the device equals the twin bit for bit.
 * Sample s is configuration n = s every; its velocity v(s) is the one sgpr_md_velocities returns had the call ended with that
 * evaluation (Langevin / velocity Verlet: v_pre + (dt/2) F / m with the evaluation's packed force, v_pre at n = 0; Nose-Hoover:
 * the centred velocity; a held component exactly 0).  For every sample s, lag k < lags and origin o = s - k >= 0 with
 * o mod origin_every == 0, per species z of the model's table (n_z atoms), J_z = sum_z v_i, c = sum m_i v_i / sum m_i (com = 1;
 * else 0):
 *     tracer[k][z]        += mean over z of (v_i(s) - c_s).(v_i(o) - c_o)
 *     collective[k][a][b] += e_a(s).e_b(o),  e_z = J_z - n_z c         (not symmetric at k > 0: the full block is kept)
 *     counts[k]           += 1
 * Fixed summation order, no float atomics.  v(s) depends on the forces, and a configuration behind a covloss halt is evaluated
 * again with the updated model: a sample is STORED behind every evaluation of its configuration (the repeat overwrites it) and
 * CORRELATED once, when the next sample arrives — so the last stored sample of a run is pending, and counts once the run goes on.
 *
 * sgpr_md_vacf       every >= 1, lags >= 1, origin_every >= 1, com 0 / 1: after sgpr_md_begin (and sgpr_md_fix, _thermostat,
 *                    _record, _msd, _rdf, if used), before the first sgpr_md_run; zeroes the tables.  every = 0 detaches and
 *                    frees: the run launches what it launched before.  Four small launches behind a sampled evaluation; device
 *                    memory: a ring of (lags + 1) x 24 N bytes.  SGPR_E_INVALID: no run begun, a run that has started, values out
 *                    of range.  SGPR_E_UNSUPPORTED: more than 8192 lags or a ring over 4 GiB; several ranks, a barostat, a
 *                    committee, a relaxation, a band, a polymer; the filter and a bias (their closing kick uses a force other than
 *                    the packed one) — and from sgpr_md_barostat, _committee, _relax, _neb, _pimd, _filter and _meta on a run that
 *                    has the accumulator.
 * sgpr_md_vacf_read  between two calls of the run (synchronises the stream): tracer[lags][S], collective[lags][S][S] (S: the
 *                    model's species), counts[lags], info[3 + S] = samples correlated, pending (0 / 1), the configuration the
 *                    table waits for next, the atoms of every species in the frame.  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_vacf(sgpr_model *h, int every, int lags, int origin_every, int com);
int sgpr_md_vacf_read(sgpr_model *h, double *tracer, double *collective, int64_t *counts, int64_t *info);
/* Van Hove correlation functions accumulated inside the loop, as integers in device memory.  The self part is the histogram the
 * reference takes from a stored trajectory at one lag (theforce/analysis/analysis.py:178-210 `hist_rtp_displacements`); the
 * reference has no distinct part.  workloads.VanHoveCounts is the host twin and the definition; the device equals it exactly.
 * Samples and levels are sgpr_md_msd's: sample s is configuration n = s every, level l < levels has the lag 2^l samples and ONE
 * origin O_l; at sample s every level with s mod 2^l == 0 measures, if s >= 2^l (counts[l] += 1), and then sets O_l <- x.
 * Self, atom i of species slot z: d = x_i - O_l,i (raw: no centre of mass is taken out), q = d0 d0 + d1 d1, r = sqrt(q + d2 d2).
 *     r >= rmax: over[l][z] += 1.   r == 0 (a held atom): bin (0, 0, pbins / 2), where atan2(0, 0) = 0 lands.   Else
 *     kr = min((int)((r / rmax) rbins), rbins - 1)
 *     kt = the number of k in 1 ... tbins - 1 with d2 <= ct[k] r,              ct[k] = cos(k pi / tbins)
 *     kp = the number of k in 1 ... pbins - 1 that pass, (cu, su)[k] = (cos, sin)(-pi + 2 pi k / pbins), c = cu[k] d1 - su[k] d0:
 *          2k < pbins: d1 >= 0 or c >= 0;   2k == pbins: d1 >= 0;   2k > pbins: d1 >= 0 and c >= 0
 * and self_hist[l][z][kr][kt][kp] += 1: np.histogramdd over linspace(0, rmax), linspace(0, pi), linspace(-pi, pi) without an acos
 * or atan2 deciding a bin.  self_hist[l][z] summed plus over[l][z] equals n_z counts[l].
 * Distinct (dbins > 0): distinct_hist[l][a][b][k] gains the triples (i of a, j of b, s in Z^3) with (j, s) != (i, 0) and
 *     d = (x_j - O_l,i) + ((s0 h0 + s1 h1) + s2 h2),  0 <= r < dmax,  k = min((int)((r / dmax) dbins), dbins - 1)
 * by sgpr_md_rdf's enumeration (nearest image by rounding, then the block of shifts that can come within dmax).  Origin and
 * present are not interchangeable: the table is the full S x S.  A frozen trajectory gives sgpr_md_rdf's table per window.
 * A configuration evaluated twice (the repeat behind a covloss halt or an overflow) counts once, the speculative evaluation
 * behind a halt not at all.
 *
 * sgpr_md_vanhove        every >= 1, 1 <= levels <= 32, rmax > 0, 1 <= rbins <= 2048, 1 <= tbins, pbins <= 64, 0 <= dbins <= 2048
 *                        (0: no distinct part; dmax is then ignored): after sgpr_md_begin (and sgpr_md_fix, _thermostat, _filter,
 *                        _meta, _record, _msd, _rdf, _vacf, if used), before the first sgpr_md_run; zeroes the tables.  every = 0
 *                        detaches and frees: the run launches what it launched before.  At most three launches behind a sampled
 *                        evaluation; the distinct part is O(N^2) per due level.  SGPR_E_INVALID: no run begun, a run that has
 *                        started, values out of range, a cell without volume with dbins > 0.  SGPR_E_UNSUPPORTED: a self table
 *                        levels S rbins tbins pbins 8 B over 1 GiB, dmax beyond 2.5 heights of the cell along a periodic
 *                        direction, several ranks, a barostat, a committee, a relaxation, a band, a polymer — and from
 *                        sgpr_md_barostat, _committee, _relax, _neb and _pimd on a run that has the accumulator.
 * sgpr_md_vanhove_edges  replaces the tables ct[tbins], cu[pbins], su[pbins] the attach made with this library's cos and sin by
 *                        the caller's, so that a host twin compares with the same doubles.  Before the first sgpr_md_run.
 * sgpr_md_vanhove_read   between two calls of the run (synchronises the stream): self_hist[levels][S][rbins][tbins][pbins],
 *                        over[levels][S], distinct_hist[levels][S][S][dbins], counts[levels], info[8 + S] = samples taken, the
 *                        configuration the tables wait for next, levels, S, rbins, tbins, pbins, dbins, the atoms of every
 *                        species in the frame; geom[3] = the volume |det cell| (0: none), rmax, dmax.  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_vanhove(sgpr_model *h, int every, int levels, double rmax, int rbins, int tbins, int pbins, double dmax, int dbins);
int sgpr_md_vanhove_edges(sgpr_model *h, const double *ct, const double *cu, const double *su);
int sgpr_md_vanhove_read(sgpr_model *h, uint64_t *self_hist, uint64_t *over, uint64_t *distinct_hist, int64_t *counts, int64_t *info,
                         double *geom);
/* Bond-angle and coordination distributions accumulated inside the loop: the three-body structure of the run (is a tetrahedron
 * intact, which corners do two share, how many neighbours sit around an ion), as integers in device memory.  The reference has
 * no angular analysis; workloads.AdfCounts is the definition.  cut[S][S] is a symmetric table of bond cutoffs over the species
 * slots of the model's table (0: the pair never bonds).  Behind the evaluation of every configuration n with n % every == 0, for
 * every centre i of species a, its neighbours are all (j of species b, s in Z^3) with (j, s) != (i, 0) and
 *     d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),  r = sqrt((d0 d0 + d1 d1) + d2 d2),  r < cut[a][b]
 * (s = 0 along an open direction; periodic self-images and several images of one atom are distinct neighbours).  For every
 * unordered pair {t, t'} of them, with species b <= c after ordering,
 *     q = (d_t0 d_t'0 + d_t1 d_t'1) + d_t2 d_t'2,  p = r_t r_t',  k = the number of e in 1 ... bins - 1 with q <= ct[e] p,
 * and angles[a][b][c][k] gains 1: bin k holds the angles in [k pi / bins, (k + 1) pi / bins), decided by comparisons with the
 * caller's ct[e] = cos(e pi / bins), never by acos.  With n_ib the neighbours of species b, coord[a][b][min(n_ib, 63)] gains 1.
 * The neighbours are read from the neighbour list the step has just built: the cost is linear in the number of atoms.  Integer
 * counts: the tables are the same bits however the run is cut; a configuration evaluated twice (the repeat behind a covloss halt
 * or an overflow) counts once — behind an overflow (halt code 2: its list was clamped) the repeat is the one that counts —, the
 * speculative evaluation behind a halt not at all.
 *
 * sgpr_md_adf       every >= 1, 1 <= bins <= 1024, cut[S * S], ct[bins] (entry 0 is never compared): after sgpr_md_begin (and
 *                   sgpr_md_fix, _thermostat, _filter, _meta, _record, _msd, _rdf, _vacf, _vanhove, if used), before the first
 *                   sgpr_md_run; zeroes the tables.  every = 0 detaches and frees them: the run launches what it launched
 *                   before.  Two launches behind a sampled evaluation.  SGPR_E_INVALID: no run begun, a run that has started,
 *                   values out of range, a table that is asymmetric, negative or all zero, edges that increase, atoms not
 *                   sorted by the model's species.  SGPR_E_UNSUPPORTED: a cutoff above the model's rc (the list holds nothing
 *                   beyond it), several ranks, a barostat, a committee, a relaxation, a band, a polymer — and from
 *                   sgpr_md_barostat, _committee, _relax, _neb and _pimd on a run that has the accumulator.  sgpr_md_run
 *                   answers SGPR_E_UNSUPPORTED for a step form that does not end in the gather form of the fused last kernel
 *                   (the forms a qlvar bias refuses) and for a neighbour list so long that one centre's neighbours do not fit
 *                   the LDS of a workgroup.
 * sgpr_md_adf_read  between two calls of the run (synchronises the stream): angles[S][S][S][bins] (symmetric in the two ends,
 *                   filled out), coord[S][S][64], info[4 + S] = samples taken, the configuration the tables wait for next, bins,
 *                   S, the atoms of every species in the frame.  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_adf(sgpr_model *h, int every, int bins, const double *cut, const double *ct);
int sgpr_md_adf_read(sgpr_model *h, uint64_t *angles, uint64_t *coord, int64_t *info);
/* Partial static structure factors S_ab(q) and coherent intermediate scattering functions F_ab(q, t) accumulated inside the loop:
 * the run in reciprocal space — what diffraction measures, Bragg and diffuse scattering, collective density fluctuations in time.
 * The reference has nothing of the kind; workloads.SqRing is the definition and the host twin.  Wave vectors are vectors of the
 * reciprocal lattice of the run's constant cell, q_j = 2 pi hkl_j inv(cell)^T, so that q_j . r = 2 pi hkl_j . s with s = r inv(cell):
 * wrapped and unwrapped positions give the same phases.  Sample s is configuration n = s every.  Per atom f = s - rint(s) per axis,
 * e_a = exp(2 pi i f_a), and per species z of the model's table
 *     rho_z(q_j; s) = sum over the atoms of z of e_0^h e_1^k e_2^l          (a negative index: the conjugate of the positive power)
 * For every lag k < lags and origin o = s - k >= 0 with o mod origin_every == 0
 *     f[k][j][a][b] += Re(rho_a(q_j; s) conj rho_b(q_j; o)),  count[k] += 1  (not symmetric in a, b at k > 0: the full block is kept)
 * and per sample mean[j][a] += rho_a(q_j; s) (complex: |<rho>|^2 is the Bragg part), samples += 1.  Lag 0 is the static S_ab.  The
 * caller passes one vector of each +- pair (the real part is the average over the pair); duplicates are not checked for.
 * Fixed summation order, no float atomics: two runs give the same bits, however they are cut.  Against the twin the device is held
 * to a bound, not bit for bit (its sincospi is not numpy's): |d rho_z| <= B_z = 128 hmax (1 + smax) n_z 2^-52 with hmax the largest
 * |index| and smax the largest |scaled coordinate|, |d f[k][j][a][b]| <= count[k] (n_a B_b + n_b B_a + count[k] n_a n_b 2^-52);
 * count, samples and next_due are equal.  The positions of a configuration do not depend on the model: a configuration evaluated
 * twice (the repeat behind a covloss halt or an overflow) counts once, at its first evaluation; the speculative evaluation behind a
 * halt not at all.  Nothing is left pending.
 *
 * sgpr_md_sq       every >= 1, 1 <= nq <= 8192, hkl[nq][3] with no zero row, every |index| <= 32 and 0 along a direction that is
 *                  not periodic, 1 <= lags <= 8192, origin_every >= 1: after sgpr_md_begin (and sgpr_md_fix, _thermostat, _filter,
 *                  _meta, _record and the other accumulators, if used), before the first sgpr_md_run; zeroes the tables.  every = 0
 *                  detaches and frees them: the run launches what it launched before.  Three launches behind a sampled evaluation:
 *                  N nq complex phase products per sample from three sincos per atom; lags nq S^2 doubles of f are updated per
 *                  sample (origin_every thins them).  SGPR_E_INVALID: no run begun, a run that has started, values out of range
 *                  (these come first), a cell without volume, atoms not sorted by the model's species.  SGPR_E_UNSUPPORTED: f and
 *                  the ring, lags nq S (8 S + 16) bytes, over 1 GiB; several ranks, a barostat, a committee, a relaxation, a band,
 *                  a polymer — and from sgpr_md_barostat, _committee, _relax, _neb and _pimd on a run that has the accumulator.
 * sgpr_md_sq_read  between two calls of the run (synchronises the stream): f[lags][nq][S][S], mean[nq][S][2] (real, imaginary),
 *                  count[lags], info[2 + S] = samples taken, the configuration the tables wait for next, the atoms of every species
 *                  in the frame.  Any pointer may be NULL.
 * The handle stays usable after every error above. */
int sgpr_md_sq(sgpr_model *h, int every, int nq, const int32_t *hkl, int lags, int origin_every);
int sgpr_md_sq_read(sgpr_model *h, double *f, double *mean, int64_t *count, int64_t *info);
/* The Bayesian committee inside the device MD loop: the reference combines frozen sub-models and the live one per step on the
 * host (theforce/calculator/active_bcm.py:589-633, get_covloss_total :885-894); here every evaluation of sgpr_md_run evaluates
 * the K members and the live handle h at the same positions and combines them on the device, members k = 0 ... K - 1 in the
 * order given, h last (k = K):
 *     covmax_k = max_i beta_k(i),  b_k = -ln(covmax_k) if covmax_k < 1 else 0,  s_k = b_k / covmax_k  (covmax_k = 0: +inf)
 *     any s_k infinite: w_k = 1 where it is, 0 elsewhere;   sum_k s_k <= 0: w = e_K;   then w <- w / sum_k w_k
 *     E, every force component and the nine virial entries: sum_k w_k (.)_k in member order, without contraction
 *     beta_tot(i) = min_k beta_k(i): the covloss sgpr_md_state reports; max_i beta_tot(i) is what `ediff` gates (scalar 11)
 * Fixed summation order, no float atomics: two runs give the same bits.  The covloss gate and a capacity overflow of ANY member
 * halt the run at the evaluation itself, before anything moves.  The rows of scalars keep their layout.
 *
 * sgpr_md_committee       after sgpr_md_begin and, if used, sgpr_md_thermostat, before the first sgpr_md_run.  K = 0 or
 *                         members = NULL detaches: the run is the one without this call and launches what it launched before.
 *                         The members are BORROWED: the caller keeps them alive until sgpr_md_end, the next sgpr_md_begin or a
 *                         detach (each lets them go), and may use them between two sgpr_md_run calls (every call binds them to the run's system
 *                         again and repeats the capacity-checked pass where needed).  Langevin with uploaded or counter-based
 *                         deviates, velocity Verlet, Nose-Hoover NVT, and — with the run's option
 *                         "md_committee_cell" set first — Nose-Hoover with a barostat (sgpr_md_barostat before
 *                         or after this call: the members are evaluated in the moving cell, whose strain rate follows the
 *                         committee's stress; sgpr_md_cells and sgpr_md_state as for a single model).  SGPR_E_UNSUPPORTED: a
 *                         barostat without that option, a
 *                         relaxation, a band, a filter, a bias, held components, an armed frame record (and sgpr_md_record,
 *                         sgpr_md_fix, sgpr_md_filter, sgpr_md_meta, sgpr_md_relax behind an attached committee) — with or
 *                         without a barostat —, a run begun on more than one rank, a member on another
 *                         device, K > 15.  SGPR_E_INVALID: a member that is h itself, a null or duplicate member, a member
 *                         without weights or without choli, a run that has started (a detach too: a started run keeps
 *                         what it has), and sgpr_md_thermostat behind an attached committee.
 * sgpr_md_committee_info  w[K + 1] and covmax[K + 1] (either may be NULL) of the last evaluation whose results stand — after a
 *                         halted or `final` call the numbers behind the packed results sgpr_md_state returns.  SGPR_E_INVALID
 *                         without a committee or before an evaluation stands.
 * The handle stays usable after every error above. */
int sgpr_md_committee(sgpr_model *h, int K, sgpr_model *const *members);
int sgpr_md_committee_info(sgpr_model *h, double *w, double *covmax);
/* The filter of model-update jumps inside the device MD loop: the reference's MD driver wraps the atoms in FilterDeltas by
 * default (theforce/cl/md.py:76-79, ml_filter = 0.8; theforce/calculator/active.py:47-76): the jumps `deltas` = results after -
 * results before that an on-the-fly update puts into forces and stress are summed, the sum is shrunk at every force or stress
 * call and subtracted — the force part clamped to +-1 eV/A — from what the integrator sees.  Here, by evaluation index, once per
 * configuration n, inside the step's last kernel and (stress, moving cell only) the barostat's launch:
 *     A_f <- (A_f + dF_n) shrink,   F_seen = F_model - min(max(A_f, -1), 1)     (a held component, sgpr_md_fix, then sees 0)
 *     A_s <- (A_s + dS_n) shrink,   stress_seen = stress_model - A_s
 * in this order, without contraction.  Everything the run REPORTS (packed results, sgpr_md_state, the frame record, the rows of
 * scalars) stays the model's own.  The accumulators live in rings indexed like the positions: an evaluation that a halt discards
 * leaves those of its configuration as they were.  A filtered run launches as many kernels as the run without a filter.
 *
 * sgpr_md_filter        after sgpr_md_begin (and sgpr_md_fix, sgpr_md_thermostat, sgpr_md_barostat), before the first
 *                       sgpr_md_run.  0 < shrink < 1.  f0[3N] (caller atom order) and s0[6] (Voigt): the accumulators of
 *                       configuration 0, NULL: zeros.  SGPR_E_UNSUPPORTED: a relaxation, a run with a committee, a run begun on
 *                       more than one rank (and sgpr_md_relax, sgpr_md_committee behind a filter; sgpr_md_run where the step
 *                       is not the single-rank gather form).  SGPR_E_INVALID: shrink outside (0, 1), a run that has started.
 *                       sgpr_md_begin switches the filter off.
 * sgpr_md_filter_push   between two sgpr_md_run calls: dF[3N] (caller atom order; NULL: none) and dS[6] (NULL: none; ignored at
 *                       constant cell, where nobody asks for a stress) are added into the accumulators of the current
 *                       configuration — the `deltas` of the calculate() a halt led to, before the evaluation is repeated.
 * sgpr_md_filter_state  f[3N], s[6] (either may be NULL): the accumulators of the current configuration, what its evaluation
 *                       will shrink and apply — and what sgpr_md_filter takes to continue in another run. */
int sgpr_md_filter(sgpr_model *h, double shrink, const double *f0, const double *s0);
int sgpr_md_filter_push(sgpr_model *h, const double *dF, const double *dS);
int sgpr_md_filter_state(sgpr_model *h, double *f, double *s);
/* Metadynamics inside the device MD loop: the bias potential of the reference's theforce/calculator/meta.py (Meta over
 * theforce/analysis/kde.py's Gaussian_kde; examples/meta-dyn/md.py), one small launch per configuration between the reverse
 * descriptor pass and the step's last kernel.  Collective variables from the raw coordinates the integrator holds (no minimum
 * image), concatenated, D <= 6 dimensions over at most 4 components: distance(i, j) = |x_j - x_i|; posvar(index, select) =
 * x_index - (1/n) sum over the atoms k != index of `select` (all atoms, or one species) of x_k, with n counting the index atom
 * where it is of that species (the reference's Posvar).  A hill deposited at c is centred at (floor(c / sigma) + 0.5) sigma
 * and is summed at x when floor(c / (5 sigma)) and floor(x / (5 sigma)) differ by at most one in every dimension;
 * kde = sum exp(-|(x - centre) / sigma|^2 / 2) / (2 pi)^(D/2); V = w kde, or log(1 + w kde / kT) kT (well-tempered).  The bias of
 * configuration n sums the hills of the configurations below n; configuration n deposits when n % pace == 0.  Energy, forces
 * and virial of everything the run reports and integrates include the bias; the covloss gate does not see it.  Hills are rows
 * indexed by configuration: what a halt discards or a cut repeats overwrites its own row.
 *
 * sgpr_md_meta        after sgpr_md_begin, between any two sgpr_md_run calls.  cvs[ncomp][3] = kind (0 distance, 1 posvar, 2 qlvar), atom
 *                     (i | index), second (j | select: an atomic number, -1: all atoms | Zj), caller atom order; sigma[D]; w; kT > 0:
 *                     well-tempered, 0: plain; pace >= 1; capacity: rows of hills; nhills rows hills_cv[nhills][D] and
 *                     hills_V[nhills] (NULL: zeros) stand from the start, for the deposits of the configurations below the
 *                     current one (a restart; the rows of sgpr_md_meta_hills when a run needs more room).  ncomp = 0 detaches.
 *                     SGPR_E_UNSUPPORTED, each naming the host loop around calculate(): a barostat, a relaxation, a nudged
 *                     elastic band, a committee, a run begun on several ranks (and those calls behind a bias; sgpr_md_run
 *                     where the step cannot take the single-rank gather form of the fused last kernel — graph replay, the
 *                     side-stream fork, a zero skin, the scatter form: refused before anything is enqueued; lists that outgrow the
 *                     gather form inside a call: at that evaluation).  sgpr_md_run refuses with SGPR_E_INVALID, before it
 *                     enqueues anything, a call whose deposits would pass the capacity.  A CV further than 1e9 blocks of 5 sigma
 *                     from the origin is beyond the scheme (keys are clamped there).  sgpr_md_begin detaches.
 * sgpr_md_meta_info   D; below: the hills below the current configuration (those given and the deposits of the configurations
 *                     before it: what sgpr_md_meta takes to go on from here); held: those and the current configuration's own
 *                     row after a halted or `final` call (not behind a fresh sgpr_md_meta: the row is written when the run goes
 *                     on); the capacity.  Any of them NULL.
 * sgpr_md_meta_hills  rows first ... first + count - 1 of the hills that stand: cv[count][D], V[count] (the bias the depositing
 *                     configuration saw); either NULL.
 * sgpr_md_meta_merge  the merged form: after sgpr_md_meta and before the next sgpr_md_run (otherwise SGPR_E_INVALID; so is a
 *                     negative chunk).  The rows are kept as before, and chunk j — the rows [j chunk, (j + 1) chunk) — is merged
 *                     into a table of one entry per occupied bin (the reference's Gaussian_kde keeps a counter per bin) in front
 *                     of the bias of the first configuration with (hills below it) / chunk > j; a configuration with nh hills
 *                     below it sums the entries of the rows [0, (nh / chunk) chunk) — count times the hill of the entry's centre —
 *                     and then the rows behind them one by one: a function of the configuration and the rows below it, whatever
 *                     the cuts and halts.  The cost of the bias then grows with the bins visited, not with time.  The chunks of
 *                     the uploaded hills are merged in this call: a run that goes on from sgpr_md_meta_hills with the same chunk
 *                     has the bits of the uninterrupted one.  chunk = 0: every hill on its own again.  sgpr_md_meta switches
 *                     merging off.  Not bit-compatible with the unmerged sum (the same terms in another order).
 * sgpr_md_meta_table  the table as the current configuration sees it (Gaussian_kde.histogram()): *n_entries entries in the order
 *                     of the first row that occupied each, centres[*n_entries][D], counts[*n_entries], from the first
 *                     *rows_merged rows.  Any of them NULL: ask for *n_entries first (at most the capacity).
 * sgpr_md_meta_ql     stages the parameters of component `comp` of the NEXT sgpr_md_meta, whose cvs triple (2, index, Zj) consumes
 *                     them (taken and cleared by that call, whether it succeeds or not): kind 2, the Steinhardt bond-order
 *                     parameters Q_l of atom `index` over its neighbours t of species Zj with r_t < cutoff in the step's own
 *                     neighbour list (r_t = x_j - x_index + shift.cell), weights w_t = (1 - r_t / cutoff)^2, W = sum w_t,
 *                     Q_l^2 = sum_{t,t'} w_t w_t' P_l(r^_t . r^_t') / W^2: one dimension per l[k], 0 <= l <= 12, 1 <= n_l <= 6, in
 *                     the order given.  0 < cutoff <= rc (the list ends at rc, where the weight is not zero).  An empty environment
 *                     gives Q_l = 0 and no force; so does Q_l = 0.  The virial is sum_t r_t (x) dV/dr_t over the images.
 *                     SGPR_E_INVALID from sgpr_md_meta: a kind-2 component without staged parameters, a species no atom has;
 *                     SGPR_E_UNSUPPORTED, there or from sgpr_md_run: (kind-2 components) x (list entries per atom) > 256.
 * sgpr_md_end releases the hills. */
int sgpr_md_meta_ql(sgpr_model *h, int comp, double cutoff, int n_l, const int32_t *l);
int sgpr_md_meta(sgpr_model *h, int ncomp, const int32_t *cvs, const double *sigma, double w, double kT, int pace, int64_t capacity,
                 int64_t nhills, const double *hills_cv, const double *hills_V);
int sgpr_md_meta_info(sgpr_model *h, int *D, int64_t *below, int64_t *held, int64_t *capacity);
int sgpr_md_meta_hills(sgpr_model *h, int64_t first, int64_t count, double *cv, double *V);
int sgpr_md_meta_merge(sgpr_model *h, int64_t chunk);
int sgpr_md_meta_table(sgpr_model *h, double *centres, double *counts, int64_t *n_entries, int64_t *rows_merged);
/*
 * Multi-GPU (one process per GPU, atoms sharded as in sgpr_bind_system): the reference combines the
 * ranks' partial sums with four MPI all-reduces per step (calculator/active.py:562,601,602,777,
 * util/parallel.py); here ONE RCCL all-reduce of the packed buffer over xGMI, issued by the library
 * on the step's stream.  Rank 0 creates the id (SGPR_COMM_ID_BYTES bytes), the host passes it to the
 * other ranks by any means (MPI, a TCP store, a file), and every rank calls sgpr_comm_init
 * (collective).  Without a communicator the caller combines the partial sums itself.
 * sgpr_comm_allreduce: in-place SUM (op_max = 0) or MAX (1) of a device buffer of doubles over the
 * same communicator (barriers, max-over-ranks timings).
 */
#define SGPR_COMM_ID_BYTES 128
int sgpr_comm_unique_id(void *id_out);
int sgpr_comm_init(sgpr_model *h, const void *id, int rank, int world);
int sgpr_comm_destroy(sgpr_model *h);
int sgpr_comm_allreduce(sgpr_model *h, double *buf_dev, int64_t count, int op_max, void *stream);

/*
 * The library's own exchange between the ranks of ONE node — an alternative to RCCL that also runs when several ranks
 * share one device (RCCL refuses that) and that gives every rank the SAME bits: every rank owns a receive buffer with
 * one slice per source rank, exported through hipIpcGetMemHandle; a step's partial sums are pushed into the slice of every
 * peer (one hop on the fully connected xGMI mesh: the all-gather BASELINE.json words, the zero-padded all-reduces of
 * calculator/active.py:770-777), released by one flag store per peer, and summed locally in rank order.  The force sums of
 * the sharded reverse pass travel as fixed-point integers and are added as integers: the total force on an atom is the same
 * bits for every number of ranks.
 *   sgpr_peer_export   allocates this rank's buffers for `world` ranks and `capacity` doubles per slice (a sharded step of N
 *                      atoms needs 3 N + 4 ceil(N / world) + 11; 7 N + 11 serves every world size) and writes
 *                      SGPR_PEER_HANDLE_BYTES bytes for the peers
 *   sgpr_peer_attach   handles[world][SGPR_PEER_HANDLE_BYTES] of all ranks in rank order (the host passes them by any means);
 *                      from then on sgpr_compute / sgpr_step_dev / sgpr_step_dev_next combine a sharded step through this
 *                      exchange (preferred over a communicator of sgpr_comm_init), sgpr_comm_allreduce works over it, and
 *                      sgpr_md_begin / sgpr_md_run run SHARDED: every rank evaluates its share, and after the exchange
 *                      integrates all atoms from the summed forces (the deviates are counter-based or uploaded alike), so the
 *                      ranks' states stay identical; the covloss gate and capacity overflows halt every rank at the same step.
 * A peer that never arrives is a time-out (SGPR_PEER_TIMEOUT_MS, default 30000: a rank's first sharded step may grow
 * capacities and load code objects while its peers already wait), not a hang: the consumer of a timed-out exchange marks the
 * step's results (poison in the overflow word; NaN in a buffer of sgpr_comm_allreduce), so the call that reads them —
 * sgpr_compute / sgpr_compute_view on their warm path included, sgpr_sync_check, sgpr_md_run — fails with the time-out's
 * message.  A time-out is permanent: every later exchange of the handle fails at once until sgpr_peer_export + sgpr_peer_attach
 * have been called again on every rank.  Exchanges are collective: every rank issues the same sequence of them, one after
 * the other (an exchange issued on another stream than the one before is ordered behind it).
 */
#define SGPR_PEER_HANDLE_BYTES 128
int sgpr_peer_export(sgpr_model *h, int rank, int world, int64_t capacity, void *handle_out);
int sgpr_peer_attach(sgpr_model *h, const void *handles);
int sgpr_peer_destroy(sgpr_model *h);

/* Synchronise `stream` (NULL = the handle's own) and verify that no step since the last
 * check overflowed the neighbour-list capacity.  Returns SGPR_E_OVERFLOW if one did (those
 * steps' results are invalid; capacity has been grown, the next step re-sizes eagerly). */
int sgpr_sync_check(sgpr_model *h, void *stream);
/* Options:
 *  "graph" = 0/1            replay sgpr_step_dev from a captured HIP graph (default 0: eager launches pipeline
 *                           well while a step is ~100 us of kernels and measured faster than replay)
 *  "qr_keep" = 1/0/2        the first-stage factorisation of sgpr_data_solve is kept with its reflectors, so that
 *                           an appended / popped inducing LCE and a pushed frame update it instead of refactoring
 *                           (default 1; 0: every refit factors from scratch, as the reference does,
 *                           gppotential.py:745-791; 2: both, the difference of mu printed on stderr).  The
 *                           environment variable SGPR_QR_KEEP sets the initial value.
 *  "skin_milliangstrom"     Verlet skin of the neighbour candidates (default 500 = 0.5 A).  The reference asks ASE
 *                           for a list with skin 0 at every step (descriptor/atoms.py:349-355); here candidate
 *                           lists of |r| < rc + skin are kept and rebuilt ON THE DEVICE whenever an atom's
 *                           displacement since the last build — measured against the affine image of its build-time
 *                           position when the cell has changed (NPT: cl/md.py:147-150) — exceeds
 *                           (sigma_min(h0^-1 h) (rc + skin) - rc) / 2 (= skin/2 at constant cell), and every step
 *                           filters them to |r| < rc: the same pairs in the same order as a from-scratch list, bit
 *                           for bit.  0 = rebuild every step
 *  "ignore_unknown_species" = 0/1  atoms and LCE neighbours outside the species table are invisible
 *                           (descriptor/sesoap.py:343-346) instead of SGPR_E_SPECIES
 *  "overlap" = 0/1          covloss product on a side stream (measured slower; default 0)
 *  "cov_in_rev" = 0/1       covloss tiles in the reverse kernel's launch instead of grouped with the W product
 *                           (measured slower at 4096 atoms: default 0).  Environment: SGPR_COV_IN_REV
 *  "zero_copy_out" = 1/0    single-rank sgpr_compute: the step's last kernel writes its results into mapped
 *                           page-locked host memory instead of a device buffer that is copied back (default 1).
 *                           Environment: SGPR_ZERO_COPY
 *  "lone_atom_weight" = k   k(x, x') of two lone atoms (no neighbour inside the cutoff) of one species: the
 *                           reference adds that term once per kernel OBJECT (similarity/similarity.py:38-40, :94-103)
 *                           and sums its kernels (regression/gppotential.py:63-84) — 1 for the wildcard kernel
 *                           (default), S for the list of S fixed-species kernels of calculator/active.py:31-38.
 *                           Set before the inducing set.
 *  "fuse_next" = 1/0        the last kernel of a step may open the next one (sgpr_step_dev_next, sgpr_md_run;
 *                           default 1; 0: every step bins for itself — sgpr_md_run then returns SGPR_E_UNSUPPORTED).
 *                           Environment: SGPR_FUSE_NEXT
 *  "gemm_fused" = 1/0       K_nm, W and covloss of a step in ONE launch (consumer tiles wait on per-panel counters;
 *                           same bits, measured slower at 4096 atoms: default 0).  Environment: SGPR_GEMM_FUSED
 *  "reverse_scatter" = 0/1  the scatter form of the reverse pass (fixed-point force sums; what sharded frames use) on a
 *                           single rank too: the twin a sharded run is compared with bit for bit (default 0: gather form)
 *  "spin_wait" = 1/0        sgpr_compute polls its stream for the end of a step instead of a blocking wait
 *                           (default 1: one host thread spins for the ~0.1 ms of a step, 16 us less wall time per
 *                           call on a 4096-atom frame; 0: hipStreamSynchronize).  Environment: SGPR_SPIN_WAIT
 *  "md_committee_cell" = 0/1  of the RUN begun by sgpr_md_begin (which switches it off again; SGPR_E_INVALID without a run
 *                           or on one that has started): 1 lets a committee and a barostat meet on the run —
 *                           sgpr_md_committee accepts a run with a barostat, sgpr_md_barostat a run with a committee, and
 *                           sgpr_md_run integrates the committee in the moving cell.  0 (default): each refuses the other. */
int sgpr_set_option(sgpr_model *h, const char *name, int value);
/* How many times the neighbour candidates were rebuilt since sgpr_create (see "skin_milliangstrom"). */
int sgpr_get_list_rebuilds(sgpr_model *h, int64_t *count);
/* stress[6] (Voigt, eV/A^3) from a (summed) packed buffer on the host:
 * calculator/active.py:604-610, volume = |det cell| or -2 for a rank-deficient cell. */
int sgpr_stress_from_virial(const double *virial9, const double *cell, double *stress6);

/* Inspection/test exports for the last sgpr_compute / sgpr_step_dev on this handle.
 * p: dense p-hat [N][S][S][D] in the reference layout (see sgpr_get_inducing_descriptors).
 * nl: neighbour list in CSR form; call with j == NULL to get only ptr[N+1]. */
int sgpr_get_descriptors(sgpr_model *h, double *P);
int sgpr_get_neighbors(sgpr_model *h, int64_t *ptr, int32_t *j, int32_t *off);

/* One atom's LCE (neighbour numbers and displacement vectors x_j - x_i + off.cell, descriptor/atoms.py:
 * 365-382 `TorchAtoms.local`) out of the neighbour list of the last evaluated frame, without moving
 * the whole list to the host (the cell is read from the device buffer that step used).
 * nbr_z / nbr_r may be NULL to ask for the count only. */
int sgpr_get_local(sgpr_model *h, int atom, int32_t *nn, int32_t *nbr_z, double *nbr_r, int capacity);

/* K_nm [N][m] of the last evaluated frame (caller order; rows of other ranks' atoms are zero): the
 * `cov` output of sgpr_compute, fetched only when somebody looks at it (calc.cov, active.py:464).
 * N and m are the dimensions the caller's buffer was sized for: SGPR_E_INVALID if the last frame the
 * device evaluated (training rows and trial models rebind it) has other dimensions. */
int sgpr_get_cov(sgpr_model *h, int N, int m, double *cov);

/* Model dimensions, out[8]: out[0]=m, out[1]=S, out[2]=D (dense per block), out[3]=Dc (packed
 * row length used on the device), out[4]=neighbour capacity per atom, out[5]=N bound,
 * out[6]=largest neighbour count seen at the last checked step, out[7]=padded row stride. */
int sgpr_get_dims(sgpr_model *h, int32_t *out);

/* Per-kernel device timings (ms) of the last profiled step; enables HIP-event timing
 * around each stage when `on` != 0 (adds synchronisation: never leave on in production).
 * names: semicolon-separated stage names; returns the number of stages. */
int sgpr_profile(sgpr_model *h, int on);
int sgpr_get_stage_times(sgpr_model *h, double *ms, int cap, char *names, int names_cap);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_HIP_H */
