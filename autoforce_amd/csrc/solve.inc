#include <time.h>
// solve.inc — included at the end of api.hip: the update-path entry points (sgpr_solve,
// sgpr_make_vscale).  Kept apart from the per-step code for readability only.

// At[k][r] = K[r][k] (k < m), At[m][r] = Y[r]: the caller's row-major design matrix transposed on the way
// (32 x 32 tiles through LDS: both sides coalesced).  The least squares runs in the CALLER's column order
// (= the order the inducing LCEs were appended in): a new LCE is then the LAST column of R1, a popped one its last
// column gone.  K_mm's factor is kept species-sorted (block diagonal for the predict path); within a species the
// sorted order IS the append order, so L in the caller's order, L_a[i][j] = L_s[sorted(i)][sorted(j)], is lower
// triangular as well — the second stage reads it through that index map.
__global__ __launch_bounds__(256) void transpose_design_kernel(int rows, int m, const double *K, const double *Y,
                                                               double *At, int ldr)
{
    __shared__ double t[32][33];
    const int r0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, k = k0 + tx;
        double v = 0.0;
        if (r < rows && k <= m) v = k < m ? K[(size_t)r * m + k] : Y[r];
        t[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, r = r0 + tx;
        if (k <= m && r < rows) At[(size_t)k * ldr + r] = t[tx][i];
    }
}

// At[c][rows + i] = sigma L[c][i], i <= c   (regression/gppotential.py:1260: cat(K, sigma @ L.t()))
__global__ void append_sigma_l_kernel(int m, const double *L, int ld, double sigma, double *At, int ldr, int rows)
{
    const int c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m && i <= c) At[(size_t)c * ldr + rows + i] = sigma * L[(size_t)c * ld + i];
}

__global__ void mu_m_mu_kernel(int m, const double *M, int ld, const double *mu, double *t)
{
    // t_q = mu_q (M mu)_q   (regression/gppotential.py:645)
    __shared__ double red[256];
    const int q = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < m; k += 256) s += M[(size_t)q * ld + k] * mu[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) t[q] = mu[q] * red[0];
}

// The stacked system [R1 | z; sigma L^T | 0] of the second QR stage, transposed storage, ROWS INTERLEAVED
// (row 2i = row i of R1, row 2i+1 = row i of sigma L^T): both blocks are upper triangular, so column c is zero
// below row 2c+1 and the factorisation works on a band (launch_lstsq_qr_blocked, band = 2) — a third of the
// flops and panels a third as tall on average.  R (hence mu) does not depend on the order of the rows.
__global__ void stage2_build_kernel(int m, const double *R1 /*column-major*/, int ldR, const double *z, const double *L, int ld,
                                    double sigma, const int *sorted_of, double *At2, int ldr2)
{
    const int c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || c > m) return;
    if (c == m) {
        At2[(size_t)m * ldr2 + 2 * i] = z[i];
        return;
    }
    if (i <= c) {
        At2[(size_t)c * ldr2 + 2 * i] = R1[(size_t)c * ldR + i];
        At2[(size_t)c * ldr2 + 2 * i + 1] = sigma * L[(size_t)sorted_of[c] * ld + sorted_of[i]];
    }
}

// the targets and (c >= 0) column c of the second-stage matrix alone, interleaved rows as stage2_build_kernel lays them out:
// W[0][.] the column (zero when c < 0), W[1][.] the targets — what a kept second stage is asked about (launch_band2_append)
__global__ void stage2_cols_kernel(int m, int c, const double *R1, int ldR, const double *z, const double *L, int ld, double sigma,
                                   const int *sorted_of, double *W, int ldw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    W[(size_t)ldw + 2 * i] = z[i];
    W[(size_t)ldw + 2 * i + 1] = 0.0;
    double a = 0.0, b = 0.0;
    if (c >= 0 && i <= c) {
        a = R1[(size_t)c * ldR + i];
        b = sigma * L[(size_t)sorted_of[c] * ld + sorted_of[i]];
    }
    W[2 * i] = a;
    W[2 * i + 1] = b;
}

// are the leading mo columns of the first-stage factor the ones a kept second stage was made for?  (The column / frame ids say
// which matrix was factored, not by which route: two factorisations of one matrix may differ in the signs of R1's rows.)
__global__ void r1_prefix_differs_kernel(int mo, const double *Rn, int ldn, const double *Ro, int ldo, const double *zn, const double *zo,
                                         int *flag)
{
    const int c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < mo && i <= c && Rn[(size_t)c * ldn + i] != Ro[(size_t)c * ldo + i]) atomicOr(flag, 1);
    if (c == 0 && i < mo && zn[i] != zo[i]) atomicOr(flag, 2);   // (bit 1: other targets than the kept solution was for)
}

// doubles of d_L / d_choli: the m_rows x m_pad matrix plus 64 rows of slack — the trailing update of a species block
// that does not start on a 64-row boundary reads whole 64-row tiles (gemm.hip loads are unguarded, stores are not)
static inline size_t chol_count(const sgpr_model *h) { return (size_t)(h->m_rows + 64) * h->m_pad; }

// jitcholesky (regression/algebra.py:29-47) of K_mm, choli = L^-1; cached until the inducing set changes.
// K_mm is block diagonal by species (sorted order), and so are L and L^-1: every species block is factored and
// inverted on its own (sum n_s^3 instead of m^3 flops, and an edit of the inducing set only costs the blocks it
// touched: blk_ok).  The jitter ladder is the reference's: ONE ridge for the whole matrix, restarted from zero at
// every refit — so blocks cached at a non-zero ridge are never reused.
static int solve_factor_kmm(sgpr_model *h)
{
    if (h->chol_valid) { h->info_blocks_done = 0; return SGPR_OK; }
    const int m = h->m, ld = h->m_pad, S = h->S;
    hipStream_t st = h->stream;
    std::vector<double> diag(m);
    HIPCHK(hipMemcpy2D(diag.data(), sizeof(double), h->d_M.p, sizeof(double) * (ld + 1), sizeof(double), m,
                       hipMemcpyDeviceToHost));
    double scale = 0.0;
    for (int i = 0; i < m; i++) scale += diag[i];
    scale /= m;
    h->chol_dmean = scale;
    const size_t cnt = chol_count(h);
    const bool shape = h->chol_shape && h->d_L.p && h->d_choli.p && h->d_L.n >= cnt && h->d_choli.n >= cnt &&
                       (int)h->blk_ok.size() == S && h->chol_ridge == 0.0;
    if (!shape) {
        if (h->d_L.alloc(cnt) || h->d_choli.alloc(cnt)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (solve)");
        h->blk_ok.assign(S, 0);
    }
    DevBuf<int> &d_info = h->sc_chol_info;
    if (d_info.alloc(S) || (!h->sc_potrf.p && h->sc_potrf.alloc(2 * 64 * 64))) return fail(SGPR_E_NODEVICE, "hipMalloc failed (solve)");
    std::vector<char> todo(S, 0);
    auto attempt = [&](double ridge, bool all, bool *ok) -> int {
        for (int sp = 0; sp < S; sp++) {
            const int b0 = h->qoff[sp], n = h->qoff[sp + 1] - b0;
            todo[sp] = n > 0 && (all || !h->blk_ok[sp]);
            if (!todo[sp]) continue;
            double *Lb = h->d_L.p + (size_t)b0 * ld + b0;
            launch_add_diag(n, h->d_M.p + (size_t)b0 * ld + b0, ld, ridge, Lb, st);
            launch_cholesky_lower(n, Lb, ld, d_info.p + sp, st, h->sc_potrf.p);
        }
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int> info(S, 0);
        HIPCHK(hipMemcpy(info.data(), d_info.p, sizeof(int) * S, hipMemcpyDeviceToHost));
        *ok = true;
        for (int sp = 0; sp < S; sp++)
            if (todo[sp] && info[sp] != 0) *ok = false;
        return 0;
    };
    double ridge = 0.0;
    bool ok = false;
    int rc_ = attempt(0.0, false, &ok);
    if (rc_) return rc_;
    std::vector<char> fresh = todo;  // blocks whose inverse is (re)computed below
    if (!ok) {
        h->blk_ok.assign(S, 0);
        if (scale == 0.0) scale = SGPR_EPS;
        ridge = 1e-6 * scale;
        for (;;) {
            rc_ = attempt(ridge, true, &ok);
            if (rc_) return rc_;
            if (!ok) ridge *= 2.0;
            if (ridge > scale) {
                h->chol_shape = false;
                return fail(SGPR_E_NOT_PD, "cholesky was not successful!");
            }
            if (ok) break;
        }
        fresh = todo;
    }
    h->chol_ridge = ridge;
    h->info_blocks = h->info_blocks_done = 0;
    for (int sp = 0; sp < S; sp++) {
        const int b0 = h->qoff[sp], n = h->qoff[sp + 1] - b0;
        h->info_blocks += n > 0;
        h->info_blocks_done += n > 0 && fresh[sp];
        if (n > 0 && fresh[sp])
            launch_tril_inverse(n, h->d_L.p + (size_t)b0 * ld + b0, ld, h->d_choli.p + (size_t)b0 * ld + b0, st);
        h->blk_ok[sp] = 1;
    }
    h->chol_shape = true;
    h->has_choli = true;
    if (!h->choli_lower) {
        h->choli_lower = true;
        if (h->N > 0) (void)build_tiles(h, 2);
    }
    h->chol_valid = true;
    return SGPR_OK;
}

// stage 1: QR of [K | Y] alone -> R1 (m x m) and z = (Q^T Y)[0:m], kept on the device.  The noise only
// enters the small second stage, so a hyper-parameter search re-solves without touching K again.
// `fill(At, ldr, st)` writes the transposed system At[k][r] (k < m: column k of the design matrix in the caller's
// order, k = m: the targets) into the zero-filled work array.
template <class Fill>
static int solve_stage1(sgpr_model *h, int rows, Fill fill)
{
    const int m = h->m;
    hipStream_t st = h->stream;
    const int R = std::max(rows, m + 1);  // zero rows below a short matrix: their reflectors are identities
    const int ldr = rup(R, 64), cpad = rup(m + 1, 64) + 64;
    DevBuf<double> &d_A = h->d_qr_A, &d_work = h->d_qr_work;  // kept across solves (refits follow each other)
    if (d_A.alloc((size_t)cpad * ldr, false) || d_work.alloc(lstsq_qr_blocked_work_doubles(R, m), false) ||
        h->d_R1.alloc((size_t)m * m + m))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, %d x %d)", R, m);
    HIPCHK(hipMemsetAsync(d_A.p, 0, sizeof(double) * (size_t)cpad * ldr, st));
    if (rows) {
        const int rc_ = fill(d_A.p, ldr, st);
        if (rc_) return rc_;
    }
    if (launch_lstsq_qr_blocked(R, m, d_A.p, ldr, nullptr, d_work.p, st))
        return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    launch_qr_gather_r(m, d_A.p, ldr, h->d_R1.p, m, h->d_R1.p + (size_t)m * m, st);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    h->r1_valid = true;
    return SGPR_OK;
}

// the caller's row-major host matrix: one upload, transposed and species-sorted on the device
static int solve_stage1_host(sgpr_model *h, int rows, const double *K, const double *Y)
{
    const int m = h->m;
    DevBuf<double> d_y, d_Kh;
    if (d_y.alloc(std::max(rows, 1), false) || d_Kh.alloc(std::max((size_t)rows * m, (size_t)1), false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, %d x %d)", rows, m);
    const int rc_ = solve_stage1(h, rows, [&](double *At, int ldr, hipStream_t st) -> int {
        HIPCHK(hipMemcpyAsync(d_Kh.p, K, sizeof(double) * (size_t)rows * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(transpose_design_kernel, dim3((rows + 31) / 32, (m + 1 + 31) / 32), dim3(256), 0, st, rows, m,
                           d_Kh.p, d_y.p, At, ldr);
        return 0;
    });
    d_y.release(); d_Kh.release();   // (in this order, as ever: the addresses later allocations get depend on it)
    return rc_;
}

// stage 2: mu = lstsq([R1; sigma L^T], [z; 0])   (gppotential.py:1255-1263 on the reduced system)
// jitcholesky (regression/algebra.py:29-47) of a matrix the CALLER holds: the ladder of solve_factor_kmm on a dense
// n x n host matrix (one block, no species structure).  L (lower, row-major n x n, upper part zero) and the ridge the
// ladder stopped at come back; SGPR_E_NOT_PD once the ridge passes mean(diag) ("cholesky was not successful!", :45-46).
extern "C" int sgpr_jitcholesky(sgpr_model *h, int n, const double *A, double *L_out, double *ridge_out)
{
    if (!h || n <= 0 || !A || !ridge_out) return fail(SGPR_E_INVALID, "sgpr_jitcholesky: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int ld = rup(n, 64);
    DevBuf<double> dA, dL, dsave;
    DevBuf<int> dinfo;
    if (dA.alloc((size_t)(ld + 64) * ld) || dL.alloc((size_t)(ld + 64) * ld) || dinfo.alloc(1) || dsave.alloc(2 * 64 * 64))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (jitcholesky)");
    HIPCHK(hipMemcpy2D(dA.p, sizeof(double) * ld, A, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice));
    // mean of the diagonal as torch computes it for these sizes (A.diag().mean(): a sequential sum)
    double scale = 0.0;
    for (int i = 0; i < n; i++) scale += A[(size_t)i * n + i];
    scale /= n;
    auto attempt = [&](double ridge, bool *ok) -> int {
        launch_add_diag(n, dA.p, ld, ridge, dL.p, st);
        launch_cholesky_lower(n, dL.p, ld, dinfo.p, st, dsave.p);
        HIPCHK(hipStreamSynchronize(st));
        int info = 0;
        HIPCHK(hipMemcpy(&info, dinfo.p, sizeof(int), hipMemcpyDeviceToHost));
        *ok = info == 0;
        return 0;
    };
    double ridge = 0.0;
    bool ok = false;
    int rc_ = attempt(0.0, &ok);
    if (rc_) return rc_;
    if (!ok) {
        if (scale == 0.0) scale = SGPR_EPS;
        ridge = 1e-6 * scale;
        for (;;) {
            rc_ = attempt(ridge, &ok);
            if (rc_) return rc_;
            if (!ok) ridge *= 2.0;
            if (ridge > scale) return fail(SGPR_E_NOT_PD, "cholesky was not successful!");
            if (ok) break;
        }
    }
    *ridge_out = ridge;
    if (L_out) HIPCHK(hipMemcpy2D(L_out, sizeof(double) * n, dL.p, sizeof(double) * ld, sizeof(double) * n, n, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// hint_we >= 0: the caller is the resident-matrix solve (data.inc) and R1 is the first-stage factor of the columns h->col_ids over
// the frames h->frame_ids with (1) or without (0) their energy rows — what a KEPT second stage is identified by: the same
// model asked again (other targets: the mean moved), or the model before an inducing trial with the trial's ONE more column,
// is answered from the kept reflectors in O(m^2) (bandqr.inc: launch_band2_append) instead of a factorisation.
static int solve_stage2(sgpr_model *h, double noise0, double *mu_out, double *choli_out, double *ridge_out,
                        double *sigma_out, int hint_we = -1)
{
    const int m = h->m, ld = h->m_pad;
    hipStream_t st = h->stream;
    const double sigma = noise0 * (h->chol_dmean * 0.99);  // gppotential.py:1219-1222,:1245-1247
    if (sigma_out) *sigma_out = sigma;
    if (ridge_out) *ridge_out = h->chol_ridge;
    const int R = 2 * m, ldr = rup(R, 64), cpad = rup(m + 1, 64) + 64;
    DevBuf<double> &d_A = h->sc_s2A, &d_x = h->sc_s2x, &d_work = h->sc_s2work;
    DevBuf<int> &d_so = h->sc_s2so;
    if (d_x.alloc(m + 1) || d_so.alloc(m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, stage 2)");
    std::vector<int> sorted_of(m);  // caller index -> species-sorted index
    for (int k = 0; k < m; k++) sorted_of[h->ind_perm[k]] = k;
    HIPCHK(hipMemcpy(d_so.p, sorted_of.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    sgpr_model::S2Keep &k2 = h->s2k;
    static const bool keep_on = !(getenv("SGPR_S2_KEEP") && atoi(getenv("SGPR_S2_KEEP")) == 0);   // SGPR_S2_KEEP=0: every second stage from scratch
    const bool ids = keep_on && hint_we >= 0 && (int)h->col_ids.size() == m && h->frame_ids.size() == h->frames.size();
    int route = 0;   // 0: factorisation; 1: the kept one asked about new targets; 2: ... about one appended column
    if (ids && k2.valid && k2.with_energies == hint_we && k2.noise0 == noise0 && k2.ridge == h->chol_ridge &&
        fabs(sigma - k2.sigma) <= 1e-12 * sigma && k2.frame_ids == h->frame_ids && k2.m >= 1 && (int)k2.col_ids.size() == k2.m) {
        // (sigma = noise * 0.99 * mean(diag K_mm): the mean moves in its last bits with every LCE — diag K_mm = 1 - O(1e-14))
        if (k2.m == m && k2.col_ids == h->col_ids) route = 1;
        else if (k2.m + 1 == m && std::equal(k2.col_ids.begin(), k2.col_ids.end(), h->col_ids.begin())) route = 2;
    }
    if (route) {
        DevBuf<int> &d_f = h->sc_s2flag;
        int differs = 1;
        if (!d_f.alloc(1)) {
            hipLaunchKernelGGL(r1_prefix_differs_kernel, dim3((k2.m + 255) / 256, k2.m), dim3(256), 0, st, k2.m, h->d_R1.p, m, k2.R1.p, k2.m,
                               h->d_R1.p + (size_t)m * m, k2.R1.p + (size_t)k2.m * k2.m, d_f.p);
            HIPCHK(hipMemcpyAsync(&differs, d_f.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        if (differs & 1) route = 0;
        else if (route == 1 && !(differs & 2)) route = 3;   // the very problem the kept solution solved: its mu, bit for bit
    }
    h->info_stage2 = route == 0 ? "factorisation" : route == 1 ? "kept reflectors, new targets" : route == 2 ? "kept reflectors, one appended column"
                                                                                                                 : "kept solution";
    if (route == 3) {
        HIPCHK(hipMemcpyAsync(d_x.p, k2.R1.p + (size_t)k2.m * k2.m + k2.m, sizeof(double) * m, hipMemcpyDeviceToDevice, st));
    } else if (route) {
        const int mo = k2.m, ldw = rup(2 * m + 2, 64);
        DevBuf<double> &d_W = h->sc_s2W;
        if (d_W.alloc((size_t)2 * ldw + mo + 64)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, stage 2)");
        hipLaunchKernelGGL(stage2_cols_kernel, dim3((m + 255) / 256), dim3(256), 0, st, m, route == 2 ? m - 1 : -1, h->d_R1.p, m,
                           h->d_R1.p + (size_t)m * m, h->d_L.p, ld, sigma, d_so.p, d_W.p, ldw);
        if (launch_band2_append(mo, route == 2 ? 1 : 0, d_W.p, ldw, k2.VT.p, d_A.p, rup(2 * mo, 64), d_x.p, d_W.p + (size_t)2 * ldw, st))
            return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    } else {
        k2.valid = false;   // (the factored matrix of the kept one lives in d_A)
        if (d_A.alloc((size_t)cpad * ldr) || d_work.alloc(lstsq_qr_blocked_work_doubles(R, m), false))
            return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, stage 2)");
        hipLaunchKernelGGL(stage2_build_kernel, dim3((m + 255) / 256, m + 1), dim3(256), 0, st, m, h->d_R1.p, m,
                           h->d_R1.p + (size_t)m * m, h->d_L.p, ld, sigma, d_so.p, d_A.p, ldr);
        int done = -2;
        if (ids && !k2.VT.alloc(band_qr_keep_doubles(m), false) && !k2.R1.alloc((size_t)m * m + 2 * (size_t)m, false)) {
            // (R1 | z | the solution: what the kept stage was made for and what it answered)
            HIPCHK(hipMemcpyAsync(k2.R1.p, h->d_R1.p, sizeof(double) * ((size_t)m * m + m), hipMemcpyDeviceToDevice, st));
            done = launch_band2_keep(R, m, d_A.p, ldr, d_x.p, d_work.p, k2.VT.p, st);
            if (done == 0) HIPCHK(hipMemcpyAsync(k2.R1.p + (size_t)m * m + m, d_x.p, sizeof(double) * m, hipMemcpyDeviceToDevice, st));
            if (done == 0) {
                k2.valid = true; k2.m = m; k2.with_energies = hint_we; k2.noise0 = noise0; k2.sigma = sigma; k2.ridge = h->chol_ridge;
                k2.col_ids = h->col_ids; k2.frame_ids = h->frame_ids;
            }
        }
        if (done != 0 && launch_lstsq_qr_blocked(R, m, d_A.p, ldr, d_x.p, d_work.p, st, 2))
            return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    }
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> mus(m), mus_sorted(std::max(h->m_pad, h->m_rows), 0.0);
    HIPCHK(hipMemcpy(mus.data(), d_x.p, sizeof(double) * m, hipMemcpyDeviceToHost));
    for (int k = 0; k < m; k++) mus_sorted[k] = mus[h->ind_perm[k]];  // the predict path's weights: species-sorted
    HIPCHK(hipMemcpy(h->d_mu.p, mus_sorted.data(), sizeof(double) * h->m_pad, hipMemcpyHostToDevice));
    h->has_mu = true;
    if (mu_out)
        for (int k = 0; k < m; k++) mu_out[k] = mus[k];
    if (choli_out) {
        std::vector<double> cs((size_t)h->m_rows * ld);
        HIPCHK(hipMemcpy(cs.data(), h->d_choli.p, sizeof(double) * cs.size(), hipMemcpyDeviceToHost));
        for (int a = 0; a < m; a++)
            for (int b = 0; b < m; b++)
                choli_out[(size_t)h->ind_perm[a] * m + h->ind_perm[b]] = cs[(size_t)a * ld + b];
    }
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

extern "C" int sgpr_solve(sgpr_model *h, int rows, const double *K, const double *Y, double noise0, double *mu_out,
                          double *choli_out, double *ridge_out, double *sigma_out)
{
    if (!h || rows < 0 || (rows > 0 && (!K || !Y))) return fail(SGPR_E_INVALID, "sgpr_solve: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_solve: no inducing set");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    static const bool timing = getenv("SGPR_SOLVE_TIMING") != nullptr;
    auto now = []() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; };
    const double t0 = now();
    int rc_ = solve_factor_kmm(h);
    if (rc_) return rc_;
    const double t1 = now();
    rc_ = solve_stage1_host(h, rows, K, Y);
    if (rc_) return rc_;
    const double t2 = now();
    rc_ = solve_stage2(h, noise0, mu_out, choli_out, ridge_out, sigma_out);
    if (timing)
        fprintf(stderr, "[sgpr solve] rows=%d m=%d: K_mm factor %.2f ms, stage 1 (QR of [K|Y]) %.2f ms, stage 2 (banded QR of [R1; sigma L^T]) %.2f ms\n",
                rows, h->m, t1 - t0, t2 - t1, now() - t2);
    return rc_;
}

extern "C" int sgpr_resolve(sgpr_model *h, double noise0, double *mu_out, double *choli_out, double *ridge_out,
                            double *sigma_out)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_resolve: bad arguments");
    if (h->m <= 0 || !h->chol_valid || !h->r1_valid)
        return fail(SGPR_E_NOMODEL, "sgpr_resolve: no factored design matrix (call sgpr_solve first)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    return solve_stage2(h, noise0, mu_out, choli_out, ridge_out, sigma_out);
}

// A rejected trial (add_1inducing / add_1atoms_fast, gppotential.py:898-982) ends with the model it started from: the
// caller hands back the weights it saved before the trial instead of refitting for them.  The K_mm factor of the
// restored set is the cached one (a bordered pop leaves it valid) or is recomputed here.
extern "C" int sgpr_restore_weights(sgpr_model *h, const double *mu)
{
    if (!h || !mu) return fail(SGPR_E_INVALID, "sgpr_restore_weights: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_restore_weights: no inducing set");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    const int rc_ = solve_factor_kmm(h);
    if (rc_) return rc_;
    std::vector<double> mus(std::max(h->m_pad, h->m_rows), 0.0);
    for (int k = 0; k < h->m; k++) mus[k] = mu[h->ind_perm[k]];
    HIPCHK(hipMemcpy(h->d_mu.p, mus.data(), sizeof(double) * h->m_pad, hipMemcpyHostToDevice));
    h->has_mu = true;
    return SGPR_OK;
}

// The second stage for `count` noise values at once: the grid scan of the noise search
// (_regression(optimize=True), gppotential.py:1265-1300) evaluates the same factored [K | Y] at a dozen noise values,
// each a 2m x m band problem whose launches use at most five CUs — here they share every launch (one grid
// dimension = noise value).  Pure evaluation: the weights installed for prediction are not touched.
extern "C" int sgpr_resolve_batch(sgpr_model *h, int count, const double *noise0, double *mu_out)
{
    if (!h || count < 1 || count > 64 || !noise0 || !mu_out) return fail(SGPR_E_INVALID, "sgpr_resolve_batch: bad arguments");
    if (h->m <= 0 || !h->chol_valid || !h->r1_valid)
        return fail(SGPR_E_NOMODEL, "sgpr_resolve_batch: no factored design matrix (call sgpr_solve first)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int m = h->m, ld = h->m_pad;
    hipStream_t st = h->stream;
    const int R = 2 * m, ldr = rup(R, 64), cpad = rup(m + 1, 64) + 64;
    const size_t bs_mat = (size_t)cpad * ldr, bs_work = lstsq_qr_blocked_work_doubles(R, m);
    DevBuf<double> &d_A = h->sc_bA, &d_x = h->sc_bx, &d_work = h->sc_bwork;
    DevBuf<int> &d_so = h->sc_s2so;
    if (d_A.alloc(bs_mat * count) || d_x.alloc((size_t)m * count) || d_work.alloc(bs_work * count, false) || d_so.alloc(m, false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, %d noise values)", count);
    std::vector<int> sorted_of(m);
    for (int k = 0; k < m; k++) sorted_of[h->ind_perm[k]] = k;
    HIPCHK(hipMemcpy(d_so.p, sorted_of.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    for (int b = 0; b < count; b++) {
        const double sigma = noise0[b] * (h->chol_dmean * 0.99);
        hipLaunchKernelGGL(stage2_build_kernel, dim3((m + 255) / 256, m + 1), dim3(256), 0, st, m, h->d_R1.p, m,
                           h->d_R1.p + (size_t)m * m, h->d_L.p, ld, sigma, d_so.p, d_A.p + b * bs_mat, ldr);
    }
    if (launch_lstsq_qr_batched(R, m, d_A.p, ldr, bs_mat, d_x.p, d_work.p, count, st, 2))
        return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(mu_out, d_x.p, sizeof(double) * (size_t)m * count, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

extern "C" int sgpr_make_vscale(sgpr_model *h, double *vscale_out)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_make_vscale: bad arguments");
    if (h->m <= 0 || !h->has_mu) return fail(SGPR_E_NOMODEL, "sgpr_make_vscale: no inducing set / weights");
    HIPCHK(hipSetDevice(h->device));
    const int m = h->m;
    DevBuf<double> &d_t = h->sc_vs_t;
    if (d_t.alloc(m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed");
    hipLaunchKernelGGL(mu_m_mu_kernel, dim3(m), dim3(256), 0, h->stream, m, h->d_M.p, h->m_pad, h->d_mu.p, d_t.p);
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<double> t(m);
    HIPCHK(hipMemcpy(t.data(), d_t.p, sizeof(double) * m, hipMemcpyDeviceToHost));
    for (int s = 0; s < h->S; s++) {
        double acc = 0.0;
        int c = 0;
        for (int k = 0; k < m; k++)
            if (h->ind_slot[k] == s) { acc += t[k]; c++; }
        h->vscale[s] = c ? acc / c : INFINITY;  // calculator/active.py:795-800
        if (vscale_out) vscale_out[s] = h->vscale[s];
    }
    upload_vscale(h);
    return SGPR_OK;
}


// ---------------------------------------------------------------------------- training rows
// part[chunk][q] = sum_{i in chunk} K[i][q]: 64 columns x 256 rows per workgroup, rows coalesced across lanes;
// the chunks are summed in order by rows_colsum_final_kernel (no atomics: K_e repeats bit for bit, and the
// ill-conditioned fit that amplifies its last bits with it)
__global__ __launch_bounds__(256) void rows_colsum_kernel(int n, int m, int ldk, const double *K, double *part)
{
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + tx;
    const int i0 = blockIdx.y * 256, i1 = min(n, i0 + 256);
    double s = 0.0;
    if (q < m)
        for (int i = i0 + ty; i < i1; i += 4) s += K[(size_t)i * ldk + q];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && q < m) part[(size_t)blockIdx.y * m + q] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

__global__ void rows_colsum_final_kernel(int nchunks, int m, const double *part, double *out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; c++) s += part[(size_t)c * m + q];
    out[q] = s;
}

// ---- sixteen columns per workgroup pass (descriptor.hip / rows16.inc): gather, virial sums ----
struct Fin16Args {
    int N, maxnn, gnn, S;
    short chunk[32];            // chunk number of each blockIdx.y
    int qoff[SGPR_MAX_S + 1];
    const int *nn, *nbr_code, *slot, *perm;
    const int *row_of;          // [m] sorted inducing index -> row of `out`, or -1 (column not asked for)
    const double *G, *Fself;
    size_t g_stride, f_stride, rowlen;
    double *out;                // [columns][rowlen] packed rows (forces in the caller's atom order)
};

// One wave per atom a and chunk: K_F[(a, x)][q] = own sum (q of a's species) - sum over a's list slots of the pair
// gradients handed over by the neighbours of q's species.  Lane = (column, quarter of the list); per-lane sums run in
// list order, the four quarters are added by two shuffles: the same bits every run.
template <int ST>
__global__ __launch_bounds__(256) void rows16_finalize_kernel(Fin16Args f)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave, ch = blockIdx.y;
    if (i >= f.N) return;
    const int col = lane & 15, tq = lane >> 4;
    const int n = min(f.nn[i], f.gnn);
    const double *G = f.G + ch * f.g_stride + (size_t)i * f.gnn * 48;
    double acc[ST][3];
#pragma unroll
    for (int s = 0; s < ST; s++) acc[s][0] = acc[s][1] = acc[s][2] = 0.0;
    for (int t = tq; t < n; t += 4) {
        const int st = (f.nbr_code[(size_t)i * f.maxnn + t] >> 24) & 0xff;
        // (a neighbour whose species block has no chunk here wrote nothing: its slot holds stale bytes, dropped below)
        const double v0 = G[(t * 3 + 0) * 16 + col], v1 = G[(t * 3 + 1) * 16 + col], v2 = G[(t * 3 + 2) * 16 + col];
#pragma unroll
        for (int s = 0; s < ST; s++) {
            acc[s][0] += st == s ? v0 : 0.0;
            acc[s][1] += st == s ? v1 : 0.0;
            acc[s][2] += st == s ? v2 : 0.0;
        }
    }
    const int si = f.slot[i], c = f.perm[i];
#pragma unroll
    for (int s = 0; s < ST; s++) {
        if (s >= f.S) break;
        const int q = f.qoff[s] + 16 * f.chunk[ch] + col;
        const bool have = q < f.qoff[s + 1];  // (lane-dependent only in the block's last chunk)
        const int row = have ? f.row_of[q] : -1;
#pragma unroll
        for (int x = 0; x < 3; x++) {
            double v = have ? acc[s][x] : 0.0;
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (tq == 0 && row >= 0) {
                const double own = s == si ? f.Fself[ch * f.f_stride + ((size_t)i * 3 + x) * 16 + col] : 0.0;
                f.out[(size_t)row * f.rowlen + 3 * (size_t)c + x] = own - v;
            }
        }
    }
}

// virial sums of a column: the per-atom partials of the atoms of the column's species, in atom order — 64 contiguous
// segments summed by 64 workgroups (16 parts each, fixed tree), then the segments in order
__global__ __launch_bounds__(256) void rows16_vir_part_kernel(int S, const int *aoff, const double *vir, size_t v_stride, double *part)
{
    __shared__ double red[16][9][16];
    const int seg = blockIdx.x, sp = blockIdx.y, ch = blockIdx.z;
    const int col = threadIdx.x & 15, pt = threadIdx.x >> 4;
    const int a0 = aoff[sp], a1 = aoff[sp + 1], len = (a1 - a0 + 63) / 64;
    const int b0 = a0 + seg * len, b1 = min(a1, b0 + len);
    double s9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = b0 + pt; a < b1; a += 16) {
        const double *src = vir + ch * v_stride + (size_t)a * 144 + col;
#pragma unroll
        for (int k = 0; k < 9; k++) s9[k] += src[k * 16];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) red[pt][k][col] = s9[k];
    __syncthreads();
    if (threadIdx.x < 144) {
        const int k = threadIdx.x >> 4, c = threadIdx.x & 15;
        double t = 0.0;
        for (int p = 0; p < 16; p++) t += red[p][k][c];
        part[(((size_t)ch * S + sp) * 64 + seg) * 144 + k * 16 + c] = t;
    }
}

__global__ void rows16_vir_final_kernel(int S, Fin16Args f, const int *qoff, const int *row_of, const double *part, double *out,
                                        size_t rowlen, int N)
{
    const int sp = blockIdx.x, ch = blockIdx.y;
    if (threadIdx.x >= 144) return;
    const int k = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int q = qoff[sp] + 16 * f.chunk[ch] + c;
    if (q >= qoff[sp + 1]) return;
    const int row = row_of[q];
    if (row < 0) return;
    double t = 0.0;
    for (int seg = 0; seg < 64; seg++) t += part[(((size_t)ch * S + sp) * 64 + seg) * 144 + k * 16 + c];
    out[(size_t)row * rowlen + 4 * (size_t)N + 1 + k] = t;
}

// Rows of one frame for inducing columns [q_first, q_first + q_count), left ON THE DEVICE and enqueued on
// h->stream (not synchronised): h->d_rows_out[c][4N+11] = packed result of column c (forces [3N] in the caller's
// atom order, then N unused, energy-free tail with the 9 virial sums at +1), h->d_rows_ke[sorted column] = K_e
// of ALL m columns, h->rows_cols[c] = species-sorted index of column q_first + c.
static int rows_compute(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                        const int32_t *pbc, int q_first, int q_count)
{
    if (!h || N <= 0 || !numbers || !positions || !cell) return fail(SGPR_E_INVALID, "sgpr_kernel_rows: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_kernel_rows: no inducing set");
    if (q_first < 0 || q_count < 0 || q_first + q_count > h->m)
        return fail(SGPR_E_INVALID, "sgpr_kernel_columns: columns [%d, %d) outside the inducing set (m = %d)", q_first,
                    q_first + q_count, h->m);
    HIPCHK(hipSetDevice(h->device));
    bool same = (N == h->N && h->rank == 0 && h->world == 1 && (int)h->numbers.size() == N);
    if (same)
        for (int i = 0; i < N && same; i++) same = h->numbers[i] == numbers[i];
    if (same && pbc)
        for (int k = 0; k < 3; k++) same = same && (h->pbc[k] == (pbc[k] != 0));
    if (!same) {
        const int rc_ = sgpr_bind_system(h, N, numbers, pbc, 0, 1);
        if (rc_) return rc_;
    }
    hipStream_t st = h->stream;
    const int m = h->m;
    HIPCHK(hipMemcpyAsync(h->d_pos_in.p, positions, sizeof(double) * 3 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->d_cell_in.p, cell, sizeof(double) * 9, hipMemcpyHostToDevice, st));
    // neighbour list, descriptors and K_nm with unit weights (Aw = eta dot^(eta-1)), capacity-checked
    DevBuf<double> &d_ones = h->d_rows_ones, &d_rows = h->d_rows_out, &d_ke = h->d_rows_ke;  // kept across calls
    const size_t rowlen = (size_t)4 * N + 11;
    if (d_ones.alloc(std::max(h->m_pad, h->m_rows), false) || d_rows.alloc(rowlen * std::max(q_count, 1)) || d_ke.alloc(m))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows, %d x %zu)", m, rowlen);
    {
        std::vector<double> ones(std::max(h->m_pad, h->m_rows), 1.0);
        HIPCHK(hipMemcpy(d_ones.p, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice));
    }
    h->rows_mu = d_ones.p;
    int rc_ = run_checked(h, h->d_pos_in.p, h->d_cell_in.p, h->d_packed.p, st);
    h->rows_mu = nullptr;
    h->warm = false;
    if (rc_) return rc_;
    {
        const int nchunks = (h->cnt + 255) / 256;
        if (h->d_rows_kepart.alloc((size_t)std::max(nchunks, 1) * m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows)");
        hipLaunchKernelGGL(rows_colsum_kernel, dim3((m + 63) / 64, nchunks), dim3(256), 0, st, h->cnt, m, h->m_pad, h->d_K.p,
                           h->d_rows_kepart.p);
        hipLaunchKernelGGL(rows_colsum_final_kernel, dim3((m + 255) / 256), dim3(256), 0, st, nchunks, m, h->d_rows_kepart.p, d_ke.p);
    }
    DescParams dp = {};
    dp.lmax = h->lmax; dp.nmax = h->nmax; dp.S = h->S; dp.N = h->cnt; dp.Nall = N; dp.first = 0; dp.stride = 1;
    dp.maxnn = h->maxnn; dp.Dc = h->Dc; dp.Dpad = h->Dpad; dp.CS = h->CS; dp.rc = h->rc; dp.stat = h->d_stat.p;
    for (int k = 0; k < SGPR_MAX_S; k++) dp.radii_v[k] = k < h->S ? h->radii[k] : 1.0;
    std::vector<int> sorted_of(m);  // caller index -> species-sorted index
    for (int k = 0; k < m; k++) sorted_of[h->ind_perm[k]] = k;
    // columns in batches of RB per launch (blockIdx.y): the reverse kernel forms the seed of column q on the
    // fly, W_i = Aw[i][q] * Pm[q][:], skips atoms of other species (Aw = 0) and writes batch-strided outputs
    const int RB = 16;
    const bool gather = h->gather_ok && h->d_T.p != nullptr;
    const size_t g_stride = (size_t)N * h->maxnn * 4, f_stride = (size_t)6 * N, v_stride = (size_t)9 * std::max(h->virpart_len, 1);
    DevBuf<double> &d_bG = h->d_rows_bG, &d_bF = h->d_rows_bF, &d_bV = h->d_rows_bV;
    DevBuf<int> &d_cols = h->d_rows_cols;
    if (d_cols.alloc(std::max(q_count, 1), false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows, batch buffers)");
    {
        std::vector<int> cols(std::max(q_count, 1), 0);
        for (int c = 0; c < q_count; c++) cols[c] = sorted_of[q_first + c];
        HIPCHK(hipMemcpy(d_cols.p, cols.data(), sizeof(int) * std::max(q_count, 1), hipMemcpyHostToDevice));
    }
    // Sixteen columns per workgroup pass (rows16.inc) where the instantiation exists: chunk c of every species block per
    // launch, only the chunks, species blocks and columns the call asks for.  The rare shapes (lists beyond 64 neighbours,
    // lmax or nmax of 4, more than four species slots) keep the one-column-per-wave form.  The choice depends on the frame
    // and the model, never on which columns are asked for: a column of the resident design matrix has the same bits
    // whether it came with all the others (set_data / add_data) or alone (the border of an appended LCE).
    int nn_longest = 0;
    bool wide = gather && q_count >= h->rows16_min && h->rows16 && h->S <= 4 && (h->nmax + 1) * (h->lmax + 1) * (h->lmax + 1) <= 64;
    if (wide) {
        std::vector<int> nnv(N);  // the longest list of this frame (64 KB at 16384 atoms: not worth a kernel)
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(nnv.data(), h->d_nn.p, sizeof(int) * N, hipMemcpyDeviceToHost));
        nn_longest = *std::max_element(nnv.begin(), nnv.end());
        if (nn_longest > 64) wide = false;
    }
    if (wide) {
        int nchunks = 0;
        for (int sp = 0; sp < h->S; sp++) nchunks = std::max(nchunks, (h->qoff[sp + 1] - h->qoff[sp] + 15) / 16);
        const int gnn = std::max(nn_longest, 1);
        const size_t g16 = (size_t)N * gnn * 48, f16 = (size_t)N * 48, v16 = (size_t)N * 144;
        size_t budget = (size_t)std::max(h->rows16_mb, 1) << 20;
        {   // (a quarter of what is free at most: several models may share the GPU)
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max<size_t>(free_b / 4 + d_bG.n * sizeof(double), (size_t)256 << 20));
        }
        // (sized for full 64-slot rows whatever this frame's longest list is: the next frame must not find the buffer a
        // few percent short and pay a multi-gigabyte hipFree + hipMalloc, 0.4 s)
        const size_t g16_cap = (size_t)N * 64 * 48;
        int per = (int)std::max<size_t>(1, std::min<size_t>(std::min(nchunks, (q_count + 15) / 16 + h->S), budget / (g16_cap * sizeof(double))));
        std::vector<int> row_of(m, -1);
        for (int c = 0; c < q_count; c++) row_of[sorted_of[q_first + c]] = c;
        DevBuf<int> &d_rowof = h->d_rows_rowof, &d_qoff = h->d_rows_qoff;
        DevBuf<double> &d_vp = h->d_rows_vpart;
        // (no room for the hand-over buffer of that many chunks: fewer per launch, down to one)
        while (per > 1 && d_bG.alloc(g16_cap * per, false)) { (void)hipGetLastError(); per = (per + 1) / 2; }
        if (d_bG.alloc(g16_cap * per, false) || d_bF.alloc(f16 * per, false) || d_bV.alloc(v16 * per, false) ||
            d_rowof.alloc(m, false) || d_qoff.alloc(2 * (h->S + 1), false) || d_vp.alloc((size_t)per * h->S * 64 * 144, false))
            return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows, %d chunks of sixteen columns)", per);
        HIPCHK(hipMemcpy(d_rowof.p, row_of.data(), sizeof(int) * m, hipMemcpyHostToDevice));
        {
            std::vector<int> offs(2 * (h->S + 1));
            for (int sp = 0; sp <= h->S; sp++) { offs[sp] = h->qoff[sp]; offs[h->S + 1 + sp] = h->aoff[sp]; }
            HIPCHK(hipMemcpy(d_qoff.p, offs.data(), sizeof(int) * offs.size(), hipMemcpyHostToDevice));
        }
        Rows16Params rp = {};
        rp.aw = h->d_Aw.p; rp.k = h->d_K.p; rp.eta = h->eta; rp.ld = h->m_pad; rp.pm = h->d_Pm.p;
        for (int sp = 0; sp <= SGPR_MAX_S; sp++) rp.qoff[sp] = h->qoff[std::min(sp, h->S)];
        rp.G = d_bG.p; rp.Fself = d_bF.p; rp.vir = d_bV.p; rp.g_stride = g16; rp.f_stride = f16; rp.v_stride = v16;
        Fin16Args fa = {};
        fa.N = N; fa.maxnn = h->maxnn; fa.gnn = gnn; fa.S = h->S;
        rp.gnn = gnn;
        for (int sp = 0; sp <= SGPR_MAX_S; sp++) fa.qoff[sp] = rp.qoff[sp];
        fa.nn = h->d_nn.p; fa.nbr_code = h->d_nbr_shift.p; fa.slot = h->d_slot.p; fa.perm = h->d_perm.p; fa.row_of = d_rowof.p;
        fa.G = d_bG.p; fa.Fself = d_bF.p; fa.g_stride = g16; fa.f_stride = f16; fa.rowlen = rowlen; fa.out = d_rows.p;
        // only the chunks that hold a column of the call, and in them only the species blocks and columns asked for
        std::vector<int> todo;
        std::vector<std::array<unsigned short, 4>> masks;
        for (int c = 0; c < nchunks; c++) {
            std::array<unsigned short, 4> mk = {0, 0, 0, 0};
            bool any = false;
            for (int sp = 0; sp < h->S; sp++)
                for (int k = 0; k < 16; k++) {
                    const int q = h->qoff[sp] + 16 * c + k;
                    if (q < h->qoff[sp + 1] && row_of[q] >= 0) { mk[sp] |= (unsigned short)(1u << k); any = true; }
                }
            if (any) { todo.push_back(c); masks.push_back(mk); }
        }
        const int per_launch = std::min(per, 32);
        for (size_t t0 = 0; t0 < todo.size() && wide; t0 += per_launch) {
            rp.nch = (int)std::min<size_t>(per_launch, todo.size() - t0);
            for (int ch = 0; ch < rp.nch; ch++) {
                rp.chunk[ch] = fa.chunk[ch] = (short)todo[t0 + ch];
                for (int sp = 0; sp < 4; sp++) rp.cmask[ch][sp] = masks[t0 + ch][sp];
            }
            rc_ = launch_rows16(dp, h->d_slot.p, h->d_nn.p, h->d_nbr_j.p, h->d_nbr_shift.p, h->d_pack.p, h->d_Pn.p, h->d_norm.p,
                                h->d_C.p, h->d_shear.p, h->d_prec.p, h->d_aux.p, h->d_T.p, h->t_stride, h->d_cidx.p, h->d_hm.p,
                                h->hmw, rp, st);
            if (rc_) { wide = false; break; }  // not compiled in: the per-column form below
            const dim3 fg((N + 3) / 4, rp.nch);
            if (h->S <= 1) hipLaunchKernelGGL(rows16_finalize_kernel<1>, fg, dim3(256), 0, st, fa);
            else if (h->S <= 2) hipLaunchKernelGGL(rows16_finalize_kernel<2>, fg, dim3(256), 0, st, fa);
            else hipLaunchKernelGGL(rows16_finalize_kernel<4>, fg, dim3(256), 0, st, fa);
            hipLaunchKernelGGL(rows16_vir_part_kernel, dim3(64, h->S, rp.nch), dim3(256), 0, st, h->S, d_qoff.p + h->S + 1, d_bV.p, v16, d_vp.p);
            hipLaunchKernelGGL(rows16_vir_final_kernel, dim3(h->S, rp.nch), dim3(256), 0, st, h->S, fa, d_qoff.p, d_rowof.p, d_vp.p,
                               d_rows.p, rowlen, N);
        }
    }
    h->info_rows = wide ? "sixteen columns per workgroup pass" : "one column per wave";
    if (!wide && ((gather && d_bG.alloc(g_stride * RB, false)) || d_bF.alloc(f_stride * RB) || d_bV.alloc(v_stride * RB)))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows, batch buffers)");
    for (int c0 = 0; c0 < q_count && !wide; c0 += RB) {
        const int nb = std::min(RB, q_count - c0);
        if (!gather) HIPCHK(hipMemsetAsync(d_bF.p, 0, sizeof(double) * f_stride * nb, st));  // scatter form accumulates
        RowsBatch rb = {h->d_Aw.p, h->d_Pm.p, d_cols.p + c0, h->d_ind_slot.p, h->m_pad, nb, g_stride, f_stride, v_stride};
        rc_ = launch_descriptor_backward(dp, h->d_pos.p, h->d_cell_in.p, h->d_slot.p, h->d_radii.p, h->d_nn.p,
                                         h->d_nbr_j.p, h->d_nbr_shift.p, h->d_pack.p, h->d_Pn.p, h->d_norm.p,
                                         h->d_C.p, h->d_shear.p, nullptr, h->d_prec.p, gather ? d_bG.p : nullptr,
                                         h->d_aux.p, h->d_T.p, h->t_stride, h->d_cidx.p, h->d_hm.p, h->hmw, d_bF.p,
                                         d_bV.p, st, &rb);
        if (rc_) return fail(SGPR_E_UNSUPPORTED, "descriptor kernel not compiled in");
        FinBatch fb = {nb, d_bG.p, d_bF.p, d_bV.p, g_stride, f_stride, v_stride, rowlen, d_cols.p + c0};
        launch_finalize(h, gather, 0, h->virpart_len, false, 0.0, d_rows.p + rowlen * c0, st, &fb);
    }
    h->rows_cols.assign(q_count, 0);
    for (int c = 0; c < q_count; c++) h->rows_cols[c] = sorted_of[q_first + c];
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

static int kernel_rows_range(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                             const double *cell, const int32_t *pbc, int q_first, int q_count, double *Ke,
                             double *Kf, double *Kv)
{
    const int rc_ = rows_compute(h, N, numbers, positions, cell, pbc, q_first, q_count);
    if (rc_) return rc_;
    hipStream_t st = h->stream;
    const int m = h->m;
    const size_t rowlen = (size_t)4 * N + 11;
    DevBuf<double> &d_rows = h->d_rows_out, &d_ke = h->d_rows_ke;
    // forces of all columns, transposed on the device into the caller's [3N][q_count] layout: one copy, no host loop
    DevBuf<double> d_kft;
    if (Kf && q_count > 0) {
        if (d_kft.alloc((size_t)3 * N * q_count, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (training rows)");
        hipLaunchKernelGGL(transpose_kernel, dim3((3 * N + 31) / 32, (q_count + 31) / 32), dim3(32, 8), 0, st, q_count, 3 * N,
                           d_rows.p, (int)rowlen, d_kft.p, q_count);
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (Kf && q_count > 0) HIPCHK(hipMemcpy(Kf, d_kft.p, sizeof(double) * (size_t)3 * N * q_count, hipMemcpyDeviceToHost));
    d_kft.release();
    std::vector<double> ke(m), tail((size_t)11 * std::max(q_count, 1));
    if (q_count > 0)
        HIPCHK(hipMemcpy2D(tail.data(), sizeof(double) * 11, d_rows.p + 4 * (size_t)N, sizeof(double) * rowlen, sizeof(double) * 11,
                           q_count, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ke.data(), d_ke.p, sizeof(double) * m, hipMemcpyDeviceToHost));
    const int voigt[6] = {0, 4, 8, 5, 2, 1};
    for (int c = 0; c < q_count; c++) {
        if (Ke) Ke[c] = ke[h->rows_cols[c]];
        if (Kv)
            for (int v = 0; v < 6; v++) Kv[(size_t)v * q_count + c] = tail[(size_t)11 * c + 1 + voigt[v]];
    }
    return SGPR_OK;
}

extern "C" int sgpr_kernel_rows(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                                const double *cell, const int32_t *pbc, double *Ke, double *Kf, double *Kv)
{
    return kernel_rows_range(h, N, numbers, positions, cell, pbc, 0, h ? h->m : 0, Ke, Kf, Kv);
}

extern "C" int sgpr_kernel_columns(sgpr_model *h, int N, const int32_t *numbers, const double *positions,
                                   const double *cell, const int32_t *pbc, int q_first, int q_count, double *Ke,
                                   double *Kf, double *Kv)
{
    return kernel_rows_range(h, N, numbers, positions, cell, pbc, q_first, q_count, Ke, Kf, Kv);
}

// ---------------------------------------------------------------------------- inducing-set edits
// The library keeps the caller's LCE list (h->env_*), edits it and rebuilds descriptors + K_mm:
// m descriptor evaluations and one m x m x Dc GEMM, microseconds next to the O(m^3) refactor
// that follows every edit in the reference as well (gppotential.py:745-772 -> make_munu).
static int rebuild_inducing(sgpr_model *h)
{
    const std::vector<int32_t> zc = h->env_zc, nz = h->env_z;
    const std::vector<int64_t> ptr = h->env_ptr;
    const std::vector<double> nr = h->env_r;
    return sgpr_set_inducing(h, (int)zc.size(), zc.data(), ptr.data(), nz.data(), nr.data());
}

// ---- incremental edits (BASELINE config 5: on-the-fly inducing-set updates) --------------------
// Appending the LCE that update_lce / add_1inducing tries (gppotential.py:745-771, :955-982) costs ONE
// descriptor row, ONE row of K_mm and a bordered Cholesky step instead of m descriptor rows, an
// m x m x D product and (at the next solve) an O(m^3) factorisation + inverse:
//   M' = [M k; k^T kxx],  L' = [L 0; l^T lam],  l = L^-1 k,  lam^2 = kxx + ridge - l.l,
//   L'^-1 = [L^-1 0; -(l^T L^-1)/lam  1/lam].
// Everything lives in species-sorted order, K_mm / L / L^-1 are block diagonal, and the new LCE joins the
// END of its species block (stable sort): only that block's rows enter l, and the later blocks shift by one.
// The K_mm row comes from the same MFMA kernel with the same reduction order as a rebuild, so M is bit
// identical to sgpr_set_inducing's.  Popping the LCE added last (pop_1inducing, :782-791) deletes the last
// row / column of its block: L and L^-1 of the rest are untouched.
// The bordered step applies while the jitter ladder sits at ridge = 0 (the normal state; the reference
// restarts its ladder from zero at every refit, algebra.py:29-47) and the new pivot is positive; anything
// else drops the cached factor and the next solve runs the full ladder.

// dst[r'][c'] = src[r][c] with one row and/or column inserted (del = 0) or removed (del = 1) at (pr, pc);
// pr / pc < 0: that axis is copied as it is.  Inserted lines are left zero (dst is zero-filled).
__global__ void reindex_copy_kernel(int rows, int cols, const double *src, int lds, double *dst, int ldd, int pr, int pc,
                                    int del)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (r >= rows || c >= cols) return;
    int r2 = r, c2 = c;
    if (pr >= 0) {
        if (del) { if (r == pr) return; r2 = r - (r > pr); }
        else r2 = r + (r >= pr);
    }
    if (pc >= 0) {
        if (del) { if (c == pc) return; c2 = c - (c > pc); }
        else c2 = c + (c >= pc);
    }
    dst[(size_t)r2 * ldd + c2] = src[(size_t)r * lds + c];
}

// row `pos` and column `pos` of the new K_mm from the row the GEMM produced (old sorted column index j -> new)
__global__ void border_fill_kernel(int m_old, int pos, const double *krow /*[m_old]*/, double kxx, double *M, int ld)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m_old) {
        const int j2 = j + (j >= pos);
        M[(size_t)pos * ld + j2] = krow[j];
        M[(size_t)j2 * ld + pos] = krow[j];
    }
    if (j == 0) M[(size_t)pos * ld + pos] = kxx;
}

// bordered Cholesky + inverse of the block [b0, pos) extended by `pos` (one workgroup; arrays already re-indexed)
__global__ __launch_bounds__(256) void chol_border_kernel(int b0, int pos, const double *M, double ridge, double *L,
                                                          double *Li, int ld, int *info)
{
    extern __shared__ double lsh[];  // [nb]
    __shared__ double red[256];
    const int nb = pos - b0, tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nb; i += 256) {
        double v = 0.0;
        for (int j = 0; j <= i; j++) v += Li[(size_t)(b0 + i) * ld + b0 + j] * M[(size_t)pos * ld + b0 + j];
        lsh[i] = v;
        acc += v * v;
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double lam2 = M[(size_t)pos * ld + pos] + ridge - red[0];
    if (!(lam2 > 0.0)) {  // the leading minor is not positive definite: potrf's criterion (linalg.hip)
        if (tid == 0) *info = pos + 1;
        return;
    }
    const double lam = sqrt(lam2), ilam = 1.0 / lam;
    for (int j = tid; j < nb; j += 256) {
        L[(size_t)pos * ld + b0 + j] = lsh[j];
        double v = 0.0;
        for (int i = j; i < nb; i++) v += lsh[i] * Li[(size_t)(b0 + i) * ld + b0 + j];
        Li[(size_t)pos * ld + b0 + j] = -v * ilam;
    }
    if (tid == 0) {
        L[(size_t)pos * ld + pos] = lam;
        Li[(size_t)pos * ld + pos] = ilam;
        *info = 0;
    }
}

// re-indexed copy of a [rows x cols] device array into the same buffer at its new padded shape: the old
// content is parked in a scratch buffer kept by the handle (no allocation unless a padded size grows),
// everything enqueued on `st`
static int reindex_into(sgpr_model *h, DevBuf<double> &buf, int rows, int cols, int ld_old, size_t new_count, int ld_new,
                        int pr, int pc, int del, hipStream_t st)
{
    const size_t old_count = (size_t)rows * ld_old;
    if (h->d_edit_tmp.n < old_count) {
        (void)hipStreamSynchronize(st);
        if (h->d_edit_tmp.alloc(old_count + old_count / 4 + 4096, false)) return -1;
    }
    if (old_count && buf.p)
        (void)hipMemcpyAsync(h->d_edit_tmp.p, buf.p, sizeof(double) * old_count, hipMemcpyDeviceToDevice, st);
    if (buf.n < new_count || !buf.p) {
        (void)hipStreamSynchronize(st);
        if (buf.alloc(new_count + new_count / 8, false)) return -1;  // head-room: the next edits reuse it
    }
    (void)hipMemsetAsync(buf.p, 0, sizeof(double) * new_count, st);
    if (rows > 0 && cols > 0)
        hipLaunchKernelGGL(reindex_copy_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, st, rows, cols, h->d_edit_tmp.p,
                           ld_old, buf.p, ld_new, pr, pc, del);
    return 0;
}

// shared tail of the incremental edits: host tables, small device tables, tile tables
static int edit_commit(sgpr_model *h, const std::vector<int> &slot_caller)
{
    const int m = h->m;
    h->ind_perm.resize(m);
    std::iota(h->ind_perm.begin(), h->ind_perm.end(), 0);
    std::stable_sort(h->ind_perm.begin(), h->ind_perm.end(), [&](int a, int b) { return slot_caller[a] < slot_caller[b]; });
    h->ind_slot.resize(m);
    h->qoff.assign(h->S + 1, 0);
    std::vector<int> nn(h->m_rows, 1), dslot(h->m_rows, -2);
    for (int k = 0; k < m; k++) {
        const int q = h->ind_perm[k];
        h->ind_slot[k] = dslot[k] = slot_caller[q];
        h->qoff[slot_caller[q] + 1]++;
        int cnt = 0;
        for (int64_t e = h->env_ptr[q]; e < h->env_ptr[q + 1]; e++) cnt += slot_of(h, h->env_z[e]) >= 0;
        nn[k] = cnt;
    }
    for (int s = 0; s < h->S; s++) h->qoff[s + 1] += h->qoff[s];
    if (h->d_ind_slot.alloc(h->m_rows) || h->d_ind_nn.alloc(h->m_rows) || h->d_mu.alloc(std::max(h->m_pad, h->m_rows)))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
    HIPCHK(hipMemcpy(h->d_ind_slot.p, dslot.data(), sizeof(int) * h->m_rows, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_ind_nn.p, nn.data(), sizeof(int) * h->m_rows, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_qoff.p, h->qoff.data(), sizeof(int) * (h->S + 1), hipMemcpyHostToDevice));
    h->has_mu = false;
    h->r1_valid = false;
    if (build_tiles(h, 3)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (tile table)");
    if (h->N > 0) return alloc_work(h);
    return SGPR_OK;
}

extern "C" int sgpr_add_inducing(sgpr_model *h, int32_t zc, int nn, const int32_t *nbr_z, const double *nbr_r)
{
    if (!h || nn < 0 || (nn > 0 && (!nbr_z || !nbr_r))) return fail(SGPR_E_INVALID, "sgpr_add_inducing: bad arguments");
    const int s_new = slot_of(h, zc);
    if (s_new < 0) return fail(SGPR_E_SPECIES, "inducing LCE: Z=%d is not in the species table", zc);
    for (int e = 0; e < nn; e++)
        if (slot_of(h, nbr_z[e]) < 0 && !h->ignore_unknown)
            return fail(SGPR_E_SPECIES, "inducing LCE: neighbour Z=%d is not in the species table", nbr_z[e]);
    HIPCHK(hipSetDevice(h->device));
    const int m_old = h->m;
    if (h->env_ptr.empty()) h->env_ptr.push_back(0);
    // the host-side LCE list grows first (the kernels below read it); every failure path before the device arrays
    // have been re-indexed takes the entry back, so that the list never runs ahead of the device
    struct EnvGuard {
        sgpr_model *h; size_t nzc, nz, nr, np; bool armed;
        ~EnvGuard() { if (armed) { h->env_zc.resize(nzc); h->env_z.resize(nz); h->env_r.resize(nr); h->env_ptr.resize(np); } }
    } guard = {h, h->env_zc.size(), h->env_z.size(), h->env_r.size(), h->env_ptr.size(), true};
    h->env_zc.push_back(zc);
    h->env_z.insert(h->env_z.end(), nbr_z, nbr_z + nn);
    h->env_r.insert(h->env_r.end(), nbr_r, nbr_r + 3 * (size_t)nn);
    h->env_ptr.push_back((int64_t)h->env_z.size());
    if (m_old == 0 || !h->d_Pm.p || !h->d_M.p) {
        const int rc0 = rebuild_inducing(h);
        if (rc0 == SGPR_OK || h->m == m_old + 1) guard.armed = false;  // (set_inducing validates before it commits)
        return rc0;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    hipStream_t st = h->stream;
    // ---- the new LCE's descriptor (one environment)
    std::vector<int> eslot;
    std::vector<double> er;
    for (int e = 0; e < nn; e++) {
        const int sl = slot_of(h, nbr_z[e]);
        if (sl < 0) continue;  // ignore_unknown
        eslot.push_back(sl);
        er.push_back(nbr_r[3 * e]); er.push_back(nbr_r[3 * e + 1]); er.push_back(nbr_r[3 * e + 2]);
    }
    const int nk = (int)eslot.size();
    const int64_t ptr[2] = {0, nk};
    DevBuf<int64_t> &d_ptr = h->sc_ai_ptr;
    DevBuf<int> &d_eslot = h->sc_ai_eslot, &d_one_slot = h->sc_ai_oslot, &d_one_nn = h->sc_ai_onn, &d_info = h->sc_ai_info;
    DevBuf<double> &d_er = h->sc_ai_er, &d_p = h->sc_ai_p, &d_norm = h->sc_ai_norm, &d_krow = h->sc_ai_krow, &d_kself = h->sc_ai_kself;
    if (d_ptr.alloc(2, false) || d_eslot.alloc(std::max(nk, 1), false) || d_er.alloc(3 * (size_t)std::max(nk, 1), false) ||
        d_p.alloc(64 * (size_t)h->Dpad) || d_norm.alloc(64) || d_krow.alloc((size_t)64 * h->m_pad) ||
        d_kself.alloc((size_t)64 * 64) || d_one_slot.alloc(64) || d_one_nn.alloc(64) || d_info.alloc(1))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
    HIPCHK(hipMemcpy(d_ptr.p, ptr, sizeof(ptr), hipMemcpyHostToDevice));
    if (nk > 0) {
        HIPCHK(hipMemcpy(d_eslot.p, eslot.data(), sizeof(int) * nk, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_er.p, er.data(), sizeof(double) * 3 * nk, hipMemcpyHostToDevice));
    }
    DescParams dp = {};
    dp.lmax = h->lmax; dp.nmax = h->nmax; dp.S = h->S; dp.N = 1; dp.Nall = 1; dp.first = 0; dp.stride = 1;
    dp.maxnn = 0; dp.Dc = h->Dc; dp.Dpad = h->Dpad; dp.CS = h->CS; dp.rc = h->rc;
    for (int k = 0; k < SGPR_MAX_S; k++) dp.radii_v[k] = k < h->S ? h->radii[k] : 1.0;
    if (launch_descriptor_forward_env(dp, d_ptr.p, d_eslot.p, d_er.p, h->d_radii.p, h->d_pack.p, d_p.p, d_norm.p, st))
        return fail(SGPR_E_UNSUPPORTED, "descriptor kernel not compiled in");
    // ---- its K_mm row: the SAME kernel and reduction order as the full K_mm product (row 0 of a 64-row panel)
    {
        std::vector<int> os(64, -2), on(64, 1);
        os[0] = s_new; on[0] = nk;
        HIPCHK(hipMemcpy(d_one_slot.p, os.data(), sizeof(int) * 64, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_one_nn.p, on.data(), sizeof(int) * 64, hipMemcpyHostToDevice));
        GemmParams g = {};
        g.M = 1; g.N = m_old; g.K = h->Dpad; g.lda = h->Dpad; g.ldb = h->Dpad; g.ldc = h->m_pad;
        g.A = d_p.p; g.B = h->d_Pm.p; g.C = d_krow.p; g.tiles = nullptr; g.bm = 64;
        g.eta = h->eta; g.lone_m1 = h->lone_w - 1.0; g.row_nn = d_one_nn.p; g.col_nn = h->d_ind_nn.p; g.row_slot = d_one_slot.p; g.col_slot = h->d_ind_slot.p;
        launch_gemm_nt(g, EPI_KERNEL, st);
        GemmParams g2 = g;  // k(x, x)
        g2.N = 1; g2.B = d_p.p; g2.C = d_kself.p; g2.ldc = 64; g2.col_nn = d_one_nn.p; g2.col_slot = d_one_slot.p;
        launch_gemm_nt(g2, EPI_KERNEL, st);
    }
    double kxx = 0.0;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(&kxx, d_kself.p, sizeof(double), hipMemcpyDeviceToHost));
    // ---- re-index every model array with the new row / column at `pos` = end of the species block
    const int pos = h->qoff[s_new + 1];
    const int m = m_old + 1, ld_old = h->m_pad, rows_old = h->m_rows;
    guard.armed = false;  // from here on the device arrays change shape: the list and they move together
    h->m = m; h->m_pad = rup(m, 32); h->m_rows = rup(m, 64);
    const int ld = h->m_pad;
    const int dpad64 = rup(h->Dpad, 64);
    int bad = 0;
    bad |= reindex_into(h, h->d_Pm, m_old, h->Dpad, h->Dpad, (size_t)h->m_rows * h->Dpad, h->Dpad, pos, -1, 0, st);
    bad |= reindex_into(h, h->d_PmT, h->Dpad, m_old, ld_old, (size_t)dpad64 * ld, ld, -1, pos, 0, st);
    bad |= reindex_into(h, h->d_M, m_old, m_old, ld_old, (size_t)h->m_rows * ld, ld, pos, pos, 0, st);
    bad |= reindex_into(h, h->d_pm_norm, 1, m_old, rows_old, (size_t)h->m_rows, h->m_rows, -1, pos, 0, st);
    // the cached factor follows while it has the current shape at ridge 0: every block moves with the re-indexing,
    // the new LCE's block is bordered if it was valid (else it is factored at the next solve), the others keep
    // their state
    const bool follow = h->chol_shape && h->chol_ridge == 0.0 && h->d_L.p && h->d_choli.p && (int)h->blk_ok.size() == h->S;
    const bool border = follow && h->blk_ok[s_new];
    if (follow) {
        bad |= reindex_into(h, h->d_L, m_old, m_old, ld_old, chol_count(h), ld, pos, pos, 0, st);
        bad |= reindex_into(h, h->d_choli, m_old, m_old, ld_old, chol_count(h), ld, pos, pos, 0, st);
        if (!border) { h->blk_ok[s_new] = 0; h->chol_valid = false; h->has_choli = false; }
    } else {
        h->chol_valid = false;
        h->chol_shape = false;
        h->has_choli = false;
        bad |= h->d_choli.alloc((size_t)h->m_rows * ld);
    }
    if (bad) return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
    HIPCHK(hipMemcpyAsync(h->d_Pm.p + (size_t)pos * h->Dpad, d_p.p, sizeof(double) * h->Dpad, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpy2DAsync(h->d_PmT.p + pos, sizeof(double) * ld, d_p.p, sizeof(double), sizeof(double), h->Dpad,
                            hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(h->d_pm_norm.p + pos, d_norm.p, sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(border_fill_kernel, dim3((m_old + 255) / 256), dim3(256), 0, st, m_old, pos, d_krow.p, kxx, h->d_M.p, ld);
    if (border) {
        const int b0 = h->qoff[s_new];
        hipLaunchKernelGGL(chol_border_kernel, dim3(1), dim3(256), sizeof(double) * std::max(pos - b0, 1), st, b0, pos, h->d_M.p,
                           h->chol_ridge, h->d_L.p, h->d_choli.p, ld, d_info.p);
        int info = 0;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(&info, d_info.p, sizeof(int), hipMemcpyDeviceToHost));
        if (info != 0) { h->chol_valid = false; h->has_choli = false; h->blk_ok[s_new] = 0; }  // not positive definite at ridge 0: the ladder next
        else h->chol_dmean = (h->chol_dmean * m_old + kxx) / m;
    }
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> slot_caller(m);
    for (int q = 0; q < m; q++) slot_caller[q] = slot_of(h, h->env_zc[q]);
    const int rc_ = edit_commit(h, slot_caller);
    return rc_ ? rc_ : design_after_add(h);
}

// dst[r][c] = src[rmap ? rmap[r] : r][cmap ? cmap[c] : c]
__global__ void gather2d_kernel(int rows, int cols, const double *src, int lds, double *dst, int ldd, const int *rmap,
                                const int *cmap)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (r >= rows || c >= cols) return;
    dst[(size_t)r * ldd + c] = src[(size_t)(rmap ? rmap[r] : r) * lds + (cmap ? cmap[c] : c)];
}

// gathered copy of a device array into the same buffer at its new padded shape (the old content parked in the
// handle's scratch, as reindex_into)
static int gather_into(sgpr_model *h, DevBuf<double> &buf, int rows_old, int ld_old, int rows_new, int cols_new, size_t new_count,
                       int ld_new, const int *rmap, const int *cmap, hipStream_t st)
{
    const size_t old_count = (size_t)rows_old * ld_old;
    if (h->d_edit_tmp.n < old_count) {
        (void)hipStreamSynchronize(st);
        if (h->d_edit_tmp.alloc(old_count + old_count / 4 + 4096, false)) return -1;
    }
    if (old_count && buf.p)
        (void)hipMemcpyAsync(h->d_edit_tmp.p, buf.p, sizeof(double) * old_count, hipMemcpyDeviceToDevice, st);
    if (buf.n < new_count || !buf.p) {
        (void)hipStreamSynchronize(st);
        if (buf.alloc(new_count + new_count / 8, false)) return -1;
    }
    (void)hipMemsetAsync(buf.p, 0, sizeof(double) * new_count, st);
    if (rows_new > 0 && cols_new > 0)
        hipLaunchKernelGGL(gather2d_kernel, dim3((cols_new + 255) / 256, rows_new), dim3(256), 0, st, rows_new, cols_new,
                           h->d_edit_tmp.p, ld_old, buf.p, ld_new, rmap, cmap);
    return 0;
}

static int qr_keep_select(sgpr_model *h, sgpr_model::QrKeep *k, int count, const int32_t *idx, const std::vector<int64_t> &new_ids);

// select_inducing (gppotential.py:1037-1046): the LCEs indices[0..count) of the current list, in that order, become
// the list — what downsize(lii=True) (:829-832: the `max_inducing` LCEs with the smallest K_mm row sums, in argsort
// order), popfirst_1inducing (:801-811) and the removal of an arbitrary LCE come down to.  The reference refits from
// scratch afterwards.  Here nothing is recomputed that survives:
//   * descriptors, K_mm, the resident design matrix: rows / columns gathered on the device;
//   * the K_mm factor: a species block whose surviving LCEs are a leading part of the old block in the old order
//     keeps its factor (the leading part of L is the factor of the leading part); any other block is re-factored
//     alone at the next solve (n_s^3 / 3 instead of m^3 / 3);
//   * the kept first-stage QR of [K | Y]: R1[:, idx] is triangularised again (an m x m problem) and its reflectors
//     join the kept chain (qr_keep_select) — not a new QR of the 10^5..10^6-row matrix.
extern "C" int sgpr_select_inducing(sgpr_model *h, int count, const int32_t *indices)
{
    if (!h || count < 0 || (count > 0 && !indices)) return fail(SGPR_E_INVALID, "sgpr_select_inducing: bad arguments");
    const int m = (int)h->env_zc.size();
    std::vector<int32_t> zc, nz;
    std::vector<int64_t> ptr(1, 0);
    std::vector<double> nr;
    std::vector<char> seen(std::max(m, 1), 0);
    bool distinct = true;
    for (int c = 0; c < count; c++) {
        const int q = indices[c];
        if (q < 0 || q >= m) return fail(SGPR_E_INVALID, "sgpr_select_inducing: index %d outside [0, %d)", q, m);
        if (seen[q]) distinct = false;
        seen[q] = 1;
        zc.push_back(h->env_zc[q]);
        const int64_t a = h->env_ptr[q], b = h->env_ptr[q + 1];
        nz.insert(nz.end(), h->env_z.begin() + a, h->env_z.begin() + b);
        nr.insert(nr.end(), h->env_r.begin() + 3 * a, h->env_r.begin() + 3 * b);
        ptr.push_back((int64_t)nz.size());
    }
    const bool incremental = distinct && count >= 1 && h->m == m && h->d_Pm.p && h->d_M.p && h->d_PmT.p && !getenv("SGPR_SELECT_REBUILD");
    if (!incremental) {
        // (an empty result, a repeated index: rebuilt from the environments; the resident matrix follows by a gather)
        for (auto &k : h->qr_keep) k.valid = false;
        int rc_ = design_select(h, count, indices);
        if (rc_) return rc_;
        h->design_hold = true;
        rc_ = sgpr_set_inducing(h, count, zc.data(), ptr.data(), nz.data(), nr.data());
        h->design_hold = false;
        return rc_;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    hipStream_t st = h->stream;
    // new sorted order: stable sort of the new caller list by species; src[k_new] = old sorted position
    std::vector<int> old_sorted_of(m);
    for (int k = 0; k < m; k++) old_sorted_of[h->ind_perm[k]] = k;
    std::vector<int> slot_caller(count), perm_n(count), src(count);
    for (int c = 0; c < count; c++) slot_caller[c] = slot_of(h, zc[c]);
    std::iota(perm_n.begin(), perm_n.end(), 0);
    std::stable_sort(perm_n.begin(), perm_n.end(), [&](int a, int b) { return slot_caller[a] < slot_caller[b]; });
    for (int k = 0; k < count; k++) src[k] = old_sorted_of[indices[perm_n[k]]];
    // which species blocks keep their factor: survivors = a leading part of the old block, in the old order
    std::vector<int> qoff_n(h->S + 1, 0);
    for (int c = 0; c < count; c++) qoff_n[slot_caller[c] + 1]++;
    for (int sp = 0; sp < h->S; sp++) qoff_n[sp + 1] += qoff_n[sp];
    const bool follow = h->chol_shape && h->chol_ridge == 0.0 && h->d_L.p && h->d_choli.p && (int)h->blk_ok.size() == h->S;
    std::vector<char> blk_n(h->S, 0);
    bool all_ok = follow;
    for (int sp = 0; sp < h->S; sp++) {
        bool lead = true;
        for (int k = qoff_n[sp]; k < qoff_n[sp + 1]; k++) lead = lead && src[k] == h->qoff[sp] + (k - qoff_n[sp]);
        blk_n[sp] = follow && h->blk_ok[sp] && lead;
        if (qoff_n[sp + 1] > qoff_n[sp] && !blk_n[sp]) all_ok = false;
    }
    DevBuf<int> &d_map = h->sc_sel_map;
    if (d_map.alloc(count, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
    HIPCHK(hipMemcpy(d_map.p, src.data(), sizeof(int) * count, hipMemcpyHostToDevice));
    // kept QR factorisations in step with the current columns follow; the others are dropped
    std::vector<int64_t> ids_n(count);
    const bool ids_ok = (int)h->col_ids.size() == m;
    for (int c = 0; c < count; c++) ids_n[c] = ids_ok ? h->col_ids[indices[c]] : h->next_id++;
    for (auto &k : h->qr_keep) {
        if (!k.valid) continue;
        if (!ids_ok || h->qr_keep_mode == 0 || k.ncols != m || k.col_ids != h->col_ids) { k.valid = false; continue; }
        const int rck = qr_keep_select(h, &k, count, indices, ids_n);
        if (rck) return rck;
    }
    int rc_ = design_select(h, count, indices);  // (installs the new column ids)
    if (rc_) {
        for (auto &k : h->qr_keep) k.valid = false;  // (the slots above already followed the selection: start over next refit)
        return rc_;
    }
    h->col_ids = ids_n;
    const int ld_old = h->m_pad, rows_old = h->m_rows;
    h->m = count; h->m_pad = rup(count, 32); h->m_rows = rup(count, 64);
    const int ld = h->m_pad, dpad64 = rup(h->Dpad, 64);
    int bad = 0;
    bad |= gather_into(h, h->d_Pm, m, h->Dpad, count, h->Dpad, (size_t)h->m_rows * h->Dpad, h->Dpad, d_map.p, nullptr, st);
    bad |= gather_into(h, h->d_PmT, h->Dpad, ld_old, h->Dpad, count, (size_t)dpad64 * ld, ld, nullptr, d_map.p, st);
    bad |= gather_into(h, h->d_M, m, ld_old, count, count, (size_t)h->m_rows * ld, ld, d_map.p, d_map.p, st);
    bad |= gather_into(h, h->d_pm_norm, 1, rows_old, 1, count, (size_t)h->m_rows, h->m_rows, nullptr, d_map.p, st);
    if (follow) {
        bad |= gather_into(h, h->d_L, m, ld_old, count, count, chol_count(h), ld, d_map.p, d_map.p, st);
        bad |= gather_into(h, h->d_choli, m, ld_old, count, count, chol_count(h), ld, d_map.p, d_map.p, st);
        h->blk_ok = blk_n;
        h->chol_valid = false;  // (also when every block survived: mean(diag K_mm), hence sigma, is recomputed)
        h->has_choli = all_ok;
    } else {
        h->chol_valid = false;
        h->chol_shape = false;
        h->has_choli = false;
        bad |= h->d_choli.alloc((size_t)h->m_rows * ld);
    }
    if (bad) return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    h->env_zc.swap(zc); h->env_z.swap(nz); h->env_ptr.swap(ptr); h->env_r.swap(nr);
    return edit_commit(h, slot_caller);
}

extern "C" int sgpr_remove_inducing(sgpr_model *h, int index)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_remove_inducing: bad arguments");
    const int m = (int)h->env_zc.size();
    if (index < 0) index += m;  // -1 = last (pop_1inducing, gppotential.py:782-791)
    if (index < 0 || index >= m) return fail(SGPR_E_INVALID, "sgpr_remove_inducing: index outside [0, %d)", m);
    if (index == m - 1 && m >= 2 && h->m == m && h->d_Pm.p && h->d_M.p) {
        // pop_1inducing (gppotential.py:782-791): the LCE added last is the last of its species block; deleting
        // its row / column leaves K_mm, L and L^-1 of the others as they are
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        drop_graph(h);
        hipStream_t st = h->stream;
        const int s_old = slot_of(h, h->env_zc[m - 1]);
        const int pos = h->qoff[s_old + 1] - 1;
        const int m_new = m - 1, ld_old = h->m_pad, rows_old = h->m_rows;
        h->m = m_new; h->m_pad = rup(m_new, 32); h->m_rows = rup(m_new, 64);
        const int ld = h->m_pad, dpad64 = rup(h->Dpad, 64);
        double kxx = 0.0;
        HIPCHK(hipMemcpy(&kxx, h->d_M.p + (size_t)pos * ld_old + pos, sizeof(double), hipMemcpyDeviceToHost));
        int bad = 0;
        bad |= reindex_into(h, h->d_Pm, m, h->Dpad, h->Dpad, (size_t)h->m_rows * h->Dpad, h->Dpad, pos, -1, 1, st);
        bad |= reindex_into(h, h->d_PmT, h->Dpad, m, ld_old, (size_t)dpad64 * ld, ld, -1, pos, 1, st);
        bad |= reindex_into(h, h->d_M, m, m, ld_old, (size_t)h->m_rows * ld, ld, pos, pos, 1, st);
        bad |= reindex_into(h, h->d_pm_norm, 1, m, rows_old, (size_t)h->m_rows, h->m_rows, -1, pos, 1, st);
        if (h->chol_shape && h->chol_ridge == 0.0 && h->d_L.p && h->d_choli.p) {
            // (the leading part of a block's factor is the factor of its leading part: every block keeps its state)
            bad |= reindex_into(h, h->d_L, m, m, ld_old, chol_count(h), ld, pos, pos, 1, st);
            bad |= reindex_into(h, h->d_choli, m, m, ld_old, chol_count(h), ld, pos, pos, 1, st);
            h->chol_dmean = (h->chol_dmean * m - kxx) / m_new;
        } else {
            h->chol_valid = false;
            h->chol_shape = false;
            h->has_choli = false;
            bad |= h->d_choli.alloc((size_t)h->m_rows * ld);
        }
        if (bad) return fail(SGPR_E_NODEVICE, "hipMalloc failed (inducing set edit)");
        h->env_zc.pop_back();
        h->env_z.resize((size_t)h->env_ptr[m - 1]);
        h->env_r.resize(3 * (size_t)h->env_ptr[m - 1]);
        h->env_ptr.pop_back();
        std::vector<int> slot_caller(m_new);
        for (int q = 0; q < m_new; q++) slot_caller[q] = slot_of(h, h->env_zc[q]);
        design_after_pop_last(h);
        return edit_commit(h, slot_caller);
    }
    std::vector<int32_t> keep;
    for (int q = 0; q < m; q++)
        if (q != index) keep.push_back(q);
    return sgpr_select_inducing(h, (int)keep.size(), keep.data());
}

// ---------------------------------------------------------------------------- k(loc, X) for one LCE
__global__ void local_k_kernel(int m, int Dpad, double eta, double lone_w, int loc_slot, int loc_nn, const double *p, const double *Pm,
                               const int *ind_slot, const int *ind_nn, double *out /*[m+1]: k(loc,X), k(loc,loc)*/)
{
    const int k = blockIdx.x;  // k == m -> the self term
    const double *q = k < m ? Pm + (size_t)k * Dpad : p;
    double s = 0.0;
    for (int e = threadIdx.x; e < Dpad; e += 64) s += p[e] * q[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const bool same = k == m || ind_slot[k] == loc_slot;
        const bool rl = loc_nn == 0, cl = k < m ? ind_nn[k] == 0 : rl;
        const double v = (!rl && !cl) ? pow(s, eta) : ((rl && cl) ? lone_w : 0.0);  // similarity.py:94-103
        out[k] = same ? v : 0.0;
    }
}

extern "C" int sgpr_kernel_local(sgpr_model *h, int32_t zc, int nn, const int32_t *nbr_z, const double *nbr_r,
                                 double *k_out, double *kxx_out)
{
    if (!h || nn < 0 || (nn > 0 && (!nbr_z || !nbr_r))) return fail(SGPR_E_INVALID, "sgpr_kernel_local: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const int slot = slot_of(h, zc);
    if (slot < 0) return fail(SGPR_E_SPECIES, "LCE: Z=%d is not in the species table", zc);
    std::vector<int> eslot(std::max(nn, 1), 0);
    std::vector<double> er(3 * (size_t)std::max(nn, 1), 0.0);
    {
        int kept = 0;
        for (int e = 0; e < nn; e++) {
            const int sl = slot_of(h, nbr_z[e]);
            if (sl < 0 && h->ignore_unknown) continue;  // descriptor/sesoap.py:343-346
            if (sl < 0) return fail(SGPR_E_SPECIES, "LCE: neighbour Z=%d is not in the species table", nbr_z[e]);
            eslot[kept] = sl;
            er[3 * kept] = nbr_r[3 * e]; er[3 * kept + 1] = nbr_r[3 * e + 1]; er[3 * kept + 2] = nbr_r[3 * e + 2];
            kept++;
        }
        nn = kept;
        nbr_r = er.data();
    }
    const int m = h->m;
    const int64_t ptr[2] = {0, nn};
    DevBuf<int64_t> d_ptr;
    DevBuf<int> d_eslot;
    DevBuf<double> d_er, d_p, d_norm, d_out;
    if (d_ptr.alloc(2, false) || d_eslot.alloc(std::max(nn, 1), false) || d_er.alloc(3 * (size_t)std::max(nn, 1), false) ||
        d_p.alloc(64 * (size_t)h->Dpad) || d_norm.alloc(64) || d_out.alloc(m + 1))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (local kernel)");
    HIPCHK(hipMemcpy(d_ptr.p, ptr, sizeof(ptr), hipMemcpyHostToDevice));
    if (nn > 0) {
        HIPCHK(hipMemcpy(d_eslot.p, eslot.data(), sizeof(int) * nn, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_er.p, nbr_r, sizeof(double) * 3 * nn, hipMemcpyHostToDevice));
    }
    DescParams dp = {};
    dp.lmax = h->lmax; dp.nmax = h->nmax; dp.S = h->S; dp.N = 1; dp.Nall = 1; dp.first = 0; dp.stride = 1;
    dp.maxnn = 0; dp.Dc = h->Dc; dp.Dpad = h->Dpad; dp.CS = h->CS; dp.rc = h->rc;
    for (int k = 0; k < SGPR_MAX_S; k++) dp.radii_v[k] = k < h->S ? h->radii[k] : 1.0;
    if (launch_descriptor_forward_env(dp, d_ptr.p, d_eslot.p, d_er.p, h->d_radii.p, h->d_pack.p, d_p.p, d_norm.p, h->stream))
        return fail(SGPR_E_UNSUPPORTED, "descriptor kernel not compiled in");
    hipLaunchKernelGGL(local_k_kernel, dim3(m + 1), dim3(64), 0, h->stream, m, h->Dpad, h->eta, h->lone_w, slot, nn, d_p.p,
                       h->d_Pm.p, h->d_ind_slot.p, h->d_ind_nn.p, d_out.p);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    std::vector<double> out(m + 1);
    HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * (m + 1), hipMemcpyDeviceToHost));
    for (int k = 0; k < m && k_out; k++) k_out[h->ind_perm[k]] = out[k];
    if (kxx_out) *kxx_out = out[m];
    d_ptr.release(); d_eslot.release(); d_er.release(); d_p.release(); d_norm.release(); d_out.release();
    return SGPR_OK;
}
