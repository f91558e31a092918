// bandqr.inc — Householder QR of a BANDED tall matrix, one launch per 32-column panel (included by tsqr.hip).
//
// The second stage of the regression (regression/gppotential.py:1255-1263 on the reduced system: mu = lstsq([R1; sigma L^T],
// [z; 0]), both blocks upper triangular, rows interleaved) is a 2m x m matrix whose column c is zero below row 2c + 1: panel k
// only touches the 32k + 64 rows [32k, 64k + 64) — at most 1056 at m = 1024.  The tree of 256-row chunks that the tall
// first-stage matrix needs (tsqr_panel: leaf, update, next level's leaf, ...) made such a factorisation a chain of ~170
// launches, 3.4 ms for 0.85 GF.  Here a panel's whole active row range sits in the REGISTERS of one 512-thread workgroup
// (wave w owns the columns w, w + 8, w + 16, w + 24; lane l the rows l, l + 64, ...: up to 17 per column), so a panel is ONE
// flat factorisation — no tree — and one launch does, per panel k:
//   workgroup 0      applies panel k - 1 (compact WY: V, T from the previous launch) to the 32 columns of panel k, factors
//                    them, leaves V_k, T_k for the next launch and R's diagonal block in the matrix;
//   workgroups 1..   apply panel k - 1 to the column blocks behind (and to the targets): the bulk of the trailing update
//                    runs beside the factorisation it does not depend on.
// m / 32 + 1 launches, no hand-offs inside a launch.  Also serves the other banded problems of the update path (energy rows on
// top of a triangular factor: band = 1 with an offset) while their panels stay within BQ_MAXR rows.
// Fixed order of every sum: the result repeats bit for bit.

#define BQT 512                   // threads per workgroup: 8 waves
#define BQ_SLOTS 17               // rows per lane and column
#define BQ_MAXR (64 * BQ_SLOTS)   // 1088 active rows at most
#define BQ_VLD BQ_MAXR            // leading dimension of a kept V (doubles per column)

struct BandStep {
    double *At;                   // column-major: element (row r, column c) at At[c * ldr + r]
    int ldr;
    int ncols_total;              // factored columns + targets + columns carried along
    int cols;                     // factored columns
    int k0, nb, r0, r1;           // this launch's panel: columns [k0, k0 + nb), active rows [r0, r1); nb = 0: none (the last launch)
    int pk0, pnb, pr0, pr1;       // the previous panel (pnb = 0: none)
    const double *Vp, *Tp;        // its V [32][BQ_VLD] (zero above the diagonal, v_jj on it; rows relative to pr0) and T [32][32]
    double *Vn, *Tn;              // this panel's
    size_t bs_mat, bs_work;       // batch (blockIdx.y): doubles between the problems' matrices / V, T scratch
    int dbg;                      // timing experiments (SGPR_BANDQR_DBG: 1 skip the trailing update, 2 skip the column steps — wrong results)
};

// A <- (I - V T V^T)^T A = A - V (T^T (V^T A)) for the columns [c0, c0 + nc) (nc <= 32) over the rows [pr0, pr1): eight
// waves, the rows dealt to the waves in slabs for W = V^T A (partial sums per wave, added in wave order), Z = T^T W by
// all threads, then A -= V Z in 16-row blocks, every product on v_mfma_f64_16x16x4.  Operands straight from global
// memory (L2: a panel's V is <= 280 KB, read by a few dozen workgroups at once).
__device__ __noinline__ void bq_apply(double *At, int ldr, int c0, int nc, int pr0, int pr1, const double *V, const double *T,
                                         double *lds)
{
    double *Wp = lds;                          // [8][32][33] partial W per wave
    double *Ws = Wp + 8 * 32 * 33;             // [32][33]
    double *Zs = Ws + 32 * 33;                 // [32][33]  (-Z)
    double *Ts = Zs + 32 * 33;                 // [32][33]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int np = pr1 - pr0;
    for (int e = tid; e < 32 * 32; e += BQT) Ts[(e >> 5) * 33 + (e & 31)] = T[e];
    // ---- W = V^T A: wave w takes the 4-row steps w, w + 8, ...
    {
        v4d acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // (i block, c block) = (0,0) (0,1) (1,0) (1,1)
        const int nsteps = (np + 3) / 4;
        const bool cok0 = l15 < nc, cok1 = 16 + l15 < nc;
        const double *a0 = At + (size_t)(c0 + (cok0 ? l15 : 0)) * ldr + pr0, *a1 = At + (size_t)(c0 + (cok1 ? 16 + l15 : 0)) * ldr + pr0;
        const double *v0 = V + (size_t)l15 * BQ_VLD, *v1 = V + (size_t)(16 + l15) * BQ_VLD;
        // (eight steps' operands requested before the first product: the loads are scattered 8-byte reads from L2, and a
        // step that waited for its own was one round trip per four multiply-adds)
        for (int s0 = wave; s0 < nsteps; s0 += 64) {
            double va0[8], va1[8], ab0[8], ab1[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int r = 4 * (s0 + 8 * u) + l4;
                const bool rok = r < np;       // (clamped index, masked value: no branch around a load)
                const int rr = rok ? r : 0;
                va0[u] = v0[rr]; va1[u] = v1[rr]; ab0[u] = a0[rr]; ab1[u] = a1[rr];
                if (!rok) { va0[u] = 0.0; va1[u] = 0.0; }
                if (!(rok && cok0)) ab0[u] = 0.0;
                if (!(rok && cok1)) ab1[u] = 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(va0[u], ab0[u], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(va0[u], ab1[u], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(va1[u], ab0[u], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(va1[u], ab1[u], acc[3], 0, 0, 0);
            }
        }
        // C/D layout: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                Wp[(wave * 32 + (t >> 1) * 16 + l4 + 4 * reg) * 33 + (t & 1) * 16 + l15] = acc[t][reg];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += BQT) {
        const int i = e >> 5, c = e & 31;
        double s = Wp[i * 33 + c];
#pragma unroll
        for (int w = 1; w < 8; w++) s += Wp[(w * 32 + i) * 33 + c];
        Ws[i * 33 + c] = s;
    }
    __syncthreads();
    // ---- -Z[i][c] = -sum_l T[l][i] W[l][c]
    for (int e = tid; e < 32 * 32; e += BQT) {
        const int i = e >> 5, c = e & 31;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < 32; l++) s4[l & 3] += Ts[l * 33 + i] * Ws[l * 33 + c];
        Zs[i * 33 + c] = -((s4[0] + s4[1]) + (s4[2] + s4[3]));
    }
    __syncthreads();
    // ---- A[r][c] += sum_i V[r][i] (-Z)[i][c]: 16-row blocks dealt to the waves
    {
        const int nblk = (np + 15) / 16;
        const bool cok[2] = {l15 < nc, 16 + l15 < nc};
        // two row blocks per trip, every operand of both requested before the first product
        for (int rb0 = wave; rb0 < nblk; rb0 += 16) {
            v4d acc[2][2];
            double va[2][8];
            double *ac[2][2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int rbase = 16 * (rb0 + 8 * u);
                const bool bok = rbase < np;
                const int rv = (bok && rbase + l15 < np) ? rbase + l15 : 0;
#pragma unroll
                for (int k = 0; k < 8; k++) va[u][k] = V[(size_t)(4 * k + l4) * BQ_VLD + rv];
#pragma unroll
                for (int cb = 0; cb < 2; cb++) {
                    ac[u][cb] = At + (size_t)(c0 + (cok[cb] ? 16 * cb + l15 : 0)) * ldr + pr0 + (bok ? rbase : 0);
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int r = l4 + 4 * reg;
                        acc[u][cb][reg] = ac[u][cb][(bok && rbase + r < np) ? r : 0];
                    }
                }
                if (!(bok && rbase + l15 < np)) {
#pragma unroll
                    for (int k = 0; k < 8; k++) va[u][k] = 0.0;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double z0 = Zs[(4 * k + l4) * 33 + l15], z1 = Zs[(4 * k + l4) * 33 + 16 + l15];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    acc[u][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][k], z0, acc[u][0], 0, 0, 0);
                    acc[u][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][k], z1, acc[u][1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int rbase = 16 * (rb0 + 8 * u);
#pragma unroll
                for (int cb = 0; cb < 2; cb++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int r = l4 + 4 * reg;
                        if (cok[cb] && rbase + r < np) ac[u][cb][r] = acc[u][cb][reg];
                    }
            }
        }
    }
    __syncthreads();
}

template <int NS>   // row slots per lane and column: panels of up to 64 NS rows
__global__ __launch_bounds__(BQT) void band_qr_step_kernel(BandStep q)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    q.At += blockIdx.y * q.bs_mat;
    q.Vp += blockIdx.y * q.bs_work; q.Tp += blockIdx.y * q.bs_work;
    q.Vn += blockIdx.y * q.bs_work; q.Tn += blockIdx.y * q.bs_work;
    // column block of this workgroup: block 0 = the panel (when there is one), then the blocks behind it
    const bool panel = q.nb > 0 && blockIdx.x == 0;
    const int cbeg = panel ? q.k0 : q.k0 + q.nb + 32 * ((int)blockIdx.x - (q.nb > 0 ? 1 : 0));   // (k0 = cols in the last launch)
    const int nc = panel ? q.nb : min(32, q.ncols_total - cbeg);
    if (nc <= 0) return;
    if (q.pnb > 0 && !(q.dbg & 1)) bq_apply(q.At, q.ldr, cbeg, nc, q.pr0, q.pr1, q.Vp, q.Tp, lds);
    if (!panel) return;
    // ---- the panel: columns [k0, k0 + nb) over the rows [r0, r1), in registers
    double *vbuf = lds;                        // [2][BQ_MAXR]
    double *G = vbuf + 2 * BQ_MAXR;            // [32][33]   V^T V (c < j filled as the factorisation goes)
    double *Ts = G + 32 * 33;                  // [32][33]
    double *Xs = Ts + 32 * 33;                 // [16][16]
    __shared__ double s_alpha[32], s_scal[32], s_vjj[32], sscal[2];
    const int nr = q.r1 - q.r0;
    double a[4][NS];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cc = wv + 8 * i;
        const double *col = q.At + (size_t)(q.k0 + (cc < q.nb ? cc : 0)) * q.ldr + q.r0;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            const int r = ln + 64 * k;
            a[i][k] = col[r < nr ? r : 0];     // (clamped index, masked value)
            if (!(cc < q.nb && r < nr)) a[i][k] = 0.0;
        }
    }
    for (int e = tid; e < 32 * 33; e += BQT) { G[e] = 0.0; Ts[e] = 0.0; }
    if (tid < 32) { s_alpha[tid] = 0.0; s_scal[tid] = 0.0; s_vjj[tid] = 0.0; }
    double rsave[4] = {0.0, 0.0, 0.0, 0.0};    // row < c of column c (the R entries above the diagonal): slot 0 of lanes < c
    // v . x over the lane's NS rows on two accumulators (a single chain of NS dependent multiply-adds was a fifth of a step)
    auto dot = [&](const double (&v)[NS], const double (&x)[NS]) {
        double g0 = 0.0, g1 = 0.0;
#pragma unroll
        for (int k = 0; k < NS; k += 2) {
            g0 += v[k] * x[k];
            if (k + 1 < NS) g1 += v[k + 1] * x[k + 1];
        }
        return g0 + g1;
    };
    // column j of its owner wave becomes v_j: published with 2 / v.v, the scalars kept for T and R
    auto publish = [&](int j, double (&col)[NS], double &keep_r) {
        const int jb = j & 1;
        keep_r = col[0];                       // (lanes < j hold R[lane][j]; the others are overwritten below anyway)
        if (ln < j) col[0] = 0.0;              // zero above the diagonal (only slot 0 can be: j < 32)
        const double s2 = wave_sum64(dot(col, col));
        const double akk = lane_f64(col[0], j);
        double nrm = 0.0, sc = 0.0;
        if (s2 > TSQR_TINY2) {                 // (rank-deficient panels: tsqr_leaf_kernel)
            double rs = __builtin_amdgcn_rsq(s2);
            rs = rs * (1.5 - 0.5 * s2 * rs * rs);
            nrm = s2 * rs;
            nrm = nrm + 0.5 * rs * (s2 - nrm * nrm);
            const double d = nrm * (nrm + fabs(akk));
            double rd = __builtin_amdgcn_rcp(d);
            rd = rd * (2.0 - d * rd);
            sc = rd * (2.0 - d * rd);
        }
        const double alpha = akk > 0.0 ? -nrm : nrm;
        const double vjj = akk - alpha;
        if (ln == j) col[0] = vjj;
#pragma unroll
        for (int k = 0; k < NS; k++) vbuf[jb * BQ_MAXR + ln + 64 * k] = col[k];
        if (ln == 0) { sscal[jb] = sc; s_alpha[j] = alpha; s_scal[j] = sc; s_vjj[j] = vjj; }
    };
    __syncthreads();
    if (wv == 0) publish(0, a[0], rsave[0]);
    __syncthreads();
    for (int j = 0; j < ((q.dbg & 2) ? 1 : q.nb); j++) {
        const int jb = j & 1;
        const double sc = sscal[jb];
        double vj[NS];                         // v_j: one LDS read per slot and step
#pragma unroll
        for (int k = 0; k < NS; k++) vj[k] = vbuf[jb * BQ_MAXR + ln + 64 * k];
        // the NEXT pivot column first: its owner updates it and publishes v_(j+1) while the others are busy with step j
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (wv + 8 * i == j + 1 && j + 1 < q.nb) {   // (wave-uniform)
                const double f = sc * wave_sum64(dot(vj, a[i]));
#pragma unroll
                for (int k = 0; k < NS; k++) a[i][k] -= f * vj[k];
                publish(j + 1, a[i], rsave[i]);
            }
        }
        // the other columns of this wave, side by side: four independent products and reductions in straight-line code
        // (the compiler interleaves their chains), then what each is for: a column still to come is reflected, a finished
        // reflector's product v_c . v_j goes to T (off the critical path)
        double g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = dot(vj, a[i]);
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = wave_sum64(g[i]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int cc = wv + 8 * i;
            if (cc > j + 1 && cc < q.nb) {               // (wave-uniform)
                const double f = sc * g[i];
#pragma unroll
                for (int k = 0; k < NS; k++) a[i][k] -= f * vj[k];
            } else if (cc < j && ln == 0) {
                G[j * 33 + cc] = g[i];
                G[cc * 33 + j] = g[i];
            }
        }
        __syncthreads();
    }
    // ---- V out (zero above the diagonal, v_jj on it; registers already hold it), R's diagonal block into the matrix
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cc = wv + 8 * i;
        double *Vc = q.Vn + (size_t)cc * BQ_VLD;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            const int r = ln + 64 * k;
            Vc[r] = (cc < q.nb && r < nr) ? a[i][k] : 0.0;
        }
        if (cc < q.nb && ln <= cc) q.At[(size_t)(q.k0 + cc) * q.ldr + q.r0 + ln] = ln == cc ? s_alpha[cc] : rsave[i];
    }
    // ---- T = [T11 T12; 0 T22] in 16 x 16 blocks (as tsqr_leaf_wave_kernel)
    if (tid < 32) {
        const int t = tid & 15, base = tid & 16;
        double Tr[16];
#pragma unroll
        for (int l = 0; l < 16; l++) Tr[l] = l == t ? s_scal[base + t] : 0.0;
#pragma unroll
        for (int j = 1; j < 16; j++) {
            double s2[2] = {0.0, 0.0};
#pragma unroll
            for (int l = 0; l < j; l++) s2[l & 1] += Tr[l] * G[(base + j) * 33 + base + l];
            const double v = -s_scal[base + j] * (s2[0] + s2[1]);
            if (j > t) Tr[j] = v;
        }
#pragma unroll
        for (int l = 0; l < 16; l++) Ts[(base + t) * 33 + base + l] = Tr[l];
    }
    __syncthreads();
    {
        const int ia = (tid >> 4) & 15, ib = tid & 15;
        if (tid < 256) {
            double x = 0.0;
#pragma unroll
            for (int l = 0; l < 16; l++) x += G[ia * 33 + 16 + l] * Ts[(16 + l) * 33 + 16 + ib];
            Xs[ia * 16 + ib] = x;
        }
        __syncthreads();
        if (tid < 256) {
            double y = 0.0;
#pragma unroll
            for (int l = 0; l < 16; l++) y += Ts[ia * 33 + l] * Xs[l * 16 + ib];
            Ts[ia * 33 + 16 + ib] = -y;
        }
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += BQT) q.Tn[e] = Ts[(e >> 5) * 33 + (e & 31)];
}

static size_t band_qr_lds_bytes() { return sizeof(double) * (8 * 32 * 33 + 3 * 32 * 33 + 64); }
static size_t band_qr_work_doubles() { return 2 * ((size_t)32 * BQ_VLD + 32 * 32); }

// rows x cols banded least squares (column c zero below row band (c + 1) + band_off) on the flat-panel kernel; -2 when a
// panel would not fit (the caller takes the tree form).  `x`: solution by back substitution (null: factor only);
// `extra` columns behind the targets are carried along.  batch problems side by side (blockIdx.y).
static int launch_band_qr(int rows, int cols, double *At, int ldr, double *x, double *work, hipStream_t st, int band, int band_off,
                          int extra, int batch, size_t bs_mat, size_t bs_work, double *keepVT = nullptr /*[panels][band_qr_keep_stride()]: V, T of every panel stay*/)
{
    if (band <= 0) return -2;
    if (cols > QR_MAX_COLS) return -1;   // the back substitution's right-hand side lives in LDS (backsolve_attr)
    for (int k0 = 0; k0 < cols; k0 += 32) {
        const int nb = std::min(32, cols - k0);
        const int row_end = std::min(rows, band * (k0 + nb) + band_off);
        if (row_end - k0 > BQ_MAXR || row_end - k0 < nb) return -2;
    }
    static bool attr = false;
    if (!attr) {
        const void *fn[] = {(const void *)band_qr_step_kernel<2>, (const void *)band_qr_step_kernel<4>, (const void *)band_qr_step_kernel<6>,
                            (const void *)band_qr_step_kernel<9>, (const void *)band_qr_step_kernel<13>, (const void *)band_qr_step_kernel<17>};
        for (auto f : fn) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)band_qr_lds_bytes());
        attr = true;
    }
    const size_t half = (size_t)32 * BQ_VLD + 32 * 32;
    static const int dbg = getenv("SGPR_BANDQR_DBG") ? atoi(getenv("SGPR_BANDQR_DBG")) : 0;
    BandStep q = {};
    q.dbg = dbg;
    q.At = At; q.ldr = ldr; q.ncols_total = cols + 1 + extra; q.cols = cols;
    q.bs_mat = bs_mat; q.bs_work = bs_work;
    int par = 0;
    for (int k0 = 0;; k0 += 32) {
        const bool last = k0 >= cols;
        q.k0 = last ? cols : k0; q.nb = last ? 0 : std::min(32, cols - k0);
        q.r0 = k0; q.r1 = last ? k0 : std::min(rows, band * (k0 + q.nb) + band_off);
        q.Vn = keepVT ? keepVT + (size_t)(k0 / 32) * half : work + (size_t)par * half;
        q.Tn = q.Vn + (size_t)32 * BQ_VLD;
        const int nblocks = (q.nb > 0 ? 1 : 0) + (q.ncols_total - (q.k0 + q.nb) + 31) / 32;
        if (nblocks > 0 && (q.nb > 0 || q.pnb > 0)) {
            const int ns = (q.r1 - q.r0 + 63) / 64;   // row slots the panel needs: the smallest instantiation that holds them
            const dim3 grid(nblocks, batch), blk(BQT);
            const size_t lb = band_qr_lds_bytes();
            if (ns <= 2) hipLaunchKernelGGL(band_qr_step_kernel<2>, grid, blk, lb, st, q);
            else if (ns <= 4) hipLaunchKernelGGL(band_qr_step_kernel<4>, grid, blk, lb, st, q);
            else if (ns <= 6) hipLaunchKernelGGL(band_qr_step_kernel<6>, grid, blk, lb, st, q);
            else if (ns <= 9) hipLaunchKernelGGL(band_qr_step_kernel<9>, grid, blk, lb, st, q);
            else if (ns <= 13) hipLaunchKernelGGL(band_qr_step_kernel<13>, grid, blk, lb, st, q);
            else hipLaunchKernelGGL(band_qr_step_kernel<17>, grid, blk, lb, st, q);
        }
        if (last) break;
        q.pk0 = q.k0; q.pnb = q.nb; q.pr0 = q.r0; q.pr1 = q.r1;
        q.Vp = q.Vn; q.Tp = q.Tn;
        par ^= 1;
    }
    if (x) backsolve_attr();
    if (x) hipLaunchKernelGGL(qr_backsolve_kernel, dim3(batch), dim3(1024), sizeof(double) * cols, st, cols, At, ldr, At + (size_t)cols * ldr, x, bs_mat);
    return 0;
}

// ---- a kept banded factorisation asked about one more column (bandqr keep: sgpr_internal.h::launch_band2_*)
// The second stage of an inducing TRIAL (add_1inducing, regression/gppotential.py:955-982: add, refit, measure, usually pop)
// is the second stage of the model before it with ONE more column: [R1 r; sigma L^T l] has the old 2m x m matrix in its
// first m columns and two new rows that are zero there.  So the kept reflectors of the old factorisation are applied to
// the new column and to the targets (32 panels, two columns: one workgroup walks through them), ONE more reflector
// zeroes the new column below its diagonal, and the back substitution runs on [R2 r'; 0 rho] — O(m^2) instead of the
// 33 launches of a factorisation.  W: [2][ldw] — column 0 the new matrix column (zero when there is none), column 1 the
// targets, both over 2 (m_old + nnew) interleaved rows.  x: [m_old + nnew].
struct BandAppend {
    double *W; int ldw;
    int m_old, nnew;
    const double *VT;          // kept panels
    size_t stride;             // doubles per panel in VT
    double *rhs;               // [m_old] out: what the back substitution on the kept R2 solves for
    double *x;                 // [m_old + nnew]: x[m_old] is set here
};

// bq_apply for TWO columns (a0, a1 over the rows [pr0, pr1) of a work array): the tile machinery of bq_apply took 38 us per
// panel for them; what two columns need is 64 dot products (four reflectors per wave, coalesced rows, eight independent
// wave reductions), a 32 x 32 by 32 x 2 product and one pass over the rows.
__device__ __forceinline__ void bq_apply_vec2(double *a0, double *a1, int pr0, int pr1, const double *V, const double *T, double *ws /*[2][32]*/,
                                              double *zs /*[2][32]*/)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int np = pr1 - pr0;
    double acc[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int r = lane; r < np; r += 64) {
        const double x0 = a0[pr0 + r], x1 = a1[pr0 + r];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const double v = V[(size_t)(4 * wave + u) * BQ_VLD + r];
            acc[u][0] += v * x0;
            acc[u][1] += v * x1;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { acc[u][0] = wave_sum64(acc[u][0]); acc[u][1] = wave_sum64(acc[u][1]); }
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < 4; u++) { ws[4 * wave + u] = acc[u][0]; ws[32 + 4 * wave + u] = acc[u][1]; }
    }
    __syncthreads();
    if (tid < 64) {   // z[c][i] = sum_l T[l][i] w[c][l]
        const int i = tid & 31, c = tid >> 5;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < 32; l++) s4[l & 3] += T[l * 32 + i] * ws[32 * c + l];
        zs[32 * c + i] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    __syncthreads();
    for (int r = tid; r < np; r += BQT) {
        double s0[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const double v = V[(size_t)i * BQ_VLD + r];
            s0[i & 1] += v * zs[i];
            s1[i & 1] += v * zs[32 + i];
        }
        a0[pr0 + r] -= s0[0] + s0[1];
        a1[pr0 + r] -= s1[0] + s1[1];
    }
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(BQT) void band_qr_append_kernel(BandAppend q)
{
    extern __shared__ double lds[];
    __shared__ double red[8], sh[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = q.m_old, R = 2 * m;
    for (int k0 = 0; k0 < m; k0 += 32) {
        const int nb = min(32, m - k0);
        const double *V = q.VT + (size_t)(k0 / 32) * q.stride;
        bq_apply_vec2(q.W, q.W + q.ldw, k0, min(R, 2 * (k0 + nb)), V, V + (size_t)32 * BQ_VLD, lds, lds + 64);
    }
    double *a = q.W, *y = q.W + q.ldw;
    double xm = 0.0;
    if (q.nnew) {
        // one reflector over the rows [m, 2m + 2) of the new column; what it does to the targets' entry of row m
        const int n = R + 2 - m;
        double s2 = 0.0, vy = 0.0;
        for (int i = tid; i < n; i += BQT) { const double v = a[m + i]; s2 += v * v; vy += v * y[m + i]; }
        s2 = wave_sum64(s2);
        if (lane == 0) red[wave] = s2;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < 8; w++) t += red[w];
            const double akk = a[m];
            const double nrm = sqrt(t);
            const double alpha = akk > 0.0 ? -nrm : nrm;
            const double v0 = akk - alpha;
            const double vv = t - akk * akk + v0 * v0;
            sh[0] = alpha; sh[1] = v0; sh[2] = vv > TSQR_TINY2 ? 2.0 / vv : 0.0; sh[3] = akk;
        }
        __syncthreads();
        // v . y with v_0 in place of a[m]
        vy = wave_sum64(vy);
        if (lane == 0) red[wave] = vy;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < 8; w++) t += red[w];
            t += (sh[1] - sh[3]) * y[m];                  // (the sum above took a[m] for v_0)
            const double ym = y[m] - sh[2] * t * sh[1];   // (H y)[row m]
            const double rho = sh[0];
            sh[0] = rho != 0.0 ? ym / rho : 0.0;
            q.x[m] = sh[0];
        }
        __syncthreads();
        xm = sh[0];
    }
    for (int i = tid; i < m; i += BQT) q.rhs[i] = y[i] - (q.nnew ? a[i] * xm : 0.0);
}

size_t band_qr_keep_stride() { return (size_t)32 * BQ_VLD + 32 * 32; }
size_t band_qr_keep_doubles(int cols) { return (size_t)((cols + 31) / 32) * band_qr_keep_stride(); }

// the banded 2m x m second stage with its reflectors kept (-2: the flat-panel form does not take this shape)
int launch_band2_keep(int rows, int cols, double *At, int ldr, double *x, double *work, double *keepVT, hipStream_t st)
{
    if (!band_qr_on()) return -2;
    return launch_band_qr(rows, cols, At, ldr, x, work, st, 2, 0, 0, 1, 0, 0, keepVT);
}

// ... asked about the targets in W column 1 and, with nnew = 1, the new column in W column 0; At_kept: the factored matrix
// launch_band2_keep left (its upper triangle is R2).  tmp: [m_old] doubles.
int launch_band2_append(int m_old, int nnew, double *W, int ldw, const double *keepVT, const double *At_kept, int ldr_kept, double *x,
                        double *tmp, hipStream_t st)
{
    if (m_old > QR_MAX_COLS) return -1;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void *)band_qr_append_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)band_qr_lds_bytes());
        attr = true;
    }
    BandAppend q = {};
    q.W = W; q.ldw = ldw; q.m_old = m_old; q.nnew = nnew; q.VT = keepVT; q.stride = band_qr_keep_stride(); q.rhs = tmp; q.x = x;
    hipLaunchKernelGGL(band_qr_append_kernel, dim3(1), dim3(BQT), band_qr_lds_bytes(), st, q);
    backsolve_attr();
    hipLaunchKernelGGL(qr_backsolve_kernel, dim3(1), dim3(1024), sizeof(double) * m_old, st, m_old, At_kept, ldr_kept, tmp, x);
    return 0;
}
