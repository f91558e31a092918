// md_meta.inc — metadynamics inside the device MD loop (sgpr_md_meta): the bias potential of the reference's
// calculator/meta.py (Meta over analysis/kde.py's Gaussian_kde), evaluated once per configuration between the reverse
// descriptor pass and the step's last kernel.  workloads.meta_bias is the host twin and the definition.
//
// Collective variables, concatenated like the reference's Catvar (D <= 6 over at most 4 components), from the raw coordinates
// the integrator holds (no minimum image, no wrapping — the reference's colvars read atoms.xyz):
//     distance(i, j)   |x_j - x_i|                                             one dimension
//     posvar(index, select)   x_index - (1/n) sum_{k in sel, k != index} x_k   three; n = |sel|, the index atom counted
// A hill deposited at c is centred at (floor(c / sigma) + 0.5) sigma and carries the key floor(c / (5 sigma)); the density at x
// sums exp(-|(x - centre) / sigma|^2 / 2) / (2 pi)^(D/2) over the hills whose key differs from floor(x / (5 sigma)) by at most
// one in every dimension.  V = w kde, or log(1 + w kde gamma) / gamma (well-tempered).
//
// Hills are rows in HBM indexed by CONFIGURATION (MdState::meta_slot): the loop evaluates speculatively and discards what it
// evaluated behind a halt; an evaluation that is repeated or discarded overwrites its own row and nothing is rolled back.  The
// bias of configuration n sums the rows below its own.
//
// Layout of the launch: every workgroup computes the CVs and the sums over the hills — the same operations in the same order,
// so the same bits — and adds the bias forces of its own 256 atoms into Fself (the reverse pass has stored Fself of every atom
// of this step, one writer each, an atom without neighbours included: nothing accumulates from step to step).  Workgroup 0
// alone adds V into slot 0 of the energy partials and x (x) F into slot 0 of the nine virial partials (both stored by the
// step's earlier kernels, read by the last kernel's reducers) and stores the hill row.  No atomics, nothing depends on the
// order the workgroups run in.
// sums of three values over the workgroup in a fixed order: fin_wave_sum per wave, the four waves as a pairwise tree
__device__ __forceinline__ void meta_block_sum3(double (&s)[3], double (*red)[4])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v = fin_wave_sum(s[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    __syncthreads();
}

// x: [N][3] positions of this configuration, sorted order; sel: [ncomp][N] bytes, sorted order (posvar: 1 = in sel and not the
// index atom); centre [cap][D], key [cap][D], rows [cap][7] = cv[6] | V; nh hills stand below this configuration; own: the row
// this configuration deposits (-1: none: n % pace != 0)
__global__ __launch_bounds__(256) void md_meta_kernel(int N, MetaPar p, const double *x, const unsigned char *sel, double *centre, int *key,
                                                      double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV,
                                                      const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double red[1 + META_MAXD][4];
    __shared__ double csh[META_MAXD], gsh[META_MAXD];   // (indexed by a running dimension: not registers)
    const int tid = threadIdx.x;
    // ---- the collective variables
    double dvec[META_MAXC][3], rlen[META_MAXC];
    int d0 = 0;
#pragma unroll
    for (int q = 0; q < META_MAXC; q++) {
        dvec[q][0] = dvec[q][1] = dvec[q][2] = 0.0;
        rlen[q] = 1.0;
        if (q >= p.ncomp) continue;
        const double *xi = x + 3 * (size_t)p.ia[q];
        if (p.kind[q] == 0) {
            const double *xj = x + 3 * (size_t)p.ib[q];
            for (int k = 0; k < 3; k++) dvec[q][k] = xj[k] - xi[k];
            rlen[q] = sqrt((dvec[q][0] * dvec[q][0] + dvec[q][1] * dvec[q][1]) + dvec[q][2] * dvec[q][2]);
            if (tid == 0) csh[d0] = rlen[q];
            d0 += 1;
        } else {
            double s[3] = {0.0, 0.0, 0.0};
            const unsigned char *sq = sel + (size_t)q * N;
            for (int k = tid; k < N; k += 256)
                if (sq[k]) { s[0] += x[3 * (size_t)k]; s[1] += x[3 * (size_t)k + 1]; s[2] += x[3 * (size_t)k + 2]; }
            meta_block_sum3(s, red);
            if (tid == 0)
                for (int k = 0; k < 3; k++) csh[d0 + k] = xi[k] - s[k] / p.nsel[q];
            d0 += 3;
        }
    }
    __syncthreads();
    const int D = p.D;
    double c[META_MAXD];
    int kx[META_MAXD];
#pragma unroll
    for (int d = 0; d < META_MAXD; d++) {
        c[d] = d < D ? csh[d] : 0.0;
        // (the key as an int: clamped to +-1e9 — a coordinate that far out, in units of 5 sigma, is beyond the scheme; sgpr_md_meta
        // clamps the keys of uploaded hills alike)
        kx[d] = d < D ? (int)fmin(fmax(floor(c[d] / p.sigma5[d]), -1e9), 1e9) : 0;
    }
    // ---- the sums over the hills: S = sum e, A_d = sum e t_d with t = (c - centre) / sigma.  Hill h belongs to thread h % 256 and
    // to its partial sum (h / 256) % 4: a fixed assignment, the same bits every run
    double acc[4][1 + META_MAXD];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int d = 0; d <= META_MAXD; d++) acc[u][d] = 0.0;
    for (int h0 = tid; h0 < nh; h0 += META_TRIP) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int h = h0 + 256 * u;
            if (h >= nh) continue;
            const int *kh = key + (size_t)D * h;   // (rows of D: a one-dimensional CV reads four bytes per hill, not twenty-four)
            bool near = true;
#pragma unroll
            for (int d = 0; d < META_MAXD; d++)
                if (d < D) near = near && abs(kh[d] - kx[d]) <= 1;
            if (!near) continue;
            const double *ch = centre + (size_t)D * h;
            double t[META_MAXD], d2 = 0.0;
#pragma unroll
            for (int d = 0; d < META_MAXD; d++) {
                t[d] = 0.0;
                if (d < D) t[d] = (c[d] - ch[d]) / p.sigma[d];
                d2 = d2 + t[d] * t[d];
            }
            const double e = exp(-0.5 * d2);
            acc[u][0] += e;
#pragma unroll
            for (int d = 0; d < META_MAXD; d++) acc[u][1 + d] += e * t[d];
        }
    }
    double S[1 + META_MAXD];
#pragma unroll
    for (int d = 0; d <= META_MAXD; d++) {
        const double v = fin_wave_sum((acc[0][d] + acc[1][d]) + (acc[2][d] + acc[3][d]));
        if ((tid & 63) == 0) red[d][tid >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d <= META_MAXD; d++) S[d] = (red[d][0] + red[d][1]) + (red[d][2] + red[d][3]);
    // ---- V and dV/dc
    const double kde = S[0] / p.norm;
    double V = p.w * kde, fac = p.w;
    if (p.wt) {
        const double a = 1.0 + V * p.gamma;
        V = log(a) / p.gamma;
        fac = p.w / a;
    }
    double g[META_MAXD];   // dV/dc_d = fac d kde / dc_d = -fac A_d / (sigma_d norm)
#pragma unroll
    for (int d = 0; d < META_MAXD; d++) g[d] = d < D ? -(fac * ((S[1 + d] / p.sigma[d]) / p.norm)) : 0.0;
    if (tid == 0)
#pragma unroll
        for (int d = 0; d < META_MAXD; d++) gsh[d] = g[d];
    __syncthreads();
    // ---- the bias forces of this workgroup's atoms, F = -dV/dx, added to the reverse pass's own sums
    const int i = blockIdx.x * 256 + tid;
    double f[3] = {0.0, 0.0, 0.0};
    bool touched = false;
    d0 = 0;
#pragma unroll
    for (int q = 0; q < META_MAXC; q++) {
        if (q >= p.ncomp) continue;
        if (p.kind[q] == 0) {
            // c = |x_j - x_i|: F_i = g (x_j - x_i) / c, F_j = -F_i
            if (i == p.ia[q] || i == p.ib[q]) {
                const double sgn = i == p.ia[q] ? 1.0 : -1.0;
                for (int k = 0; k < 3; k++) f[k] = f[k] + sgn * ((gsh[d0] * dvec[q][k]) / rlen[q]);
                touched = true;
            }
            d0 += 1;
        } else {
            // c = x_index - (1/n) sum x_k: F_index = -g, F_k = g / n
            if (i == p.ia[q]) {
                for (int k = 0; k < 3; k++) f[k] = f[k] - gsh[d0 + k];
                touched = true;
            } else if (i < N && sel[(size_t)q * N + i]) {
                for (int k = 0; k < 3; k++) f[k] = f[k] + gsh[d0 + k] / p.nsel[q];
                touched = true;
            }
            d0 += 3;
        }
    }
    if (touched && i < N)
        for (int k = 0; k < 3; k++) Fself[3 * (size_t)i + k] = Fself[3 * (size_t)i + k] + f[k];
    // ---- workgroup 0: energy, virial, the hill row
    if (blockIdx.x != 0 || tid != 0) return;
    Epart[0] = Epart[0] + V;
    // the last kernel's virial is sum r (x) dE/dr, the stress its Voigt part over the volume; the bias adds -sum_i x_i (x) F_i:
    // a distance contributes d (x) F_i (F_j = -F_i), a posvar c (x) g (the forces on sel sum to g, weighted with the positions)
    double vir[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    d0 = 0;
#pragma unroll
    for (int q = 0; q < META_MAXC; q++) {
        if (q >= p.ncomp) continue;
        if (p.kind[q] == 0) {
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) vir[3 * a + b] = vir[3 * a + b] + dvec[q][a] * ((gsh[d0] * dvec[q][b]) / rlen[q]);
            d0 += 1;
        } else {
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) vir[3 * a + b] = vir[3 * a + b] + csh[d0 + a] * gsh[d0 + b];
            d0 += 3;
        }
    }
    for (int q = 0; q < 9; q++) virpart[(size_t)q * nV] = virpart[(size_t)q * nV] + vir[q];
    if (own >= 0) {
        double *ch = centre + (size_t)D * own, *row = rows + (size_t)(META_MAXD + 1) * own;
        int *kh = key + (size_t)D * own;
        for (int d = 0; d < META_MAXD; d++) {
            if (d < D) {
                ch[d] = (floor(c[d] / p.sigma[d]) + 0.5) * p.sigma[d];
                kh[d] = kx[d];
            }
            row[d] = c[d];
        }
        row[META_MAXD] = V;
    }
}
