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
// Hills are rows in HBM indexed by CONFIGURATION (MdRun::meta_slot): the loop evaluates speculatively and discards what it
// evaluated behind a halt; an evaluation that is repeated or discarded overwrites its own row and nothing is rolled back.  The
// bias of configuration n sums the rows below its own.
//
// Layout of the launch: every workgroup computes the CVs and the sums over the hills — the same operations in the same order,
// so the same bits — and adds the bias forces of its own 256 atoms into Fself (the reverse pass has stored Fself of every atom
// of this step, one writer each, an atom without neighbours included: nothing accumulates from step to step).  Workgroup 0
// alone adds V into slot 0 of the energy partials and x (x) F into slot 0 of the nine virial partials (both stored by the
// step's earlier kernels, read by the last kernel's reducers) and stores the hill row.  No atomics, nothing depends on the
// order the workgroups run in.
//
// The merged form (sgpr_md_meta_merge(chunk = CH); workloads.meta_density(merge=) is the definition): the rows are still kept,
// and chunk j — the rows [j CH, (j + 1) CH) — is merged into a table of one entry per occupied bin (centre, the block key of the
// first row, the number of rows as a double) by md_meta_merge_kernel, enqueued in front of the bias of the first configuration n
// with slot(n) / CH > j.  Those rows are final there: a kernel of step n that runs un-halted has the positions of every
// configuration below n behind it.  The bias of configuration n sums the entries of the chunks below slot(n) — entry k in thread
// k % 256, partial sum (k / 256) % 4 — and then the rows [(slot(n) / CH) CH, slot(n)) — row B + r in thread r % 256, partial sum
// (r / 256) % 4 of the same accumulators —, so it is a function of n and the rows below it alone.  The covloss gate halts
// configuration k from the last kernel of step k + 1, whose merge, when k + 1 crosses a chunk, has run by then: the table is then
// one chunk ahead of the halted configuration, which is evaluated again.  Each entry therefore keeps what the last chunk added to
// it (last, stamp) and the table the entry count before that chunk: an evaluation that finds the table one chunk ahead takes
// the last chunk off again — integers in doubles, the same bits as a table that never held it.
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
// (the body of both forms of the bias: MERGED sums the table tb and then the rows behind its chunks, otherwise every row)
template <bool MERGED>
__device__ __forceinline__ void meta_eval(int N, const MetaPar &p, const double *x, const unsigned char *sel, double *centre, int *key,
                                          double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV, const MetaTab &tb)
{
#pragma clang fp contract(off)
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
    int hb = 0;   // the first row summed on its own
    if constexpr (MERGED) {
        // the entries of the chunks below this configuration: entry k adds cnt e and (cnt e) t_d
        int T = tb.ctl[META_CTL_T];
        const int done = tb.ctl[META_CTL_DONE];
        const bool ahead = done != tb.want;   // (the table holds one chunk more: the speculative step behind a halted configuration merged it)
        if (ahead) T = tb.ctl[META_CTL_TPREV];
        for (int k0 = tid; k0 < T; k0 += META_TRIP) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int k = k0 + 256 * u;
                if (k >= T) continue;
                const int *kh = tb.key + (size_t)D * k;
                bool near = true;
#pragma unroll
                for (int d = 0; d < META_MAXD; d++)
                    if (d < D) near = near && abs(kh[d] - kx[d]) <= 1;
                if (!near) continue;
                const double *ch = tb.centre + (size_t)D * k;
                double t[META_MAXD], d2 = 0.0;
#pragma unroll
                for (int d = 0; d < META_MAXD; d++) {
                    t[d] = 0.0;
                    if (d < D) t[d] = (c[d] - ch[d]) / p.sigma[d];
                    d2 = d2 + t[d] * t[d];
                }
                double n = tb.cnt[k];
                if (ahead && tb.stamp[k] == done - 1) n = n - tb.last[k];
                const double e = n * exp(-0.5 * d2);
                acc[u][0] += e;
#pragma unroll
                for (int d = 0; d < META_MAXD; d++) acc[u][1 + d] += e * t[d];
            }
        }
        hb = tb.want * tb.ch;
    }
    for (int h0 = hb + tid; h0 < nh; h0 += META_TRIP) {
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

// x: [N][3] positions of this configuration, sorted order; sel: [ncomp][N] bytes, sorted order (posvar: 1 = in sel and not the
// index atom); centre [cap][D], key [cap][D], rows [cap][7] = cv[6] | V; nh hills stand below this configuration; own: the row
// this configuration deposits (-1: none: n % pace != 0)
__global__ __launch_bounds__(256) void md_meta_kernel(int N, MetaPar p, const double *x, const unsigned char *sel, double *centre, int *key,
                                                      double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV,
                                                      const int *halt, int step)
{
    if (*halt < step) return;
    meta_eval<false>(N, p, x, sel, centre, key, rows, nh, own, Fself, Epart, virpart, nV, MetaTab());
}

// the merged form: the same launch in the same place of the step
__global__ __launch_bounds__(256) void md_meta_merged_kernel(int N, MetaPar p, const double *x, const unsigned char *sel, double *centre, int *key,
                                                             double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV,
                                                             MetaTab tb, const int *halt, int step)
{
    if (*halt < step) return;
    meta_eval<true>(N, p, x, sel, centre, key, rows, nh, own, Fself, Epart, virpart, nV, tb);
}

// Merges chunk j — the rows [j ch, (j + 1) ch) of centre / key — into the table: ONE workgroup.  Acts only when the table holds
// exactly the chunks below j, so that an enqueue that is repeated, or one behind a discarded one, changes nothing.  256 rows at
// a time, in row order: every row looks for its centre (by bits) among the entries that stand; the first row of each centre
// among the 256 is its leader and counts the rows equal to it; the leaders whose centre is new take the positions T + rank, the
// rank counted over the rows in row order — the order of first occurrence whatever the scheduling —; each leader is the one
// writer of its entry (no atomics; the counts are integers in doubles, exact in any order).
__global__ __launch_bounds__(256) void md_meta_merge_kernel(int D, int ch, int j, const double *centre, const int *key, MetaTab tb,
                                                            const int *halt, int step)
{
    if (*halt < step) return;
    __shared__ long long csh[256][META_MAXD];
    __shared__ int wnew[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int done = tb.ctl[META_CTL_DONE];
    int T = tb.ctl[META_CTL_T];
    __syncthreads();   // (every thread has read the words thread 0 writes on its way out)
    if (done != j) return;
    const int T0 = T;
    for (int r0 = 0; r0 < ch; r0 += 256) {
        const int nr = ch - r0 < 256 ? ch - r0 : 256;
        const bool live = tid < nr;
        const size_t h = (size_t)j * ch + r0 + (live ? tid : 0);
        long long cb[META_MAXD];
#pragma unroll
        for (int d = 0; d < META_MAXD; d++) {
            cb[d] = d < D ? __double_as_longlong(centre[(size_t)D * h + d]) : 0;
            csh[tid][d] = cb[d];
        }
        int m = -1;   // the entry that holds this row's centre
        if (live)
            for (int k = 0; k < T && m < 0; k++) {
                bool eq = true;
#pragma unroll
                for (int d = 0; d < META_MAXD; d++)
                    if (d < D) eq = eq && __double_as_longlong(tb.centre[(size_t)D * k + d]) == cb[d];
                if (eq) m = k;
            }
        __syncthreads();
        int first = -1;
        double n = 0.0;
        if (live)
            for (int r = 0; r < nr; r++) {
                bool eq = true;
#pragma unroll
                for (int d = 0; d < META_MAXD; d++) eq = eq && csh[r][d] == cb[d];
                if (eq) {
                    if (first < 0) first = r;
                    n += 1.0;
                }
            }
        const bool leader = live && first == tid, fresh = leader && m < 0;
        const unsigned long long b = __ballot(fresh);
        if (lane == 0) wnew[wave] = __popcll(b);
        __syncthreads();
        int pos = m;
        if (fresh) {
            pos = T + __popcll(b & ((1ull << lane) - 1ull));
            for (int q = 0; q < wave; q++) pos += wnew[q];
        }
        if (leader) {
            double old = 0.0, add = n;
            if (fresh) {
                for (int d = 0; d < D; d++) {
                    tb.centre[(size_t)D * pos + d] = __longlong_as_double(cb[d]);
                    tb.key[(size_t)D * pos + d] = key[(size_t)D * h + d];
                }
            } else {
                old = tb.cnt[pos];
                if (tb.stamp[pos] == j) add = tb.last[pos] + n;   // (an earlier 256 of this chunk)
            }
            tb.cnt[pos] = old + n;
            tb.last[pos] = add;
            tb.stamp[pos] = j;
        }
        T += (wnew[0] + wnew[1]) + (wnew[2] + wnew[3]);
        __syncthreads();   // (the new entries stand for the next 256 rows; csh and wnew are free)
    }
    if (tid == 0) {
        tb.ctl[META_CTL_TPREV] = T0;
        tb.ctl[META_CTL_T] = T;
        tb.ctl[META_CTL_DONE] = j + 1;
    }
}
