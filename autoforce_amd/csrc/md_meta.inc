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

// ---- kind 2: qlvar(index, j, cutoff, l...) — the Steinhardt bond-order parameters Q_l of the atom `index` over its neighbours t
// of species j with r_t < cutoff, r_t = x_j - x_index + shift.cell from THIS step's list (the forward pass has written it, sorted by
// (atom, image)); weights w_t = (1 - r_t / cutoff)^2, W = sum w_t.  By the addition theorem
//     Q_l^2 = (1 / W^2) sum_{t,t'} w_t w_t' P_l(u_t . u_t'),   u = r / |r|
// with P_l and P_l' from the three-term recurrence: no Y_lm, no pole on the z axis, any l.  workloads.meta_bias is the definition.
// Like the reference's Ylm, the directions u are those of the environment sheared by 1e-2 when a selected neighbour lies inside the
// cone around the z axis (workloads.ql_rows; ylm.py:10-23) — the lengths in the weights are not.
// Departures from the reference (calculator/meta.py's Qlvar over descriptor/ql.py): an empty environment gives Q_l = 0 with no
// gradient (the reference: NaN), and where Q_l = 0 the gradient is 0 (the reference: NaN, which its nan_to_num zeroes).
//   The selected neighbours are compacted into LDS by ballot, in list order; those of the components stand one behind the other
// and row k of them all belongs to thread k (META_QL_MAXT rows).  For each dimension the pair sums of row t,
//     A_t = sum_t' w_t' P_l(c),   B_t = sum_t' w_t' P_l'(c) (u_t' - c u_t),   c = u_t . u_t',
// are formed by K = min(64, 256 / T rounded up to a power of two) neighbouring lanes: lane k adds t' = k, k + K, ... one after
// the other and the K partial sums meet in a butterfly (lanes ^ 1, ^ 2, ...: every lane ends with the same bits); S = sum w_t A_t
// and W in fin_wave_sum's tree over the workgroup.  Thread t keeps dQ_d / dr_t of its row in registers until the hills have given
// g_d = dV/dQ_d, then leaves G_t = sum_d g_d dQ_d / dr_t in LDS: atom j_t takes -G_t once per image it stands under, in list
// order, the index atom the sum over the rows of other atoms (its own images cancel: they count in the virial only), and the
// virial takes sum_t r_t (x) G_t.
struct MetaQlLds {
    double r[META_QL_MAXT][3], rh[META_QL_MAXT][3];  // r_t, r_t / |r_t|
    double u[META_QL_MAXT][3];                       // v_t / |v_t|: the direction the harmonics see (v: r, or r sheared)
    double w[META_QL_MAXT][3];                       // w_t, dw_t / dr_t, |v_t| (while the rows are gathered: |r_t|)
    double eps[META_MAXC];                           // the shear of the component (0: none)
    double row[META_QL_MAXT][4];                     // A_t | B_t of the dimension at hand
    double g[META_QL_MAXT][3];                       // G_t
    int j[META_QL_MAXT];
    int cnt[4], base[META_MAXC], T[META_MAXC];
};
__device__ __forceinline__ MetaQlLds &meta_ql_lds()
{
    __shared__ MetaQlLds s;
    return s;
}

// compacts the environment of component q behind the `base` rows that stand; returns its length (every thread the same)
__device__ __forceinline__ int meta_ql_gather(const MetaQl &ql, int q, int ia, const double *x, MetaQlLds &s, int base)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nn = min(ql.nn[ia], ql.maxnn);
    const double *xi = x + 3 * (size_t)ia, *h = ql.cell;
    const double cut = ql.cut[q];
    int T = 0;
    bool near = false;
    for (int c0 = 0; c0 < nn; c0 += 256) {
        const int t = c0 + tid;
        bool hit = false;
        double r[3] = {0.0, 0.0, 0.0}, len = 1.0;
        int j = 0;
        if (t < nn) {
            const size_t e = (size_t)ia * ql.maxnn + t;
            const int code = ql.nbr_code[e];
            j = ql.nbr_j[e];
            if (((code >> 24) & 0xff) == ql.slot[q]) {
                const double s0 = (double)(int)(int8_t)(code & 0xff), s1 = (double)(int)(int8_t)((code >> 8) & 0xff),
                             s2 = (double)(int)(int8_t)((code >> 16) & 0xff);
                for (int k = 0; k < 3; k++) r[k] = (x[3 * (size_t)j + k] - xi[k]) + ((s0 * h[k] + s1 * h[3 + k]) + s2 * h[6 + k]);
                len = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
                hit = len < cut;
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s.cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = base + T + __popcll(m & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; v++) pos += s.cnt[v];
        if (hit && pos < META_QL_MAXT) {
            for (int k = 0; k < 3; k++) s.r[pos][k] = r[k];
            s.w[pos][2] = len;
            s.j[pos] = j;
            const double tol = META_QL_TINY_ANGLE * fabs(r[2]);
            near = near || (fabs(r[0]) < tol && fabs(r[1]) < tol);
        }
        T += (s.cnt[0] + s.cnt[1]) + (s.cnt[2] + s.cnt[3]);
        __syncthreads();
    }
    T = min(T, META_QL_MAXT - base);
    // the reference's Ylm shears the whole environment when one neighbour lies inside the cone around the z axis (ylm.py:10-23):
    // v = (x, y - eps z, eps y + z); the weights keep the lengths as they are
    const double eps = __syncthreads_or(near) ? META_QL_TINY_ANGLE : 0.0;
    if (tid >= base && tid < base + T) {
        const double r0 = s.r[tid][0], r1 = s.r[tid][1], r2 = s.r[tid][2], len = s.w[tid][2];
        const double v[3] = {r0, r1 - eps * r2, eps * r1 + r2};
        const double vlen = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const double a = 1.0 - len / cut;
        for (int k = 0; k < 3; k++) { s.u[tid][k] = v[k] / vlen; s.rh[tid][k] = s.r[tid][k] / len; }
        s.w[tid][0] = a * a; s.w[tid][1] = -((2.0 * a) / cut); s.w[tid][2] = vlen;
    }
    if (tid == 0) s.eps[q] = eps;
    return T;
}

// Q_l of the rows [base, base + T) and, for the thread that owns one of them, dQ_l / dr_t into dq; every thread returns the same Q
__device__ __forceinline__ double meta_ql_dim(int l, int base, int T, double eps, MetaQlLds &s, double (*red)[4], double (&dq)[3])
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    dq[0] = dq[1] = dq[2] = 0.0;
    if (T <= 0) return 0.0;
    int Tp = 1;
    while (Tp < T) Tp <<= 1;
    const int K = min(64, 256 / Tp);
    {
        const int rl = tid / K, k = tid % K;
        const bool live = rl < T;
        const int t = base + (live ? rl : 0);
        const double u0 = s.u[t][0], u1 = s.u[t][1], u2 = s.u[t][2];
        double a = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        if (live)
            for (int o = k; o < T; o += K) {
                const double v0 = s.u[base + o][0], v1 = s.u[base + o][1], v2 = s.u[base + o][2], wo = s.w[base + o][0];
                const double c = (u0 * v0 + u1 * v1) + u2 * v2;
                double p0 = 1.0, p1 = c, e0 = 0.0, e1 = 1.0;   // P_{n-1}, P_n and their derivatives, n = 1
                if (l == 0) { p1 = 1.0; e1 = 0.0; }
                for (int n = 2; n <= l; n++) {
                    const double pn = ((((double)(2 * n - 1)) * c) * p1 - ((double)(n - 1)) * p0) / (double)n;
                    const double en = ((double)n) * p1 + c * e1;
                    p0 = p1; p1 = pn; e1 = en;
                }
                const double we = wo * e1;
                a = a + wo * p1;
                b0 = b0 + we * (v0 - c * u0);
                b1 = b1 + we * (v1 - c * u1);
                b2 = b2 + we * (v2 - c * u2);
            }
        for (int m = 1; m < K; m <<= 1) {
            a = a + __shfl_xor(a, m, 64);
            b0 = b0 + __shfl_xor(b0, m, 64);
            b1 = b1 + __shfl_xor(b1, m, 64);
            b2 = b2 + __shfl_xor(b2, m, 64);
        }
        if (live && k == 0) { s.row[t][0] = a; s.row[t][1] = b0; s.row[t][2] = b1; s.row[t][3] = b2; }
    }
    __syncthreads();
    const bool mine = tid >= base && tid < base + T;
    double A = 0.0, B[3] = {0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0};
    if (mine) {
        A = s.row[tid][0]; B[0] = s.row[tid][1]; B[1] = s.row[tid][2]; B[2] = s.row[tid][3];
        sum[0] = s.w[tid][0] * A;
        sum[1] = s.w[tid][0];
    }
    meta_block_sum3(sum, red);   // (its barriers also free row[] for the next dimension)
    const double W = sum[1], W2 = W * W;
    const double Q2 = sum[0] / W2;
    if (!(Q2 > 0.0)) return 0.0;
    const double Q = sqrt(Q2);
    if (mine) {
        const double w = s.w[tid][0], wp = s.w[tid][1], vlen = s.w[tid][2];
        const double av[3] = {(w * B[0]) / vlen, (w * B[1]) / vlen, (w * B[2]) / vlen};   // by v_t; by r_t: through the shear
        const double ang[3] = {av[0], av[1] + eps * av[2], av[2] - eps * av[1]};
        for (int k = 0; k < 3; k++) {
            const double wu = wp * s.rh[tid][k];
            const double t1 = wu * A + ang[k];
            dq[k] = ((2.0 * t1) / W2 - ((2.0 * Q2) * wu) / W) / (2.0 * Q);
        }
    }
    return Q;
}

// x: [N][3] positions of this configuration, sorted order; sel: [ncomp][N] bytes, sorted order (posvar: 1 = in sel and not the
// index atom); centre [cap][D], key [cap][D], rows [cap][7] = cv[6] | V; nh hills stand below this configuration; own: the row
// this configuration deposits (-1: none: n % pace != 0)
// (the body of both forms of the bias: MERGED sums the table tb and then the rows behind its chunks, otherwise every row; QL:
// the spec has a qlvar — a template parameter, so that the kernels of a spec without one are the ones they were)
template <bool MERGED, bool QL = false>
__device__ __forceinline__ void meta_eval(int N, const MetaPar &p, const double *x, const unsigned char *sel, double *centre, int *key,
                                          double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV, const MetaTab &tb,
                                          const MetaQl &ql = MetaQl())
{
#pragma clang fp contract(off)
    __shared__ double red[1 + META_MAXD][4];
    __shared__ double csh[META_MAXD], gsh[META_MAXD];   // (indexed by a running dimension: not registers)
    const int tid = threadIdx.x;
    double qdq[META_MAXD][3];   // QL: dQ_d / dr_t of this thread's row
    if constexpr (QL) {
        MetaQlLds &qs = meta_ql_lds();
        int base = 0;
        for (int q = 0; q < META_MAXC; q++) {
            int T = 0;
            if (q < p.ncomp && p.kind[q] == 2) T = meta_ql_gather(ql, q, p.ia[q], x, qs, base);
            if (tid == 0) { qs.base[q] = base; qs.T[q] = T; }
            base += T;
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < META_MAXD; d++) {
            qdq[d][0] = qdq[d][1] = qdq[d][2] = 0.0;
            const int q = ql.dcomp[d];
            if (q < 0) continue;
            const double Q = meta_ql_dim(ql.dl[d], qs.base[q], qs.T[q], qs.eps[q], qs, red, qdq[d]);
            if (tid == 0) csh[d] = Q;
        }
    }
    // ---- the collective variables
    double dvec[META_MAXC][3], rlen[META_MAXC];
    int d0 = 0;
#pragma unroll
    for (int q = 0; q < META_MAXC; q++) {
        dvec[q][0] = dvec[q][1] = dvec[q][2] = 0.0;
        rlen[q] = 1.0;
        if (q >= p.ncomp) continue;
        if constexpr (QL)
            if (p.kind[q] == 2) { d0 += ql.nl[q]; continue; }   // (csh holds its dimensions already)
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
    double qvir[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // QL, workgroup 0: sum_t r_t (x) G_t of the qlvars
    if constexpr (QL) {
        // G_t of every row, its dimensions in order
        MetaQlLds &qs = meta_ql_lds();
        double G[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < META_MAXD; d++) {
            const int q = ql.dcomp[d];
            if (q < 0) continue;
            if (tid >= qs.base[q] && tid < qs.base[q] + qs.T[q])
                for (int k = 0; k < 3; k++) G[k] = G[k] + gsh[d] * qdq[d][k];
        }
        for (int k = 0; k < 3; k++) qs.g[tid][k] = G[k];
        __syncthreads();
    }
    d0 = 0;
#pragma unroll
    for (int q = 0; q < META_MAXC; q++) {
        if (q >= p.ncomp) continue;
        if constexpr (QL)
            if (p.kind[q] == 2) {
                // F_j -= G_t for every image t of j, in list order; F_index += sum of the G_t of the other atoms
                MetaQlLds &qs = meta_ql_lds();
                const int base = qs.base[q], T = qs.T[q], ia = p.ia[q];
                const bool mine = tid >= base && tid < base + T;
                double s[3] = {0.0, 0.0, 0.0};
                if (mine && qs.j[tid] != ia)
                    for (int k = 0; k < 3; k++) s[k] = qs.g[tid][k];
                meta_block_sum3(s, red);
                if (i == ia) {
                    for (int k = 0; k < 3; k++) f[k] = f[k] + s[k];
                    touched = true;
                } else
                    for (int t = base; t < base + T; t++)
                        if (qs.j[t] == i) {
                            for (int k = 0; k < 3; k++) f[k] = f[k] - qs.g[t][k];
                            touched = true;
                        }
                if (blockIdx.x == 0)   // (the whole workgroup: the sums have barriers)
                    for (int a = 0; a < 3; a++) {
                        double v[3] = {0.0, 0.0, 0.0};
                        if (mine)
                            for (int b = 0; b < 3; b++) v[b] = qs.r[tid][a] * qs.g[tid][b];
                        meta_block_sum3(v, red);
                        for (int b = 0; b < 3; b++) qvir[3 * a + b] = qvir[3 * a + b] + v[b];
                    }
                d0 += ql.nl[q];
                continue;
            }
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
        if constexpr (QL)
            if (p.kind[q] == 2) { d0 += ql.nl[q]; continue; }
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
    // (a qlvar: the pair form over the images, not -sum x (x) F of raw coordinates — an atom stands under several images)
    if constexpr (QL)
        for (int q = 0; q < 9; q++) vir[q] = vir[q] + qvir[q];
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

// the two forms for a spec with a qlvar (kind 2): the same launches in the same place, with the step's neighbour list
__global__ __launch_bounds__(256) void md_meta_ql_kernel(int N, MetaPar p, MetaQl ql, const double *x, const unsigned char *sel, double *centre, int *key,
                                                         double *rows, int nh, int own, double *Fself, double *Epart, double *virpart, int nV,
                                                         const int *halt, int step)
{
    if (*halt < step) return;
    meta_eval<false, true>(N, p, x, sel, centre, key, rows, nh, own, Fself, Epart, virpart, nV, MetaTab(), ql);
}

__global__ __launch_bounds__(256) void md_meta_merged_ql_kernel(int N, MetaPar p, MetaQl ql, const double *x, const unsigned char *sel, double *centre,
                                                                int *key, double *rows, int nh, int own, double *Fself, double *Epart, double *virpart,
                                                                int nV, MetaTab tb, const int *halt, int step)
{
    if (*halt < step) return;
    meta_eval<true, true>(N, p, x, sel, centre, key, rows, nh, own, Fself, Epart, virpart, nV, tb, ql);
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
