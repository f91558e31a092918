// Limited-memory BFGS in the place of FIRE in a relaxation on the device (sgpr_md_relax_lbfgs behind sgpr_md_relax):
// ase/optimize/lbfgs.py without line search (ASE 3.22, LGPL; Nocedal, Math. Comp. 35, 773 (1980)) on md_relax.inc's generalised
// coordinates X = [ r ; c D ] and forces G = [ F D ; (W D^-T o M) / c ] — N rows at constant cell, N + 3 with the cell.
// workloads.lbfgs_relax / LbfgsTwin is the host twin and the definition; everything is written by evaluation index n:
//     converged:  max over rows |G_row|^2 < fmax^2:  nothing moves (halt code 3)
//     behind a start or reset (at `base`): pair n, s_n = X_n - X_(n-1) (stored by the move out of n - 1), y_n = G_(n-1) - G_n;
//     the window is the pairs max(base + 1, n - memory + 1) ... n; a pair whose s.y is zero or not finite keeps its slot and is
//     left out of every product (ASE would divide by it)
//     p = H G,  step = damping p,  scaled by maxstep / longest when the longest row of p reaches maxstep (ASE's >=)
// The two-loop recursion would be 2 memory dependent sums of length 3N.  The compact form (Byrd, Nocedal & Schnabel, Math.
// Program. 63, 129 (1994)) needs ONE pass of sums: with S, Y the window (oldest first), R the upper triangle of S^T Y,
// Dg its diagonal, H0 = 1 / alpha:
//     u = S^T G,  v = H0 Y^T G,  t = R^-1 u,  top = R^-T ((Dg + H0 Y^T Y) t - v),  p = H0 G + S top - H0 Y t
// and R^-1 is never solved for: pair n adds the column [ -R^-1 c / d ; 1 / d ] (c_i = s_i.y_n, d = s_n.y_n), the oldest pair
// leaves with its row and column — every entry is written once.
//   State by evaluation index: pair i in slot i % memory of S and Y ([memory][rows][3]), column i of R^-1 (and of its
// transpose, for coalesced reads) and row / column i of Y^T Y in row / column i % memory of memory x memory arrays, G_i in slot
// i % 2, the cell rows of X_i in slot i % 2.  An evaluation that is repeated (behind a covloss halt, a `final` call) writes its
// own slots again; what the host has enqueued behind a halt returns at once; nothing is rolled back.
//   Behind the plain last kernel of every evaluation:
//   * md_lbfgs_dots_kernel, workgroup (w, a): rows 256 w ... of pair a of the window — G_n (F D, held components zero) and
//     y_n in registers, the partial sums of s_a.y_n, y_a.y_n, s_a.G and y_a.G; the workgroups of the newest pair also store
//     G_n and y_n and leave G.G, the largest |G_row|^2 and the largest covloss;
//   * md_lbfgs_solve_kernel, ONE workgroup: the partials added in index order, the cell rows behind them; the halts (as
//     md_fire_kernel decides them, nothing moved); the new column, t, top, p.G in closed form; a thread per pair;
//   * md_lbfgs_dir_kernel, a thread per row: p, and the largest |p_row|^2 per workgroup;
//   * md_lbfgs_move_kernel, a thread per row: the scale, X_(n+1), s_(n+1), x = r D'^T, the next slot of the ring of cells.
// Sums: fin_wave_sum per wave, the waves pairwise, workgroups in index order, pairs oldest first; no float atomics; no
// contraction; true divisions.  Held components (sgpr_md_fix): G = 0, the step is 0, r keeps its bits — selected.
#pragma once

struct LbfgsBuf {
    double *S, *Y;        // [mem][rows][3]
    double *G;            // [2][rows][3]
    double *dir;          // [rows][3] p
    double *Rinv, *RinvT; // [mem][mem] by slot: Rinv[i][j] = (R^-1)_ij, i <= j
    double *YY;           // [mem][mem]
    double *Dg, *valid;   // [mem]
    double *part;         // [mem][4][B] md_lbfgs_dots_kernel's partial sums by window position
    double *pgg, *pgmx, *pbmx;   // [B] G.G, largest |G_row|^2, largest covloss per workgroup
    double *coef;         // [3][mem] top | H0 t | valid, by window position
    double *pmax;         // [ceil(rows / 64)] largest |p_row|^2 per workgroup
    double *xc;           // [2][9] the cell rows of X by evaluation index % 2
};

template <bool FIX>
__global__ __launch_bounds__(256) void md_lbfgs_dots_kernel(int N, int cell, int mem, LbfgsBuf b, long long n, int cnt, const double *packed, const int *perm,
                                                            const double *cur, const int *halt, int step, const unsigned char *fixed)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double wsum[7][4];
    const int tid = threadIdx.x, B = gridDim.x, a = blockIdx.y;
    const int k = blockIdx.x * 256 + tid;
    const bool act = k < N;
    const size_t NR = (size_t)N + (cell ? 3 : 0);
    const bool last = a == (cnt > 0 ? cnt - 1 : 0);   // the newest pair (or a fresh evaluation, which has none)
    double D[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (cell) {
#pragma unroll
        for (int j = 0; j < 9; j++) D[j] = cur[9 + j];
    }
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0, bm = 0.0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, z0 = 0.0, z1 = 0.0, z2 = 0.0;
    if (act) {
        const int c = perm[k];
        double f0 = packed[3 * (size_t)c], f1 = packed[3 * (size_t)c + 1], f2 = packed[3 * (size_t)c + 2];
        bool h0 = false, h1 = false, h2 = false;
        if (FIX) {
            h0 = fixed[3 * (size_t)k] != 0; h1 = fixed[3 * (size_t)k + 1] != 0; h2 = fixed[3 * (size_t)k + 2] != 0;
            if (h0) f0 = 0.0;
            if (h1) f1 = 0.0;
            if (h2) f2 = 0.0;
        }
        rlx_g_row<FIX>(cell, D, f0, f1, f2, h0, h1, h2, g0, g1, g2);
        if (last) bm = packed[3 * (size_t)N + c];
        if (cnt > 0) {
            const double *gp = b.G + ((size_t)((n - 1) & 1) * NR + k) * 3;
            y0 = gp[0] - g0; y1 = gp[1] - g1; y2 = gp[2] - g2;
            const size_t slot = (size_t)((n - cnt + 1 + a) % mem);
            const double *sp = b.S + (slot * NR + k) * 3;
            s0 = sp[0]; s1 = sp[1]; s2 = sp[2];
            if (last) { z0 = y0; z1 = y1; z2 = y2; }
            else {
                const double *yp = b.Y + (slot * NR + k) * 3;
                z0 = yp[0]; z1 = yp[1]; z2 = yp[2];
            }
        }
        if (last) {
            double *go = b.G + ((size_t)(n & 1) * NR + k) * 3;
            go[0] = g0; go[1] = g1; go[2] = g2;
            if (cnt > 0) {
                double *yo = b.Y + ((size_t)(n % mem) * NR + k) * 3;
                yo[0] = y0; yo[1] = y1; yo[2] = y2;
            }
        }
    }
    const double gg = (g0 * g0 + g1 * g1) + g2 * g2;
    double q0 = fin_wave_sum((s0 * y0 + s1 * y1) + s2 * y2);
    double q1 = fin_wave_sum((z0 * y0 + z1 * y1) + z2 * y2);
    double q2 = fin_wave_sum((s0 * g0 + s1 * g1) + s2 * g2);
    double q3 = fin_wave_sum((z0 * g0 + z1 * g1) + z2 * g2);
    double q4 = fin_wave_sum(gg);
    double gmx = gg;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gmx = fmax(gmx, __shfl_xor(gmx, o, 64)); bm = fmax(bm, __shfl_xor(bm, o, 64)); }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        wsum[0][w] = q0; wsum[1][w] = q1; wsum[2][w] = q2; wsum[3][w] = q3; wsum[4][w] = q4; wsum[5][w] = gmx; wsum[6][w] = bm;
    }
    __syncthreads();
    if (tid < 4 && cnt > 0) b.part[((size_t)a * 4 + tid) * B + blockIdx.x] = (wsum[tid][0] + wsum[tid][1]) + (wsum[tid][2] + wsum[tid][3]);
    if (tid == 4 && last) {
        b.pgg[blockIdx.x] = (wsum[4][0] + wsum[4][1]) + (wsum[4][2] + wsum[4][3]);
        b.pgmx[blockIdx.x] = fmax(fmax(wsum[5][0], wsum[5][1]), fmax(wsum[5][2], wsum[5][3]));
        b.pbmx[blockIdx.x] = fmax(fmax(wsum[6][0], wsum[6][1]), fmax(wsum[6][2], wsum[6][3]));
    }
}

// (the three rows of a 3 x 3 dot, added behind the atoms' sum as workloads.LbfgsTwin._dot does)
__device__ __forceinline__ double lbfgs_dot9(const double *l, const double *r)
{
#pragma clang fp contract(off)
    const double r0 = (l[0] * r[0] + l[1] * r[1]) + l[2] * r[2];
    const double r1 = (l[3] * r[3] + l[4] * r[4]) + l[5] * r[5];
    const double r2 = (l[6] * r[6] + l[7] * r[7]) + l[8] * r[8];
    return (r0 + r1) + r2;
}

// The sixteen scalars of an evaluation: 0..10 as the last kernel left them in `packed`, 11 the largest covloss, 12 the largest
// |G_row|^2, 13 p.G, 14 the scale applied to p (md_lbfgs_move_kernel writes it), 15 the valid pairs in the window; 13 and 14 are
// zero where nothing moves.
__global__ __launch_bounds__(256) void md_lbfgs_solve_kernel(int N, RelaxParams p, int mem, double H0, LbfgsBuf b, long long n, int cnt, int B,
                                                             const double *packed, const double *cur, double ediff, int *halt, int *halt_host, int step,
                                                             double *scal_row, double *cell_row, int *mark, int stay)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double c[128], yy[128], u[128], v[128], t[128], w[128], col[128], top[128], Gc[9], yc[9], shGG;
    __shared__ int val[128], go;
    const int tid = threadIdx.x;
    const size_t NR = (size_t)N + (p.cell ? 3 : 0), N3 = (size_t)3 * N;
    const long long lo = n - cnt + 1;
    const int nw = cnt - 1, sn = (int)(n % mem);
    const double *sc = packed + 4 * (size_t)N;
    if (tid == 0 && p.cell) {
        double h[9], D[9], G9[9];
        for (int k = 0; k < 9; k++) { h[k] = cur[k]; D[k] = cur[9 + k]; }
        rlx_cell_g(p, h, D, sc, G9);
        for (int k = 0; k < 9; k++) {
            Gc[k] = G9[k];
            b.G[(size_t)(n & 1) * NR * 3 + N3 + k] = G9[k];
            if (cnt > 0) {
                const double yk = b.G[(size_t)((n - 1) & 1) * NR * 3 + N3 + k] - G9[k];
                yc[k] = yk;
                b.Y[(size_t)sn * NR * 3 + N3 + k] = yk;
            }
        }
    }
    if (tid < RLX_CELL && cell_row) cell_row[tid] = cur[tid];
    __syncthreads();
    for (int e = tid; e < 4 * cnt; e += 256) {
        const int a = e >> 2, q = e & 3;
        double acc = 0.0;
        for (int wg = 0; wg < B; wg++) acc = acc + b.part[(size_t)e * B + wg];
        if (p.cell) {
            const size_t slot = (size_t)((lo + a) % mem);
            const double *sp = b.S + slot * NR * 3 + N3;
            const double *yp = a == nw ? yc : b.Y + slot * NR * 3 + N3;
            acc = acc + lbfgs_dot9((q & 1) ? yp : sp, q < 2 ? yc : Gc);
        }
        if (q == 0) c[a] = acc;
        else if (q == 1) yy[a] = acc;
        else if (q == 2) u[a] = acc;
        else v[a] = H0 * acc;
    }
    if (tid < nw) val[tid] = b.valid[(lo + tid) % mem] != 0.0 ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
        double GG = 0.0, gmax2 = 0.0, bmax = 0.0;
        for (int wg = 0; wg < B; wg++) { GG = GG + b.pgg[wg]; gmax2 = fmax(gmax2, b.pgmx[wg]); bmax = fmax(bmax, b.pbmx[wg]); }
        if (p.cell) {
            for (int r = 0; r < 3; r++)
                gmax2 = fmax(gmax2, (Gc[3 * r] * Gc[3 * r] + Gc[3 * r + 1] * Gc[3 * r + 1]) + Gc[3 * r + 2] * Gc[3 * r + 2]);
            GG = GG + lbfgs_dot9(Gc, Gc);
        }
        int pairs = 0;
        if (cnt > 0) {
            const double d = c[nw];
            const int vn = (fabs(d) <= 1.7976931348623157e308 && d != 0.0) ? 1 : 0;
            val[nw] = vn;
            b.valid[sn] = vn ? 1.0 : 0.0;
            for (int a = 0; a < cnt; a++) pairs += val[a];
        }
        shGG = GG;
        const bool ov = sc[10] != 0.0;
        for (int k = 0; k < 11; k++) scal_row[k] = sc[k];
        scal_row[11] = bmax; scal_row[12] = gmax2; scal_row[13] = 0.0; scal_row[14] = 0.0; scal_row[15] = (double)pairs;
        int why = -1;   // halt_host word: 0 the covloss gate, 1 a capacity overflow, 2 converged
        if (ov) why = 1;
        else if (bmax >= ediff) why = 0;
        else if (gmax2 < p.fmax2) why = 2;
        if (why >= 0) {
            atomicMin(halt, step);
            halt_host[why] = step;
        }
        go = (why < 0 && !stay) ? 1 : 0;
        if (!go) *mark = 1;
    }
    __syncthreads();
    if (!go) return;
    if (cnt > 0) {
        const double d = c[nw];
        const int a = tid;
        const size_t sa = a < cnt ? (size_t)((lo + a) % mem) : 0;
        const int lo_s = (int)(lo % mem);   // (the slot of window position l: lo_s + l, less mem where it wraps — no division per trip)
        auto slot_of = [lo_s, mem](int l) -> size_t { const int s = lo_s + l; return (size_t)(s >= mem ? s - mem : s); };
        // the new column of R^-1 (and row of its transpose), row / column of Y^T Y, entry of Dg
        if (a < nw) {
            double acc = 0.0;
#pragma unroll 4
            for (int l = a; l < nw; l++) {
                const double r = b.RinvT[slot_of(l) * mem + sa];
                acc = val[l] ? acc + r * c[l] : acc;
            }
            const double cv = (val[nw] && val[a]) ? RLX_DIV(-acc, d) : 0.0;
            col[a] = cv;
            b.Rinv[sa * mem + sn] = cv; b.RinvT[(size_t)sn * mem + sa] = cv;
        }
        if (a == nw) {
            const double cv = val[nw] ? RLX_DIV(1.0, d) : 0.0;
            col[a] = cv;
            b.Rinv[(size_t)sn * mem + sn] = cv; b.RinvT[(size_t)sn * mem + sn] = cv;
            b.Dg[sn] = d;
        }
        if (a < cnt) { b.YY[sa * mem + sn] = yy[a]; b.YY[(size_t)sn * mem + sa] = yy[a]; }
        __syncthreads();
        // t = R^-1 u
        if (a < cnt) {
            double acc = 0.0;
#pragma unroll 4
            for (int l = a; l < cnt; l++) {
                const double r = l == nw ? col[a] : b.RinvT[slot_of(l) * mem + sa];
                acc = val[l] ? acc + r * u[l] : acc;
            }
            t[a] = val[a] ? acc : 0.0;
        }
        __syncthreads();
        // w = (Dg + H0 Y^T Y) t - v
        if (a < cnt) {
            double acc = 0.0;
            const double dg = a == nw ? d : b.Dg[sa];
#pragma unroll 4
            for (int j = 0; j < cnt; j++) {
                const double yv = j == nw ? yy[a] : (a == nw ? yy[j] : b.YY[slot_of(j) * mem + sa]);
                double mij = H0 * yv;
                if (j == a) mij = dg + mij;
                acc = val[j] ? acc + mij * t[j] : acc;
            }
            w[a] = val[a] ? acc - v[a] : 0.0;
        }
        __syncthreads();
        // top = R^-T w
        if (a < cnt) {
            double acc = 0.0;
#pragma unroll 4
            for (int i = 0; i <= a; i++) {
                const double r = a == nw ? col[i] : b.Rinv[slot_of(i) * mem + sa];
                acc = val[i] ? acc + r * w[i] : acc;
            }
            const double tv = val[a] ? acc : 0.0;
            top[a] = tv;
            b.coef[a] = tv; b.coef[mem + a] = H0 * t[a]; b.coef[2 * mem + a] = val[a] ? 1.0 : 0.0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double pG = H0 * shGG;
        for (int a = 0; a < cnt; a++)
            if (val[a]) pG = (pG + top[a] * u[a]) - t[a] * v[a];
        scal_row[13] = pG;
        *mark = 1;
    }
}

// p = H0 G + S top - H0 Y t, row by row, the pairs oldest first; the largest |p_row|^2 of the workgroup.
template <bool FIX>
__global__ __launch_bounds__(64) void md_lbfgs_dir_kernel(int N, int NR, int mem, double H0, LbfgsBuf b, long long n, int cnt, const int *halt, int step,
                                                          const unsigned char *fixed)
{
#pragma clang fp contract(off)
    if (*halt <= step) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    const bool act = k < NR;
    const size_t kk = act ? k : 0, R3 = (size_t)NR * 3;
    const double *g = b.G + (size_t)(n & 1) * R3 + kk * 3;
    double p0 = H0 * g[0], p1 = H0 * g[1], p2 = H0 * g[2];
    const int lo_s = (int)((n - cnt + 1) % mem);   // (the slot of window position a: lo_s + a, less mem where it wraps)
#pragma unroll 4
    for (int a = 0; a < cnt; a++) {
        const double tp = b.coef[a], ht = b.coef[mem + a];
        const bool ok = b.coef[2 * mem + a] != 0.0;
        const size_t slot = (size_t)(lo_s + a >= mem ? lo_s + a - mem : lo_s + a);
        const double *sp = b.S + slot * R3 + kk * 3, *yp = b.Y + slot * R3 + kk * 3;
        const double s0 = sp[0], s1 = sp[1], s2 = sp[2], y0 = yp[0], y1 = yp[1], y2 = yp[2];
        if (ok) {
            p0 = (p0 + tp * s0) - ht * y0;
            p1 = (p1 + tp * s1) - ht * y1;
            p2 = (p2 + tp * s2) - ht * y2;
        }
    }
    if (FIX && k < N) {
        if (fixed[3 * kk] != 0) p0 = 0.0;
        if (fixed[3 * kk + 1] != 0) p1 = 0.0;
        if (fixed[3 * kk + 2] != 0) p2 = 0.0;
    }
    double mx = act ? (p0 * p0 + p1 * p1) + p2 * p2 : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (act) { b.dir[kk * 3] = p0; b.dir[kk * 3 + 1] = p1; b.dir[kk * 3 + 2] = p2; }
    if (threadIdx.x == 0) b.pmax[blockIdx.x] = mx;
}

// The move out of an evaluation that md_lbfgs_solve_kernel has let pass: the scale from the largest row, r and the cell rows of
// X moved, s of the pair evaluation n + 1 completes, x = r D'^T, the next slot of the ring of cells.
template <bool FIX>
__global__ __launch_bounds__(256) void md_lbfgs_move_kernel(int N, RelaxParams p, int mem, double maxstep, double damping, LbfgsBuf b, long long n, int nmax,
                                                            double *ref, double *x_next, double *nxt, const int *halt, int step, double *scal_row,
                                                            const unsigned char *fixed)
{
#pragma clang fp contract(off)
    if (*halt <= step) return;
    const int tid = threadIdx.x, k = blockIdx.x * 256 + tid;
    const int NR = N + (p.cell ? 3 : 0);
    double l2 = 0.0;
    for (int e = tid & 63; e < nmax; e += 64) l2 = fmax(l2, b.pmax[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l2 = fmax(l2, __shfl_xor(l2, o, 64));
    const double longest = RLX_SQRT(l2);
    const double sc = longest >= maxstep ? RLX_DIV(maxstep, longest) : 1.0;
    double Xc[9] = {}, Xn[9] = {}, Dn[9] ={1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (p.cell) {
#pragma unroll
        for (int j = 0; j < 9; j++) {
            Xc[j] = b.xc[(size_t)(n & 1) * 9 + j];
            Xn[j] = Xc[j] + (b.dir[(size_t)3 * N + j] * sc) * damping;
            Dn[j] = RLX_DIV(Xn[j], p.cf);
        }
    }
    double *so = b.S + ((size_t)((n + 1) % mem) * NR) * 3;
    if (k < N) {
        const size_t k3 = (size_t)3 * k;
        double rn[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double r = ref[k3 + j];
            double v = r + (b.dir[k3 + j] * sc) * damping;
            if (FIX && fixed[k3 + j] != 0) v = r;   // (selected, not computed)
            rn[j] = v;
            so[k3 + j] = v - r;
            ref[k3 + j] = v;
        }
#pragma unroll
        for (int j = 0; j < 3; j++)
            x_next[k3 + j] = p.cell ? (rn[0] * Dn[3 * j] + rn[1] * Dn[3 * j + 1]) + rn[2] * Dn[3 * j + 2] : rn[j];
    } else if (k < NR) {
        const int r = k - N;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            so[(size_t)3 * k + j] = Xn[3 * r + j] - Xc[3 * r + j];
            b.xc[(size_t)((n + 1) & 1) * 9 + 3 * r + j] = Xn[3 * r + j];
        }
        if (r == 0) rlx_next_cell(p, Xn, nxt);
    }
    if (k == 0) scal_row[14] = sc;
}
