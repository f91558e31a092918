// Moving-cell MD on the device (sgpr_md_barostat): the combined Nose-Hoover / Parrinello-Rahman scheme of ase.md.npt.NPT —
// what the reference's command line runs when a bulk modulus is given, cl/md.py:131-166; restated in autoforce_amd/npt.py —
// written by evaluation index n (configuration n: scaled coordinates q_n, cell h_n, positions (q_n + 1/2) h_n):
//     zeta_(n+1) = zeta_(n-1) + 2 dt tfact (KE_n - K0)
//     eta_(n+1)  = eta_(n-1) + mask * U(-2 dt pfact det(h_n) (sigma_n - sigma_ext))           (or the trace / traceless split)
//     h_(n+2)    = h_n + 2 dt h_(n+1) eta_(n+1)
//     q_(n+1)    = (2 q_n + q_(n-1) (B_n - 1) + dt^2 (F_n / m) h_n^-1) (B_n + 1)^-1,   B_n = dt h_n (eta_n + zeta_n / 2) h_n^-1
//     v_n        = (q_(n+1) - q_(n-1)) h_n / 2 dt,         x_(n+1) = (q_(n+1) + 1/2) h_(n+1)
// Nothing in the last kernel of evaluation n that is NOT per atom depends on evaluation n itself: zeta_n, eta_n, h_n, h_(n+1)
// follow from evaluation n - 1 and earlier.  So one one-workgroup launch behind each evaluation (md_npt_kernel, the slot
// md_nh_kernel has at constant cell) prepares, from the sums over the atoms of evaluation n, everything the last kernel of
// evaluation n + 1 reads: the matrices of its position update, the cell h_(n+2) it moves its atoms into, the bin grid of that
// cell and the rebuild rule for it.  The per-atom part is finalize_next_kernel<3> (api.hip).
//   Operations and their order are those of workloads.npt_moving_cell (the host twin): no contraction, true divisions, the
// 3 x 3 products and the inverse of an upper-triangular matrix spelled out.  The functions marked __host__ __device__ also
// compute the start of a trajectory on the host (md_npt_start, api.hip).
#pragma once
#include "nl_grid.inc"

#if defined(__HIP_DEVICE_COMPILE__)
#define NPT_DIV(a, b) __ddiv_rn((a), (b))
#else
#define NPT_DIV(a, b) ((a) / (b))
#endif

// (NptSlot — the rings, and why they have four slots — and NptParams: sgpr_internal.h)

__host__ __device__ inline void npt_m3_mul(const double *a, const double *b, double *c)
{
#pragma clang fp contract(off)
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) c[3 * r + k] = (a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k]) + a[3 * r + 2] * b[6 + k];
}

// inverse of an upper-triangular matrix, closed form
__host__ __device__ inline void npt_inv_upper(const double *h, double *o)
{
#pragma clang fp contract(off)
    const double i00 = NPT_DIV(1.0, h[0]), i11 = NPT_DIV(1.0, h[4]), i22 = NPT_DIV(1.0, h[8]);
    o[0] = i00; o[4] = i11; o[8] = i22;
    o[1] = -((h[1] * i00) * i11);
    o[5] = -((h[5] * i11) * i22);
    o[2] = ((h[1] * h[5] - h[2] * h[4]) * i00) * (i11 * i22);
    o[3] = 0.0; o[6] = 0.0; o[7] = 0.0;
}

// sigma = the stress of the packed virial in the cell h (sgpr_stress_from_virial's operations) minus the ideal-gas part S / V;
// acc (sgpr_md_filter; null: none): the accumulated stress jumps, subtracted from the model's stress first (FilterDeltas.get_stress)
__host__ __device__ inline void npt_sigma(const double *vir, const double *c, const double *S, double *sig, const double *acc = nullptr)
{
#pragma clang fp contract(off)
    double vol = fabs(c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]));
    if (!(vol > 0.0)) vol = -2.0;
    const int voigt[6] = {0, 4, 8, 5, 2, 1};
    const double vh = fabs((c[0] * c[4]) * c[8]);
    if (!acc) {
        for (int k = 0; k < 6; k++) sig[k] = NPT_DIV(vir[voigt[k]], vol) - NPT_DIV(S[k], vh);
        return;
    }
    for (int k = 0; k < 6; k++) sig[k] = (NPT_DIV(vir[voigt[k]], vol) - acc[k]) - NPT_DIV(S[k], vh);
}

// npt.NPT._deta: -fdt pfact det(h) (sigma - external) as a strain-rate increment
__host__ __device__ inline void npt_deta(double fdt, const NptParams &p, const double *h, const double *sig, double *d)
{
#pragma clang fp contract(off)
    const double c = fdt * (p.pfact * ((h[0] * h[4]) * h[8]));
    double de[6];
    for (int k = 0; k < 6; k++) de[k] = -(c * (sig[k] - p.ext[k]));
    const double u[9] = {de[0], de[5], de[4], 0.0, de[1], de[3], 0.0, 0.0, de[2]};
    if (p.frac == 1.0) {
        for (int k = 0; k < 9; k++) d[k] = p.mask[k] * u[k];
        return;
    }
    const double tr = NPT_DIV((u[0] + u[4]) + u[8], 3.0);
    for (int k = 0; k < 9; k++) {
        const double t = (k % 4 == 0) ? tr : 0.0;
        d[k] = t + p.frac * (u[k] - t);
    }
}

// h^-1, B - 1, (B + 1)^-1 with B = dt h ((eta + zeta / 2) h^-1)
__host__ __device__ inline void npt_matrices(double dt, const double *h, const double *eta, double zeta, double *hinv, double *bm1, double *bp1inv)
{
#pragma clang fp contract(off)
    npt_inv_upper(h, hinv);
    const double hz = 0.5 * zeta;
    double g[9], t[9], gh[9], bp1[9];
    for (int k = 0; k < 9; k++) g[k] = eta[k] + ((k % 4 == 0) ? hz : 0.0);
    npt_m3_mul(g, hinv, t);
    npt_m3_mul(h, t, gh);
    for (int k = 0; k < 9; k++) {
        const double b = dt * gh[k], one = (k % 4 == 0) ? 1.0 : 0.0;
        bm1[k] = b - one;
        bp1[k] = b + one;
    }
    npt_inv_upper(bp1, bp1inv);
}

// nl_bin_kernel's rule for lists built in the cell whose inverse is h0inv, used in the cell h (neighbor.hip): A = h0^-1 h,
// every atom within thr = ((1 - |A - 1|_F) (rc + skin) - rc) / 2 of its affinely mapped build-time position
__device__ inline void npt_affine_rule(const double *h0inv, const double *h, const NptParams &p, double *aff, double *thr2)
{
    double fro = 0.0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double v = h0inv[3 * r] * h[c] + h0inv[3 * r + 1] * h[3 + c] + h0inv[3 * r + 2] * h[6 + c];
            aff[3 * r + c] = v;
            const double d = v - (r == c ? 1.0 : 0.0);
            fro += d * d;
        }
    double thr = 0.5 * ((1.0 - sqrt(fro)) * p.rc_list - p.rc_phys);
    if (!(fro < 1.0)) thr = -1.0;   // (also NaN: no lists have been built yet)
    *thr2 = thr > 0.0 ? thr * thr : -1.0;
}

// Behind evaluation n (ONE workgroup; n = -1: before the first evaluation of a trajectory, whose slot 0 the host has filled):
// seven sums over the atoms in md_nh_kernel's fixed order (thread t adds the atoms t, t + 256, ..., then a pairwise tree:
// workloads._device_order_sum) — m v_a v_b for the six Voigt components of the ideal-gas stress and the kinetic energy's
// m v^2 as the last kernel left it per atom —, then on one lane the recurrences above and what the last kernel of evaluation
// n + 1 needs.  Exits on the halt word like md_nh_kernel.
//   fs_cur / fs_next (sgpr_md_filter; null: no filter, today's arithmetic): the six accumulated stress jumps of configuration n
// and, out, of n + 1 — this one's times `shrink`, which is also what the stress of configuration n is reduced by.
__global__ __launch_bounds__(256) void md_npt_kernel(int N, NptParams p, NptSlot *ring, double *zeta, const double *ke, const double *vel,
                                                     const double *mass, const double *packed, const double *cell0, int n,
                                                     const int *halt, int step, double *scal_row, double *cell_row,
                                                     const double *fs_cur, double *fs_next, double shrink)
{
    if (*halt < step) return;
    __shared__ double wsum[7][4];
    const int tid = threadIdx.x;
    NptSlot &cur = ring[n & 3], &nxt = ring[(n + 1) & 3], &nn2 = ring[(n + 2) & 3];
    if (n >= 0) {
        double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = tid; k < N; k += 256) {
#pragma clang fp contract(off)
            const double ms = mass[k], vx = vel[3 * (size_t)k], vy = vel[3 * (size_t)k + 1], vz = vel[3 * (size_t)k + 2];
            s[0] += ms * (vx * vx); s[1] += ms * (vy * vy); s[2] += ms * (vz * vz);
            s[3] += ms * (vy * vz); s[4] += ms * (vx * vz); s[5] += ms * (vx * vy);
            s[6] += ke[2 * (size_t)k];
        }
#pragma unroll
        for (int q = 0; q < 7; q++) {
            const double t = fin_wave_sum(s[q]);
            if ((tid & 63) == 0) wsum[q][tid >> 6] = t;
        }
        if (tid < 18 && cell_row) cell_row[tid] = tid < 9 ? cur.h[tid] : cur.eta[tid - 9];
    }
    __syncthreads();
    if (tid != 0) return;
    if (n >= 0) {
#pragma clang fp contract(off)
        double S[6], sig[6], d[9], hc[9], h1[9], eprev[9], enew[9], t9[9];
        for (int q = 0; q < 6; q++) S[q] = (wsum[q][0] + wsum[q][1]) + (wsum[q][2] + wsum[q][3]);
        const double KE = 0.5 * ((wsum[6][0] + wsum[6][1]) + (wsum[6][2] + wsum[6][3]));
        for (int k = 0; k < 9; k++) { hc[k] = cur.h[k]; h1[k] = nxt.h[k]; }
        if (fs_cur) {
            double acc[6];
            for (int q = 0; q < 6; q++) { acc[q] = fs_cur[q] * shrink; fs_next[q] = acc[q]; }
            npt_sigma(packed + 4 * (size_t)N + 1, hc, S, sig, acc);
        } else
            npt_sigma(packed + 4 * (size_t)N + 1, hc, S, sig);
        if (n == 0) {   // NPT.initialize(): eta_(-1) = eta_0 - half the increment, zeta_(-1) likewise
            npt_deta(p.dt, p, hc, sig, d);
            for (int k = 0; k < 9; k++) eprev[k] = cur.eta[k] - d[k];
        } else
            for (int k = 0; k < 9; k++) eprev[k] = ring[(n + 3) & 3].eta[k];
        npt_deta(2.0 * p.dt, p, hc, sig, d);
        for (int k = 0; k < 9; k++) { enew[k] = eprev[k] + d[k]; nxt.eta[k] = enew[k]; }
        const int sc = n & 3, sn = (n + 1) & 3, sp = (n + 3) & 3;
        const double dk = KE - p.K0;
        const double zcur = n == 0 ? 0.0 : zeta[sc], zint = n == 0 ? 0.0 : zeta[4 + sc];
        const double zprev = n == 0 ? zcur - p.c1 * dk : zeta[sp];
        const double znew = zprev + p.c2 * dk;
        zeta[sn] = znew;
        zeta[4 + sn] = zint + p.dt * znew;
        scal_row[14] = zcur;
        scal_row[15] = zint;
        npt_m3_mul(h1, enew, t9);
        for (int k = 0; k < 9; k++) nn2.h[k] = hc[k] + (2.0 * p.dt) * t9[k];
        double hinv[9], bm1[9], bp1inv[9];
        npt_matrices(p.dt, h1, enew, znew, hinv, bm1, bp1inv);
        for (int k = 0; k < 9; k++) { nxt.hinv[k] = hinv[k]; nxt.bm1[k] = bm1[k]; nxt.bp1inv[k] = bp1inv[k]; }
    } else {
        NlGrid g0;
        nl_make_grid(nxt.h, p.pbc, p.rc_list, g0, nullptr);
        nxt.grid = g0;
    }
    // the cell the last kernel of evaluation n + 1 moves its atoms into: its grid, and how far the lists reach in it
    double h2[9], hi1[9], c0i[9], aff[9], thr2;
    for (int k = 0; k < 9; k++) { h2[k] = nn2.h[k]; hi1[k] = nxt.hinv[k]; c0i[k] = cell0[9 + k]; }
    NlGrid g;
    nl_make_grid(h2, p.pbc, p.rc_list, g, nullptr);
    nn2.grid = g;
    npt_affine_rule(c0i, h2, p, aff, &thr2);
    for (int k = 0; k < 9; k++) nxt.aff_keep[k] = aff[k];
    nxt.thr2_keep = thr2;
    npt_affine_rule(hi1, h2, p, aff, &thr2);
    for (int k = 0; k < 9; k++) nxt.aff_reb[k] = aff[k];
    nxt.thr2_reb = thr2;
}
