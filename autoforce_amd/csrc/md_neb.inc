// md_neb.inc — the nudged elastic band inside the device loop (sgpr_md_neb): ASE's default `aseneb` method (ase/neb.py, ASE 3.22,
// LGPL; Henkelman & Jonsson, J. Chem. Phys. 113, 9978 and 9901) under FIRE (md_relax.inc's recurrence with cell = 0), what the
// reference's cl/neb.py drives through ase.neb.NEB(images, climb=climb, allow_shared_calculator=True) — restated by evaluation
// index; workloads.neb_fire is the host twin and the definition.  Images 0 ... K + 1, the two ends fixed and never evaluated,
// the K interior ones i = 1 ... K evaluated by the SAME live handle, one plain step each, at every evaluation of the band:
//     t_i = mic(R_i - R_(i-1)), i = 1 ... K + 1      (per atom: d - rint(d h^-1) h in the periodic directions)
//     imax: the interior image of highest energy, the later one on a tie
//     tau_i = t_(i+1) (i < imax),  t_i (i > imax),  t_i + t_(i+1) (i = imax)
//     G_i = F_i - (F_i.tau_i / tau_i^2) tau_i - (((k t_i - k t_(i+1)).tau_i) / tau_i^2) tau_i
//     climb, i = imax:  G_i = F_i - 2 (F_i.tau_i / tau_i^2) tau_i     (no spring)
// F with zeros on the held components (sgpr_md_fix, one mask for every image), the dots over all 3N components of an image.
// Every one of those dots is a linear combination of five sums per image — F.t_i, F.t_(i+1), t_i.t_i, t_(i+1).t_(i+1),
// t_i.t_(i+1) — so G_i = (F_i - ca_i t_i) - cb_i t_(i+1) with two coefficients per image, and behind the K plain steps of an
// evaluation (results in K packed buffers, caller atom order) three launches follow:
//   * md_neb_sums_kernel, K workgroups: the five sums, the largest covloss, E and the overflow word of its image;
//   * md_neb_fire_kernel, ONE workgroup: imax, the coefficients, the band record, then one pass over all K N rows of G for
//     G.v, G.G, v.v and max |G_row|^2 (per image in md_fire_kernel's fixed order, the images added in the order 1 ... K), the
//     halts — overflow, covloss gate, convergence, with nothing moved yet: no speculative evaluation, no lag —, the FIRE
//     scalars, the row of sixteen scalars and the mark;
//   * md_neb_move_kernel, a quad of lanes per atom per image: G again from the coefficients, v = alpha v + beta G,
//     x += cd v into the next slot of the band ring; held components selected, not computed.
// The band, its velocity and the results are in caller atom order (the handle bins every image itself, as the members of a
// committee bin bcm_x); sums run over the atoms in the library's species-sorted order, through the permutation, and the mask
// is in sorted order as sgpr_md_fix left it.  No float atomics, no contraction, true divisions: two runs give the same bits.
#pragma once

#define NEB_MAX 16      // interior images of a band
#define NEB_INFO 32     // doubles per evaluation of the band record: E[NEB_MAX] | covmax[NEB_MAX]
#define NEB_SUMS 8      // per image: F.t_i, F.t_(i+1), t_i.t_i, t_(i+1).t_(i+1), t_i.t_(i+1), largest covloss, E, overflow

// (NebCell, the band's constant cell: sgpr_internal.h)

// minimum-image form of a displacement: d - rint(d h^-1) h in the periodic directions
__host__ __device__ inline void neb_mic(const NebCell &c, double d0, double d1, double d2, double &o0, double &o1, double &o2)
{
#pragma clang fp contract(off)
    double n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double s = (d0 * c.hi[k] + d1 * c.hi[3 + k]) + d2 * c.hi[6 + k];
        n[k] = c.pbc[k] ? rint(s) : 0.0;
    }
    o0 = d0 - ((n[0] * c.h[0] + n[1] * c.h[3]) + n[2] * c.h[6]);
    o1 = d1 - ((n[0] * c.h[1] + n[1] * c.h[4]) + n[2] * c.h[7]);
    o2 = d2 - ((n[0] * c.h[2] + n[1] * c.h[5]) + n[2] * c.h[8]);
}

// The scalar part of md_fire_kernel as a function (that kernel keeps its own copy of these twenty lines: its compiled form
// does not change): dt, a, nsteps in and out; alpha, beta of v = alpha v + beta G and the step factor cd out.
__host__ __device__ inline void rlx_fire_scalars(const RelaxParams &p, bool fresh, double P, double GG, double vv, double &dt, double &a,
                                                 double &nsteps, double &alpha, double &beta, double &cd)
{
#pragma clang fp contract(off)
    if (fresh) {
        alpha = 0.0; beta = dt;
        vv = 0.0;
    } else if (P > 0.0) {
        alpha = 1.0 - a;
        const double gamma = RLX_DIV(a * RLX_SQRT(vv), RLX_SQRT(GG));
        if (nsteps > p.nmin) {
            dt = fmin(dt * p.finc, p.dtmax);
            a = a * p.fa;
        }
        nsteps += 1.0;
        beta = gamma + dt;
    } else {
        alpha = 0.0; a = p.astart; nsteps = 0.0;
        dt = dt * p.fdec;
        beta = dt;
        vv = 0.0;
    }
    const double nv2 = ((alpha * alpha) * vv + (2.0 * (alpha * beta)) * P) + (beta * beta) * GG;
    const double drn = dt * RLX_SQRT(nv2);
    cd = drn > p.maxstep ? dt * RLX_DIV(p.maxstep, drn) : dt;
}

// What the three kernels share of an evaluation: the band's ring slot [K][N][3], the two ends [2][N][3], the K packed results
// `plen` doubles apart (all caller atom order), the run's permutation (sorted -> caller) and the mask (sorted order; null: none).
struct NebBand {
    int N, K;
    size_t plen;
    const double *band, *ends, *P;
    const int *perm;
    const unsigned char *fixed;
};
__device__ __forceinline__ const double *neb_prev(const NebBand &b, int im) { return im > 0 ? b.band + 3 * (size_t)b.N * (im - 1) : b.ends; }
__device__ __forceinline__ const double *neb_next(const NebBand &b, int im)
{
    return im < b.K - 1 ? b.band + 3 * (size_t)b.N * (im + 1) : b.ends + 3 * (size_t)b.N;
}

// Workgroup im: the sums of interior image im + 1, in md_fire_kernel's order (thread t adds the sorted atoms t, t + 256, ...,
// fin_wave_sum, the four waves pairwise).
__global__ __launch_bounds__(256) void md_neb_sums_kernel(NebBand b, NebCell cell, double *sums, const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double wsum[6][4];
    const int tid = threadIdx.x, im = blockIdx.x, N = b.N;
    const double *xc = b.band + 3 * (size_t)N * im, *xp = neb_prev(b, im), *xn = neb_next(b, im), *pk = b.P + b.plen * im;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, bmx = 0.0;
    for (int k = tid; k < N; k += 256) {
        const size_t c = (size_t)b.perm[k];
        double f0 = pk[3 * c], f1 = pk[3 * c + 1], f2 = pk[3 * c + 2];
        if (b.fixed) {
            if (b.fixed[3 * (size_t)k]) f0 = 0.0;
            if (b.fixed[3 * (size_t)k + 1]) f1 = 0.0;
            if (b.fixed[3 * (size_t)k + 2]) f2 = 0.0;
        }
        const double c0 = xc[3 * c], c1 = xc[3 * c + 1], c2 = xc[3 * c + 2];
        double a0, a1, a2, b0, b1, b2;
        neb_mic(cell, c0 - xp[3 * c], c1 - xp[3 * c + 1], c2 - xp[3 * c + 2], a0, a1, a2);
        neb_mic(cell, xn[3 * c] - c0, xn[3 * c + 1] - c1, xn[3 * c + 2] - c2, b0, b1, b2);
        s0 += (f0 * a0 + f1 * a1) + f2 * a2;
        s1 += (f0 * b0 + f1 * b1) + f2 * b2;
        s2 += (a0 * a0 + a1 * a1) + a2 * a2;
        s3 += (b0 * b0 + b1 * b1) + b2 * b2;
        s4 += (a0 * b0 + a1 * b1) + a2 * b2;
        bmx = fmax(bmx, pk[3 * (size_t)N + c]);
    }
    s0 = fin_wave_sum(s0); s1 = fin_wave_sum(s1); s2 = fin_wave_sum(s2); s3 = fin_wave_sum(s3); s4 = fin_wave_sum(s4);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmx = fmax(bmx, __shfl_xor(bmx, o, 64));
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        wsum[0][w] = s0; wsum[1][w] = s1; wsum[2][w] = s2; wsum[3][w] = s3; wsum[4][w] = s4; wsum[5][w] = bmx;
    }
    __syncthreads();
    double *out = sums + NEB_SUMS * im;
    if (tid < 5) out[tid] = (wsum[tid][0] + wsum[tid][1]) + (wsum[tid][2] + wsum[tid][3]);
    else if (tid == 5) out[5] = fmax(fmax(wsum[5][0], wsum[5][1]), fmax(wsum[5][2], wsum[5][3]));
    else if (tid == 6) out[6] = pk[4 * (size_t)N];
    else if (tid == 7) out[7] = pk[4 * (size_t)N + 10];
}

// Behind the sums of evaluation n of a band.  state: the optimizer's scalars (RLX_*: the relaxation's layout, the cell rows
// unused); vel: the band's velocity [K][N][3], caller order; coef: [K][2] = ca_i, cb_i of G_i = (F_i - ca_i t_i) - cb_i t_(i+1);
// info: this evaluation's band record.  The sixteen scalars: 0 E of imax, 1 imax, 2 the image of the largest covloss (both
// 1 ... K), 10 overflow, 11 largest covloss, 12 max |G_row|^2, 13 G.v, 14 dt and 15 a as used for the move out of this
// configuration (as they stand when nothing moves); the others zero.
// par: the band's constants in device memory (cell, FIRE's keywords, spring constant, climb) — by value they would not leave
// the kernel enough scalar registers.
struct NebFirePar { NebCell cell; RelaxParams p; double kspr; int climb; };
__global__ __launch_bounds__(256) void md_neb_fire_kernel(NebBand b, const NebFirePar *par, double *state, const double *vel, const double *sums, double *coef,
                                                          double *info, double ediff, int *halt, int *halt_host, int step, double *scal_row, int *mark,
                                                          int stay)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    const NebCell &cell = par->cell;
    const RelaxParams &p = par->p;
    const double kspr = par->kspr;
    const int climb = par->climb;
    __shared__ double wsum[NEB_MAX][4][4];
    __shared__ double cf[NEB_MAX][2];
    const int tid = threadIdx.x, N = b.N, K = b.K;
    int imax = 0;
    double emax = sums[6];
    for (int i = 1; i < K; i++) {
        const double e = sums[NEB_SUMS * i + 6];
        if (e >= emax) { emax = e; imax = i; }
    }
    if (tid < K) {
        const double *s = sums + NEB_SUMS * tid;
        double ft, tt, spr;
        if (tid < imax) { ft = s[1]; tt = s[3]; spr = kspr * s[4] - kspr * s[3]; }
        else if (tid > imax) { ft = s[0]; tt = s[2]; spr = kspr * s[2] - kspr * s[4]; }
        else { ft = s[0] + s[1]; tt = (s[2] + 2.0 * s[4]) + s[3]; spr = kspr * (s[2] + s[4]) - kspr * (s[4] + s[3]); }
        const double c = (climb && tid == imax) ? RLX_DIV(2.0 * ft, tt) : RLX_DIV(ft, tt) + RLX_DIV(spr, tt);
        const double ca = tid < imax ? 0.0 : c, cb = tid > imax ? 0.0 : c;
        cf[tid][0] = ca; cf[tid][1] = cb;
        coef[2 * tid] = ca; coef[2 * tid + 1] = cb;
        info[tid] = s[6]; info[NEB_MAX + tid] = s[5];
    }
    __syncthreads();
    for (int im = 0; im < K; im++) {
        const double *xc = b.band + 3 * (size_t)N * im, *xp = neb_prev(b, im), *xn = neb_next(b, im), *pk = b.P + b.plen * im;
        const double *vi = vel + 3 * (size_t)N * im;
        const double ca = cf[im][0], cb = cf[im][1];
        double s_gv = 0.0, s_gg = 0.0, s_vv = 0.0, gmx = 0.0;
        for (int k = tid; k < N; k += 256) {
            const size_t c = (size_t)b.perm[k];
            const double f0 = pk[3 * c], f1 = pk[3 * c + 1], f2 = pk[3 * c + 2];
            const double c0 = xc[3 * c], c1 = xc[3 * c + 1], c2 = xc[3 * c + 2];
            const double v0 = vi[3 * c], v1 = vi[3 * c + 1], v2 = vi[3 * c + 2];
            double a0, a1, a2, b0, b1, b2;
            neb_mic(cell, c0 - xp[3 * c], c1 - xp[3 * c + 1], c2 - xp[3 * c + 2], a0, a1, a2);
            neb_mic(cell, xn[3 * c] - c0, xn[3 * c + 1] - c1, xn[3 * c + 2] - c2, b0, b1, b2);
            double g0 = (f0 - ca * a0) - cb * b0, g1 = (f1 - ca * a1) - cb * b1, g2 = (f2 - ca * a2) - cb * b2;
            if (b.fixed) {
                if (b.fixed[3 * (size_t)k]) g0 = 0.0;
                if (b.fixed[3 * (size_t)k + 1]) g1 = 0.0;
                if (b.fixed[3 * (size_t)k + 2]) g2 = 0.0;
            }
            const double gg = (g0 * g0 + g1 * g1) + g2 * g2;
            s_gv += (g0 * v0 + g1 * v1) + g2 * v2;
            s_gg += gg;
            s_vv += (v0 * v0 + v1 * v1) + v2 * v2;
            gmx = fmax(gmx, gg);
        }
        s_gv = fin_wave_sum(s_gv); s_gg = fin_wave_sum(s_gg); s_vv = fin_wave_sum(s_vv);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gmx = fmax(gmx, __shfl_xor(gmx, o, 64));
        if ((tid & 63) == 0) {
            const int w = tid >> 6;
            wsum[im][0][w] = s_gv; wsum[im][1][w] = s_gg; wsum[im][2][w] = s_vv; wsum[im][3][w] = gmx;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double Gv = 0.0, GG = 0.0, vv = 0.0, gmax2 = 0.0, ov = 0.0, bmax = sums[5];
    int bimg = 0;
    for (int im = 0; im < K; im++) {
        Gv = Gv + ((wsum[im][0][0] + wsum[im][0][1]) + (wsum[im][0][2] + wsum[im][0][3]));
        GG = GG + ((wsum[im][1][0] + wsum[im][1][1]) + (wsum[im][1][2] + wsum[im][1][3]));
        vv = vv + ((wsum[im][2][0] + wsum[im][2][1]) + (wsum[im][2][2] + wsum[im][2][3]));
        gmax2 = fmax(gmax2, fmax(fmax(wsum[im][3][0], wsum[im][3][1]), fmax(wsum[im][3][2], wsum[im][3][3])));
        ov = fmax(ov, sums[NEB_SUMS * im + 7]);
        if (sums[NEB_SUMS * im + 5] > bmax) { bmax = sums[NEB_SUMS * im + 5]; bimg = im; }   // (the earlier image on a tie)
    }
    double dt = state[RLX_DT], a = state[RLX_A], nsteps = state[RLX_NSTEPS];
    const bool fresh = state[RLX_FRESH] != 0.0;
    const double P = fresh ? 0.0 : Gv;
    scal_row[0] = emax; scal_row[1] = (double)(imax + 1); scal_row[2] = (double)(bimg + 1);
    scal_row[10] = ov; scal_row[11] = bmax; scal_row[12] = gmax2; scal_row[13] = P;
    int why = -1;   // halt_host word: 0 the covloss gate, 1 a capacity overflow, 2 converged
    if (ov != 0.0) why = 1;
    else if (bmax >= ediff) why = 0;
    else if (gmax2 < p.fmax2) why = 2;
    if (why >= 0 || stay) {   // (stay: the last evaluation of a `final` call — nothing moves, the optimizer stays as it is)
        scal_row[14] = dt; scal_row[15] = a;
        if (why >= 0) {
            atomicMin(halt, step);
            halt_host[why] = step;
        }
        *mark = 1;
        return;
    }
    double alpha, beta, cd;
    rlx_fire_scalars(p, fresh, P, GG, vv, dt, a, nsteps, alpha, beta, cd);
    scal_row[14] = dt; scal_row[15] = a;
    state[RLX_DT] = dt; state[RLX_A] = a; state[RLX_NSTEPS] = nsteps; state[RLX_FRESH] = 0.0;
    state[RLX_ALPHA] = alpha; state[RLX_BETA] = beta; state[RLX_CD] = cd;
    *mark = 1;
}

// The move out of an evaluation that md_neb_fire_kernel has let pass: workgroup (x, im), lanes 0..2 of a quad take the three
// components of sorted atom i of interior image im + 1 — every lane forms both minimum-image displacements of its atom and
// selects its component: no exchange between lanes.  A halted run (at this evaluation or before it) moves nothing.
__global__ __launch_bounds__(256) void md_neb_move_kernel(NebBand b, NebCell cell, const double *state, const double *coef, double *vel, double *band_next,
                                                          const int *halt, int step)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 3, l3 = lane < 3 ? lane : 2, im = blockIdx.y, N = b.N;
    const int i = blockIdx.x * 64 + (tid >> 2);
    const bool act = i < N;
    const int ia = act ? i : 0;
    // requests: one round trip (unconditional loads with clamped indices), then the ones behind the permutation
    const int halt_w = *halt;
    const size_t c = (size_t)b.perm[ia];
    const double alpha = state[RLX_ALPHA], beta = state[RLX_BETA], cd = state[RLX_CD];
    const double ca = coef[2 * im], cb = coef[2 * im + 1];
    const bool held = b.fixed ? b.fixed[3 * (size_t)ia + l3] != 0 : false;
    const size_t off = 3 * (size_t)N * im;
    const double *xc = b.band + off, *xp = neb_prev(b, im), *xn = neb_next(b, im);
    const double c0 = xc[3 * c], c1 = xc[3 * c + 1], c2 = xc[3 * c + 2];
    const double p0 = xp[3 * c], p1 = xp[3 * c + 1], p2 = xp[3 * c + 2];
    const double n0 = xn[3 * c], n1 = xn[3 * c + 1], n2 = xn[3 * c + 2];
    const double F = b.P[b.plen * im + 3 * c + l3], v = vel[off + 3 * c + l3];
    if (halt_w <= step) return;
    double a0, a1, a2, b0, b1, b2;
    neb_mic(cell, c0 - p0, c1 - p1, c2 - p2, a0, a1, a2);
    neb_mic(cell, n0 - c0, n1 - c1, n2 - c2, b0, b1, b2);
    const double x = l3 == 0 ? c0 : (l3 == 1 ? c1 : c2);
    const double ti = l3 == 0 ? a0 : (l3 == 1 ? a1 : a2), tn = l3 == 0 ? b0 : (l3 == 1 ? b1 : b2);
    const double G = (F - ca * ti) - cb * tn;
    double vn = alpha * v + beta * G;
    double xw = x + cd * vn;
    if (held) { vn = 0.0; xw = x; }   // (selected, not computed)
    if (act && lane < 3) {
        vel[off + 3 * c + lane] = vn;
        band_next[off + 3 * c + lane] = xw;
    }
}
