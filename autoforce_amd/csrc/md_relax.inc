// FIRE relaxation of the positions, and optionally of the cell, on the device (sgpr_md_relax): ase/optimize/fire.py (ASE 3.22,
// LGPL; Bitzek et al., PRL 97, 170201) on the generalised coordinates of ase.constraints.UnitCellFilter(atoms, mask=mask) —
// what the reference's relax(cell=True) minimises, cl/relax.py:45-48; restated in autoforce_amd/cl/relax.py — written by
// evaluation index n.  With h0 the cell at the start (rows = vectors), D the deformation gradient (D = 1 at the start), c = N:
//     cell h = h0 D^T,   positions x = r D^T,   X = [ r ; c D ],   G = [ F D ; (W D^-T o M) / c ],  W = -V stress
//     converged:  max over rows |G_row|^2 < fmax^2:  nothing moves (halt code 3)
//     first evaluation (or the first behind sgpr_md_relax_reset):  alpha = 0, beta = dt
//     P = G.v > 0:  alpha = 1 - a, beta = a |v| / |G| + dt'   (dt' = min(dt finc, dtmax), a *= fa when nsteps > nmin; nsteps += 1)
//     else:         alpha = 0, a = astart, dt *= fdec, nsteps = 0, beta = dt
//     v = alpha v + beta G,   |v|^2 = alpha^2 v.v + 2 alpha beta G.v + beta^2 G.G,   X += s dt v,  s = min(1, maxstep / (dt |v|))
// Unlike the thermostats, the move out of configuration n needs three sums over the forces of evaluation n ITSELF (G.v, G.G,
// v.v; the length of the step follows from them in closed form), so the integrator cannot sit in the evaluation's last kernel.
// Behind the plain last kernel of every evaluation (forces, beta, the eleven scalars):
//   * md_fire_kernel, ONE workgroup: the three sums in md_nh_kernel's fixed order (thread t adds the atoms t, t + 256, ..., then
//     a pairwise tree: workloads._device_order_sum), the largest |G_row|^2 and the largest covloss of THIS evaluation — the
//     covloss gate, the overflow halt and convergence are decided here, with nothing moved yet: no speculative evaluation,
//     no lag —, the cell rows of G from the packed virial, the FIRE scalars, the three coefficients of the move, the new D
//     and the next cell h0 D^T (into the next slot of the ring of cells);
//   * md_fire_move_kernel, a quad of lanes per atom: v, r, x = r D^T of the next configuration.
// Held components (sgpr_md_fix; the FIX instantiations, `fixed` a byte per component in sorted order): the optimizer sees F = 0
// there and the component of G = F D is zero in the three sums and in max |G_row|^2 — convergence is judged on the free
// components, the cell rows are as they are —; its velocity is 0 and the coordinate r is handed on as it is, selected
// explicitly: at constant cell x = r keeps its bits, under a moving cell r is what is held and x = r D^T follows the cell
// (ase.constraints.FixAtoms inside UnitCellFilter).  The forces in `packed` stay the model's.
// The next evaluation bins its atoms itself (the binning kernel: general cells, the affine rebuild rule under strain).
//   Operations and their order are those of workloads.fire_relax (the host twin): no contraction, true divisions, the 3 x 3
// algebra spelled out with a general closed-form inverse (a relaxed cell has all nine components).
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define RLX_DIV(a, b) __ddiv_rn((a), (b))
#define RLX_SQRT(a) __dsqrt_rn(a)
#else
#define RLX_DIV(a, b) ((a) / (b))
#define RLX_SQRT(a) sqrt(a)
#endif

// (RelaxParams, the layout of the optimizer's state and the rings' length: sgpr_internal.h)

// general 3 x 3 inverse: cofactors over the determinant
__host__ __device__ inline void rlx_m3_inv(const double *d, double *o)
{
#pragma clang fp contract(off)
    const double c00 = d[4] * d[8] - d[5] * d[7], c01 = d[3] * d[8] - d[5] * d[6], c02 = d[3] * d[7] - d[4] * d[6];
    const double det = (d[0] * c00 - d[1] * c01) + d[2] * c02;
    o[0] = RLX_DIV(c00, det); o[1] = RLX_DIV(d[2] * d[7] - d[1] * d[8], det); o[2] = RLX_DIV(d[1] * d[5] - d[2] * d[4], det);
    o[3] = RLX_DIV(-c01, det); o[4] = RLX_DIV(d[0] * d[8] - d[2] * d[6], det); o[5] = RLX_DIV(d[2] * d[3] - d[0] * d[5], det);
    o[6] = RLX_DIV(c02, det); o[7] = RLX_DIV(d[1] * d[6] - d[0] * d[7], det); o[8] = RLX_DIV(d[0] * d[4] - d[1] * d[3], det);
}

// a b^T
__host__ __device__ inline void rlx_m3_mul_t(const double *a, const double *b, double *c)
{
#pragma clang fp contract(off)
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) c[3 * r + k] = (a[3 * r] * b[3 * k] + a[3 * r + 1] * b[3 * k + 1]) + a[3 * r + 2] * b[3 * k + 2];
}

__host__ __device__ inline double rlx_det(const double *c)
{
#pragma clang fp contract(off)
    return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
}

// ---- what the optimizers of a relaxation share: rlx_g_row serves md_fire_kernel and md_lbfgs.inc; rlx_cell_g and rlx_next_cell
// serve md_lbfgs.inc, and md_fire_kernel keeps its own copy of their lines below (calling them moved its compiled form from 122
// to 106 VGPRs: a FIRE run launches the kernels it launched before); md_fire_move_kernel spreads an atom over a quad of lanes ----
// The row of G of one atom: G = F D with a moving cell, else F — the force as the optimizer sees it (held components zero
// on entry) — with the held components of G zero again.
template <bool FIX>
__device__ __forceinline__ void rlx_g_row(int cell, const double *D, double f0, double f1, double f2, bool h0, bool h1, bool h2,
                                          double &g0, double &g1, double &g2)
{
#pragma clang fp contract(off)
    g0 = f0; g1 = f1; g2 = f2;
    if (cell) {
        g0 = (f0 * D[0] + f1 * D[3]) + f2 * D[6];
        g1 = (f0 * D[1] + f1 * D[4]) + f2 * D[7];
        g2 = (f0 * D[2] + f1 * D[5]) + f2 * D[8];
        if (FIX) {
            if (h0) g0 = 0.0;
            if (h1) g1 = 0.0;
            if (h2) g2 = 0.0;
        }
    }
}

// The cell rows of G: (W D^-T o M) / c with W = -V stress, the stress as sgpr_stress_from_virial gives it.  h: the cell of
// the configuration, sc: the eleven scalars of its evaluation.
__device__ __forceinline__ void rlx_cell_g(const RelaxParams &p, const double *h, const double *D, const double *sc, double *Gc)
{
#pragma clang fp contract(off)
    double Di[9], T[9];
    const double vol = fabs(rlx_det(h));
    const double vq = vol > 0.0 ? vol : -2.0;
    const int voigt[6] = {0, 4, 8, 5, 2, 1};
    double w6[6];
    for (int k = 0; k < 6; k++) w6[k] = -(vol * RLX_DIV(sc[1 + voigt[k]], vq));
    const double W[9] = {w6[0], w6[5], w6[4], w6[5], w6[1], w6[3], w6[4], w6[3], w6[2]};
    rlx_m3_inv(D, Di);
    rlx_m3_mul_t(W, Di, T);
    for (int k = 0; k < 9; k++) Gc[k] = RLX_DIV(T[k] * p.mask[k], p.cf);
}

// The next configuration's deformation gradient D' = Xc / c and cell h0 D'^T from the cell rows Xc of X, into its slot of
// the ring of cells.
__device__ __forceinline__ void rlx_next_cell(const RelaxParams &p, const double *Xc, double *nxt)
{
#pragma clang fp contract(off)
    double Dn[9], hn[9];
    for (int k = 0; k < 9; k++) Dn[k] = RLX_DIV(Xc[k], p.cf);
    rlx_m3_mul_t(p.h0, Dn, hn);
    for (int k = 0; k < 9; k++) { nxt[k] = hn[k]; nxt[9 + k] = Dn[k]; }
}

// Behind evaluation n of a relaxation (see above).  packed: the results of this evaluation (caller atom order), vel: the
// velocities of the atoms' coordinates (sorted order), cur / nxt: this configuration's and the next one's slot of the ring of
// cells.  The sixteen scalars: 0..10 as the last kernel left them in `packed`, 11 the largest covloss, 12 the largest |G_row|^2,
// 13 G.v, 14 dt and 15 a as used for the move out of this configuration (as they stand when nothing moves).
template <bool FIX>
__global__ __launch_bounds__(256) void md_fire_kernel(int N, RelaxParams p, double *state, const double *packed, const int *perm, const double *vel,
                                                      const double *cur, double *nxt, double ediff, int *halt, int *halt_host, int step,
                                                      double *scal_row, double *cell_row, int *mark, int stay, const unsigned char *fixed)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double wsum[5][4];
    const int tid = threadIdx.x;
    double D[9];
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = cur[9 + k];
    double s_gv = 0.0, s_gg = 0.0, s_vv = 0.0, gmx = 0.0, bmx = 0.0;
    for (int k = tid; k < N; k += 256) {
        const int c = perm[k];
        double f0 = packed[3 * (size_t)c], f1 = packed[3 * (size_t)c + 1], f2 = packed[3 * (size_t)c + 2];
        bool h0 = false, h1 = false, h2 = false;
        if (FIX) {
            h0 = fixed[3 * (size_t)k] != 0; h1 = fixed[3 * (size_t)k + 1] != 0; h2 = fixed[3 * (size_t)k + 2] != 0;
            if (h0) f0 = 0.0;
            if (h1) f1 = 0.0;
            if (h2) f2 = 0.0;
        }
        const double v0 = vel[3 * (size_t)k], v1 = vel[3 * (size_t)k + 1], v2 = vel[3 * (size_t)k + 2];
        double g0, g1, g2;
        rlx_g_row<FIX>(p.cell, D, f0, f1, f2, h0, h1, h2, g0, g1, g2);
        const double gg = (g0 * g0 + g1 * g1) + g2 * g2;
        s_gv += (g0 * v0 + g1 * v1) + g2 * v2;
        s_gg += gg;
        s_vv += (v0 * v0 + v1 * v1) + v2 * v2;
        gmx = fmax(gmx, gg);
        bmx = fmax(bmx, packed[3 * (size_t)N + c]);
    }
    s_gv = fin_wave_sum(s_gv); s_gg = fin_wave_sum(s_gg); s_vv = fin_wave_sum(s_vv);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gmx = fmax(gmx, __shfl_xor(gmx, o, 64)); bmx = fmax(bmx, __shfl_xor(bmx, o, 64)); }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        wsum[0][w] = s_gv; wsum[1][w] = s_gg; wsum[2][w] = s_vv; wsum[3][w] = gmx; wsum[4][w] = bmx;
    }
    if (tid < RLX_CELL && cell_row) cell_row[tid] = cur[tid];
    __syncthreads();
    if (tid != 0) return;
    const double *sc = packed + 4 * (size_t)N;
    double Gv = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
    double GG = (wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3]);
    double vv = (wsum[2][0] + wsum[2][1]) + (wsum[2][2] + wsum[2][3]);
    double gmax2 = fmax(fmax(wsum[3][0], wsum[3][1]), fmax(wsum[3][2], wsum[3][3]));
    const double bmax = fmax(fmax(wsum[4][0], wsum[4][1]), fmax(wsum[4][2], wsum[4][3]));
    double dt = state[RLX_DT], a = state[RLX_A], nsteps = state[RLX_NSTEPS];
    const bool fresh = state[RLX_FRESH] != 0.0;
    double Gc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, vc[9], Xc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { vc[k] = state[RLX_VC + k]; Xc[k] = state[RLX_XC + k]; }
    if (p.cell) {
        // the cell rows of G: (W D^-T o M) / c with W = -V stress, the stress as sgpr_stress_from_virial gives it
        double h[9], Di[9], T[9];
#pragma unroll
        for (int k = 0; k < 9; k++) h[k] = cur[k];
        const double vol = fabs(rlx_det(h));
        const double vq = vol > 0.0 ? vol : -2.0;
        const int voigt[6] = {0, 4, 8, 5, 2, 1};
        double w6[6];
        for (int k = 0; k < 6; k++) w6[k] = -(vol * RLX_DIV(sc[1 + voigt[k]], vq));
        const double W[9] = {w6[0], w6[5], w6[4], w6[5], w6[1], w6[3], w6[4], w6[3], w6[2]};
        rlx_m3_inv(D, Di);
        rlx_m3_mul_t(W, Di, T);
        for (int k = 0; k < 9; k++) Gc[k] = RLX_DIV(T[k] * p.mask[k], p.cf);
        double rg[3], rv[3], rw[3];
        for (int r = 0; r < 3; r++) {
            rg[r] = (Gc[3 * r] * Gc[3 * r] + Gc[3 * r + 1] * Gc[3 * r + 1]) + Gc[3 * r + 2] * Gc[3 * r + 2];
            rv[r] = (Gc[3 * r] * vc[3 * r] + Gc[3 * r + 1] * vc[3 * r + 1]) + Gc[3 * r + 2] * vc[3 * r + 2];
            rw[r] = (vc[3 * r] * vc[3 * r] + vc[3 * r + 1] * vc[3 * r + 1]) + vc[3 * r + 2] * vc[3 * r + 2];
            gmax2 = fmax(gmax2, rg[r]);
        }
        GG = GG + ((rg[0] + rg[1]) + rg[2]);
        Gv = Gv + ((rv[0] + rv[1]) + rv[2]);
        vv = vv + ((rw[0] + rw[1]) + rw[2]);
    }
    const double P = fresh ? 0.0 : Gv;
    const bool ov = sc[10] != 0.0;
    for (int k = 0; k < 11; k++) scal_row[k] = sc[k];
    scal_row[11] = bmax; scal_row[12] = gmax2; scal_row[13] = P;
    int why = -1;   // halt_host word: 0 the covloss gate, 1 a capacity overflow, 2 converged
    if (ov) why = 1;
    else if (bmax >= ediff) why = 0;
    else if (gmax2 < p.fmax2) why = 2;
    if (why >= 0) {
        scal_row[14] = dt; scal_row[15] = a;
        atomicMin(halt, step);
        halt_host[why] = step;
        *mark = 1;
        return;
    }
    if (stay) {   // (the last evaluation of a `final` call: nothing moves, the optimizer stays as it is)
        scal_row[14] = dt; scal_row[15] = a;
        *mark = 1;
        return;
    }
    double alpha, beta;
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
    const double cd = drn > p.maxstep ? dt * RLX_DIV(p.maxstep, drn) : dt;
    scal_row[14] = dt; scal_row[15] = a;
    state[RLX_DT] = dt; state[RLX_A] = a; state[RLX_NSTEPS] = nsteps; state[RLX_FRESH] = 0.0;
    state[RLX_ALPHA] = alpha; state[RLX_BETA] = beta; state[RLX_CD] = cd;
    if (p.cell) {
        double Dn[9], hn[9];
        for (int k = 0; k < 9; k++) {
            vc[k] = alpha * vc[k] + beta * Gc[k];
            Xc[k] = Xc[k] + cd * vc[k];
            Dn[k] = RLX_DIV(Xc[k], p.cf);
        }
        rlx_m3_mul_t(p.h0, Dn, hn);
        for (int k = 0; k < 9; k++) { state[RLX_VC + k] = vc[k]; state[RLX_XC + k] = Xc[k]; nxt[k] = hn[k]; nxt[9 + k] = Dn[k]; }
    }
    *mark = 1;
}

// The move out of an evaluation that md_fire_kernel has let pass: lanes 0..2 of a quad take the three components of sorted atom
// i — G = F D, v = alpha v + beta G, r += cd v, x = r D'^T (D' the next configuration's) — in workloads.fire_relax's operations.
// A halted run (at this evaluation or before it) moves nothing.
template <bool FIX>
__global__ __launch_bounds__(256) void md_fire_move_kernel(int N, int cell, const double *state, const int *perm, const double *packed, double *vel,
                                                           double *ref, double *x_next, const double *cur, const double *nxt, const int *halt, int step,
                                                           const unsigned char *fixed)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 3, l3 = lane < 3 ? lane : 2;
    const int i = blockIdx.x * 64 + (tid >> 2);
    const bool act = i < N;
    const int ia = act ? i : 0;
    // requests: one round trip (unconditional loads with clamped indices), then the one behind the permutation
    const int halt_w = *halt;
    const int c = perm[ia];
    const double v = vel[3 * (size_t)ia + l3], r = ref[3 * (size_t)ia + l3];
    const double alpha = state[RLX_ALPHA], beta = state[RLX_BETA], cd = state[RLX_CD];
    double dcol[3] = {0.0, 0.0, 0.0}, drow[3] = {0.0, 0.0, 0.0};
    if (cell) {
#pragma unroll
        for (int j = 0; j < 3; j++) { dcol[j] = cur[9 + 3 * j + l3]; drow[j] = nxt[9 + 3 * l3 + j]; }
    }
    const bool held = FIX ? fixed[3 * (size_t)ia + l3] != 0 : false;   // (with the first round trip)
    double F = packed[3 * (size_t)c + l3];
    if (halt_w <= step) return;
    if (held) F = 0.0;
    double G = F;
    if (cell) G = (fin_quad_lane<0>(F) * dcol[0] + fin_quad_lane<1>(F) * dcol[1]) + fin_quad_lane<2>(F) * dcol[2];
    if (held) G = 0.0;
    double vn = alpha * v + beta * G;
    double rn = r + cd * vn;
    if (held) { vn = 0.0; rn = r; }   // (selected, not computed)
    double xn = rn;
    if (cell) xn = (fin_quad_lane<0>(rn) * drow[0] + fin_quad_lane<1>(rn) * drow[1]) + fin_quad_lane<2>(rn) * drow[2];
    if (act && lane < 3) {
        vel[3 * (size_t)i + lane] = vn;
        ref[3 * (size_t)i + lane] = rn;
        x_next[3 * (size_t)i + lane] = xn;
    }
}
