// md_pimd.inc — path-integral molecular dynamics inside the device loop (sgpr_md_pimd): a ring polymer of P beads under BAOAB
// with the PILE-L thermostat (Ceriotti, Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104; the BAOAB ordering of
// Liu, Li, Liu, J. Chem. Phys. 145, 024103), what the reference's ActiveCalculator(nbeads=P) is driven with from outside —
// restated by evaluation index; workloads.pimd_baoab is the host twin and the definition.  Beads j = 0 ... P - 1 (cyclic), all
// evaluated by the SAME live handle, one plain step each, at every evaluation of the polymer; physical temperature T, the polymer
// sampled at kT_P = P kB T with w_P = kT_P / hbar (the RPMD convention):
//     H_P = sum_j sum_i [ m_i v_ij^2 / 2 + m_i w_P^2 / 2 |x_ij - x_i,j+1|^2 ] + sum_j V(x_j)
// on the raw coordinates (no minimum image in the springs: the beads of an atom start together and stay unwrapped relative to
// each other).  Behind the P plain steps of evaluation n (results in P packed buffers, caller atom order) three launches:
//   * md_pimd_sums_kernel, P workgroups: E, the largest covloss, the overflow word, the two sum m v^2 (after | before the closing
//     half kick), sum (x - xbar).F and the spring sum with bead j + 1 of its bead — the centroid xbar recomputed per atom from the
//     P slots in the order 0 ... P - 1;
//   * md_pimd_gate_kernel, ONE workgroup: the beads combined in the order 0 ... P - 1, the halts — overflow, covloss gate, with
//     nothing moved yet —, the row of sixteen scalars, the record of the evaluation and the mark;
//   * md_pimd_move_kernel, a tile of PIMD_TILE atoms per workgroup with x and v of all P beads of the tile in LDS: the closing
//     half kick of step n - 1 (`pending`), the opening half kick v += (dt/2) F_n / m, to normal modes (x~_k = sum_j C[j][k] x_j, the
//     same for v), A(dt/2) O A(dt/2) there — A the exact free ring polymer, O the Ornstein-Uhlenbeck step of every mode —, back
//     (x_j = sum_k C[j][k] x~_k), into the next slot of the rings.
// C, cos(w_k dt/2), sin(w_k dt/2) / w_k, w_k sin(w_k dt/2), c1_k and c2_k come from the host (sgpr_md_pimd, once per run): the
// device multiplies and adds.  Every mode sum runs sequentially in the order 0, 1, ..., P - 1 (s = C a_0; s = s + C a_j).  No
// float atomics, no contraction, true divisions: two runs give the same bits; at P = 1 (C = 1) the scheme is, operation for
// operation, md_baoab_advance.  Sums over atoms in md_fire_kernel's order (thread t adds the sorted atoms t, t + 256, ...,
// fin_wave_sum, the four waves pairwise), through the permutation: beads, velocities and results are in caller atom order.
#pragma once

#define PIMD_MAX 32     // beads of a polymer
#define PIMD_INFO 64    // doubles per evaluation of the record: E[PIMD_MAX] | covmax[PIMD_MAX]
#define PIMD_SUMS 8     // per bead: E, largest covloss, overflow, sum m v^2 closed, ... before the closing kick, (x - xbar).F, spring sum
#define PIMD_TILE 16    // atoms of a workgroup of the move kernel: x, v of P beads twice (beads | modes) and C in LDS, 56 KB at P = 32
// hbar in eV (A sqrt(amu / eV)) — the units of the run's masses, dt and kT —, CODATA 2014 as ase.units: workloads.HBAR
#define PIMD_HBAR 0.06465415105180661

// What the kernels share of an evaluation: the slots [P][N][3] of the rings of beads and velocities, the P packed results
// `plen` doubles apart (all caller atom order), the run's permutation (sorted -> caller), masses (sorted), dt / 2 and whether
// the closing half kick of this configuration is due.
struct PimdRing {
    int N, P;
    size_t plen;
    const double *x, *v, *pk;
    const int *perm;
    const double *mass;
    double hdt;
    int pending;
};

// Workgroup j: the sums of bead j.
__global__ __launch_bounds__(256) void md_pimd_sums_kernel(PimdRing b, double *sums, const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double wsum[5][4];
    const int tid = threadIdx.x, j = blockIdx.x, N = b.N, P = b.P;
    const size_t N3 = 3 * (size_t)N;
    const double *xj = b.x + N3 * j, *xn = b.x + N3 * (j + 1 < P ? j + 1 : 0), *vj = b.v + N3 * j, *pk = b.pk + b.plen * j;
    const double dP = (double)P;
    double s_kc = 0.0, s_kp = 0.0, s_cv = 0.0, s_sp = 0.0, bmx = 0.0;
    for (int k = tid; k < N; k += 256) {
        const size_t c = (size_t)b.perm[k];
        const double ms = b.mass[k];
        const double f0 = pk[3 * c], f1 = pk[3 * c + 1], f2 = pk[3 * c + 2];
        const double x0 = xj[3 * c], x1 = xj[3 * c + 1], x2 = xj[3 * c + 2];
        const double v0 = vj[3 * c], v1 = vj[3 * c + 1], v2 = vj[3 * c + 2];
        double m0 = b.x[3 * c], m1 = b.x[3 * c + 1], m2 = b.x[3 * c + 2];
        for (int q = 1; q < P; q++) {
            const double *xq = b.x + N3 * q + 3 * c;
            m0 = m0 + xq[0]; m1 = m1 + xq[1]; m2 = m2 + xq[2];
        }
        m0 = __ddiv_rn(m0, dP); m1 = __ddiv_rn(m1, dP); m2 = __ddiv_rn(m2, dP);
        const double d0 = x0 - m0, d1 = x1 - m1, d2 = x2 - m2;
        s_cv += (d0 * f0 + d1 * f1) + d2 * f2;
        const double e0 = x0 - xn[3 * c], e1 = x1 - xn[3 * c + 1], e2 = x2 - xn[3 * c + 2];
        s_sp += ms * ((e0 * e0 + e1 * e1) + e2 * e2);
        s_kp += ms * ((v0 * v0 + v1 * v1) + v2 * v2);
        double w0 = v0, w1 = v1, w2 = v2;
        if (b.pending) {
            w0 = v0 + __ddiv_rn(b.hdt * f0, ms); w1 = v1 + __ddiv_rn(b.hdt * f1, ms); w2 = v2 + __ddiv_rn(b.hdt * f2, ms);
        }
        s_kc += ms * ((w0 * w0 + w1 * w1) + w2 * w2);
        bmx = fmax(bmx, pk[3 * (size_t)N + c]);
    }
    s_kc = fin_wave_sum(s_kc); s_kp = fin_wave_sum(s_kp); s_cv = fin_wave_sum(s_cv); s_sp = fin_wave_sum(s_sp);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmx = fmax(bmx, __shfl_xor(bmx, o, 64));
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        wsum[0][w] = s_kc; wsum[1][w] = s_kp; wsum[2][w] = s_cv; wsum[3][w] = s_sp; wsum[4][w] = bmx;
    }
    __syncthreads();
    double *out = sums + PIMD_SUMS * j;
    if (tid < 4) out[3 + tid] = (wsum[tid][0] + wsum[tid][1]) + (wsum[tid][2] + wsum[tid][3]);
    else if (tid == 4) out[1] = fmax(fmax(wsum[4][0], wsum[4][1]), fmax(wsum[4][2], wsum[4][3]));
    else if (tid == 5) out[0] = pk[4 * (size_t)N];
    else if (tid == 6) out[2] = pk[4 * (size_t)N + 10];
    else if (tid == 7) out[7] = 0.0;
}

// Behind the sums of evaluation n of a polymer: the beads combined in the order 0 ... P - 1, the halts, the row, the record.
// The sixteen scalars: 0 the mean of the beads' energies, 1 the bead (1 ... P) with the largest covloss (the earlier one on a
// tie), 10 overflow, 11 largest covloss, 12 | 13 sum m v^2 over all beads after | before the closing half kick, 14 the
// centroid-virial kinetic energy 3 N kT / 2 - (1 / 2P) sum (x - xbar).F, 15 the spring energy; the others zero.
// kT: the physical one; wP2 = w_P^2.
__global__ __launch_bounds__(64) void md_pimd_gate_kernel(int N, int P, const double *sums, double kT, double wP2, double *info, double ediff, int *halt,
                                                         int *halt_host, int step, double *scal_row, int *mark)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    const int tid = threadIdx.x;
    if (tid < P) {
        info[tid] = sums[PIMD_SUMS * tid];
        info[PIMD_MAX + tid] = sums[PIMD_SUMS * tid + 1];
    }
    if (tid != 0) return;
    double E = sums[0], bmax = sums[1], ov = sums[2], kc = sums[3], kp = sums[4], cv = sums[5], sp = sums[6];
    int bb = 0;
    for (int j = 1; j < P; j++) {
        const double *s = sums + PIMD_SUMS * j;
        E = E + s[0];
        if (s[1] > bmax) { bmax = s[1]; bb = j; }
        ov = fmax(ov, s[2]);
        kc = kc + s[3]; kp = kp + s[4]; cv = cv + s[5]; sp = sp + s[6];
    }
    const double dP = (double)P;
    scal_row[0] = __ddiv_rn(E, dP); scal_row[1] = (double)(bb + 1);
    scal_row[10] = ov; scal_row[11] = bmax; scal_row[12] = kc; scal_row[13] = kp;
    scal_row[14] = (1.5 * (double)N) * kT - __ddiv_rn(cv, 2.0 * dP);
    scal_row[15] = (0.5 * wP2) * sp;
    int why = -1;   // halt_host word: 0 the covloss gate, 1 a capacity overflow
    if (ov != 0.0) why = 1;
    else if (bmax >= ediff) why = 0;
    if (why >= 0) {
        atomicMin(halt, step);
        halt_host[why] = step;
    }
    *mark = 1;
}

// The move out of an evaluation that md_pimd_gate_kernel has let pass.  Workgroup t: the sorted atoms PIMD_TILE t ... ; element
// e = q W + r of a [P][W] array (W = 3 PIMD_TILE) is component r % 3 of tile atom r / 3 at bead or mode q, one thread per element
// in trips of 256.  tab: C[P][P] | cos | sin / w | w sin | c1 | c2, P each; sq: sqrt(kT_P / m), sorted; noise: the deviates of
// this evaluation [P][N][3] (mode k, caller atom order; null: none — or, with a seed, drawn here: md_deviate of
// t = n P + k).  A halted run (at this evaluation or before it) moves nothing.
struct PimdMove {
    const double *sq, *tab, *noise;
    double *x_next, *v_next;
    unsigned long long seed;
    long long n;
};
__global__ __launch_bounds__(256) void md_pimd_move_kernel(PimdRing b, PimdMove a, const int *halt, int step)
{
#pragma clang fp contract(off)
    extern __shared__ double pimd_lds[];
    const int P = b.P, N = b.N, tid = threadIdx.x, W = 3 * PIMD_TILE, tot = P * W, i0 = blockIdx.x * PIMD_TILE;
    if (*halt <= step) return;   // (the same word for every thread: nobody waits at a barrier)
    double *ax = pimd_lds, *av = ax + tot, *bx = av + tot, *bv = bx + tot, *cm = bv + tot;
    const size_t N3 = 3 * (size_t)N;
    for (int e = tid; e < P * P; e += 256) cm[e] = a.tab[e];
    for (int e = tid; e < tot; e += 256) {
        const int j = e / W, r = e - j * W, at = r / 3, comp = r - 3 * at, i = i0 + at;
        double x = 0.0, v2 = 0.0;
        if (i < N) {
            const size_t c = (size_t)b.perm[i];
            const double ms = b.mass[i], F = b.pk[b.plen * j + 3 * c + comp], vc = b.v[N3 * j + 3 * c + comp];
            x = b.x[N3 * j + 3 * c + comp];
            const double kick = __ddiv_rn(b.hdt * F, ms);
            double v = vc;
            if (b.pending) v = v + kick;   // closes step n - 1
            v2 = v + kick;                 // B
        }
        ax[e] = x; av[e] = v2;
    }
    __syncthreads();
    const double *cs = a.tab + P * P, *sn = cs + P, *wsn = sn + P, *c1 = wsn + P, *c2 = c1 + P;
    for (int e = tid; e < tot; e += 256) {
        const int k = e / W, r = e - k * W, at = r / 3, comp = r - 3 * at, i = i0 + at;
        double xt = cm[k] * ax[r], vt = cm[k] * av[r];
        for (int j = 1; j < P; j++) {
            const double cc = cm[j * P + k];
            xt = xt + cc * ax[j * W + r];
            vt = vt + cc * av[j * W + r];
        }
        const double ck = cs[k], sk = sn[k], wk = wsn[k];
        if (k == 0) xt = xt + b.hdt * vt;   // A: the centroid drifts
        else {
            const double xa = ck * xt + sk * vt, va = ck * vt - wk * xt;
            xt = xa; vt = va;
        }
        double nz = 0.0, sg = 0.0;
        if (i < N) {
            const int c = b.perm[i];
            sg = c2[k] * a.sq[i];
            if (a.noise) nz = a.noise[N3 * k + 3 * (size_t)c + comp];
            else if (a.seed != 0ull && sg != 0.0) nz = md_deviate(a.seed, a.n * (long long)P + k, c, comp);
        }
        vt = c1[k] * vt + sg * nz;          // O
        if (k == 0) xt = xt + b.hdt * vt;   // A
        else {
            const double xa = ck * xt + sk * vt, va = ck * vt - wk * xt;
            xt = xa; vt = va;
        }
        bx[e] = xt; bv[e] = vt;
    }
    __syncthreads();
    for (int e = tid; e < tot; e += 256) {
        const int j = e / W, r = e - j * W, at = r / 3, comp = r - 3 * at, i = i0 + at;
        double xo = cm[j * P] * bx[r], vo = cm[j * P] * bv[r];
        for (int k = 1; k < P; k++) {
            const double cc = cm[j * P + k];
            xo = xo + cc * bx[k * W + r];
            vo = vo + cc * bv[k * W + r];
        }
        if (i < N) {
            const size_t o = N3 * j + 3 * (size_t)b.perm[i] + comp;
            a.x_next[o] = xo; a.v_next[o] = vo;
        }
    }
}
