// md_vacf.inc — velocity autocorrelations accumulated inside the device MD loop (sgpr_md_vacf).  The reference has none
// (theforce/analysis has `correlator` for displacements only): the definition is ours, workloads.VacfRing is the host twin and
// the definition, and these kernels are held to it bit for bit.
//   Sample s is configuration n = s every of the run.  Its velocity v(s) is the one an observer sees, what sgpr_md_velocities
// returns had the call ended with that evaluation: Langevin / velocity Verlet v_pre + hdt F / m (n > 0; v_pre at n = 0) with F the
// evaluation's packed force; Nose-Hoover the centred velocity the last kernel writes into V slot n; a held component exactly 0.
// For every sample s, lag k < lags and origin o = s - k with o >= 0 and o mod origin_every == 0, per species z of the model's
// table with n_z atoms in the frame, J_z(s) = sum_z v_i(s) and c_s = sum_all m_i v_i(s) / sum_all m_i (com; else 0):
//     A         = sum_z ((v_i0(s) v_i0(o) + v_i1(s) v_i1(o)) + v_i2(s) v_i2(o))
//     tr[k][z] += ((A - (c_s.J_z(o) + c_o.J_z(s))) + n_z (c_s.c_o)) / n_z          (mean over z of (v_i(s) - c_s).(v_i(o) - c_o))
//     col[k][a][b] += e_a(s).e_b(o),  e_z = J_z - n_z c                            (the full S x S block)
//     count[k] += 1
//   A sample is taken in two parts, because v(s) depends on F and a covloss halt makes the next call evaluate the configuration
// again with the updated model, while the halt of an evaluation is known only behind the next one:
//   * STORE, behind every evaluation of a sampled configuration that the halt word does not skip: v(s) and the chunk parts of J
//     and sum m v go into slot s mod (lags + 1) of a ring.  Idempotent, not gated by next_due: the repeat behind a halt or an
//     overflow overwrites the slot with the values that stand.
//   * CORRELATE, in the same place, gated by next_due == n (once per sample): sample s - 1 is final — the run has moved past it —
//     and is the current one: its J and c are folded into their own rings, all its due lags are accumulated, next_due += every.
//     Sample 0 only stores; the last stored sample of a run stays pending.  With lags + 1 slots the oldest origin of s - 1 is
//     slot (s + 1) mod (lags + 1), never the slot being written.
//   Four launches behind a sampled evaluation:
//   * md_vacf_store_kernel, one workgroup of 256 per CHUNK — VACF_CHUNK consecutive sorted atoms of one species (listed by the
//     host at the attach; a species' last chunk is ragged), one atom per thread: V slot n in sorted order, the kick from the packed
//     force through the permutation, the mask; the ring slot and six block sums (v[3], m v[3]: fin_wave_sum per wave, the four
//     waves pairwise).
//   * md_vacf_corr_kernel, grid (chunks, lag groups of VACF_GROUP): the atom's current velocity in registers, per due lag of the
//     group the origin row, the dot product and its block sum into part[k][chunk].
//   * md_vacf_fold_kernel, one workgroup per VACF_FOLD lags: chunk partials in ascending order, species in table order; J and c
//     of the current sample (every workgroup forms them, the first writes them into the rings), tr, col, count.
//   * md_vacf_done_kernel, one workgroup: samples += 1, next_due += every — behind the fold, so that no workgroup writes ctl[0]
//     while another of the same launch may still read it.
// All leave at once when the run has halted before this evaluation.  No float atomics, no contraction, true divisions.
#pragma once

#define VACF_CHUNK 256     // atoms per chunk: one per thread
#define VACF_GROUP 8       // lags per workgroup of md_vacf_corr_kernel
#define VACF_FOLD 16       // lags per workgroup of md_vacf_fold_kernel
#define VACF_MAXLAGS 8192  // lags of a table
#define VACF_MAXBYTES (4ull << 30)   // bytes of the velocity ring, (lags + 1) 24 N

// chunk: [nch][2] first atom and atoms of the chunk.  v: V slot n, sorted order.  force: the packed forces of the evaluation in
// caller order (null: no kick — Nose-Hoover, or configuration 0), perm: sorted -> caller.  fixed: [N][3] sorted, or null.
// ring: slot s of the velocity ring [N][3]; vpart: slot s of [nch][6].
__global__ __launch_bounds__(256) void md_vacf_store_kernel(const int *__restrict__ chunk, const double *__restrict__ v,
                                                            const double *__restrict__ force, const int *__restrict__ perm,
                                                            const double *__restrict__ mass, const unsigned char *__restrict__ fixed, double hdt,
                                                            double *__restrict__ ring, double *__restrict__ vpart, const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double ws[4][6];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int len = chunk[2 * c + 1];
    const bool in = tid < len;
    const size_t i = (size_t)chunk[2 * c] + (in ? tid : 0), i3 = 3 * i;
    double v0 = v[i3], v1 = v[i3 + 1], v2 = v[i3 + 2];
    const double mi = mass[i];
    if (force) {
        const size_t p3 = 3 * (size_t)perm[i];
        v0 = v0 + __ddiv_rn(hdt * force[p3], mi); v1 = v1 + __ddiv_rn(hdt * force[p3 + 1], mi); v2 = v2 + __ddiv_rn(hdt * force[p3 + 2], mi);
    }
    if (fixed) {
        if (fixed[i3]) v0 = 0.0;
        if (fixed[i3 + 1]) v1 = 0.0;
        if (fixed[i3 + 2]) v2 = 0.0;
    }
    if (in) { ring[i3] = v0; ring[i3 + 1] = v1; ring[i3 + 2] = v2; }
    else v0 = v1 = v2 = 0.0;
    const double s[6] = {v0, v1, v2, mi * v0, mi * v1, mi * v2};
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double t = fin_wave_sum(s[k]);
        if ((tid & 63) == 0) ws[tid >> 6][k] = t;
    }
    __syncthreads();
    if (tid < 6) vpart[(size_t)6 * c + tid] = (ws[0][tid] + ws[1][tid]) + (ws[2][tid] + ws[3][tid]);
}

// The due lags of the current sample p = s - 1 (slot p mod slots of ring [slots][N][3], sstride = 3N): part[k][chunk] for the
// lags k of group blockIdx.y whose origin o = p - k exists and has o mod origin_every == 0.  ctl[0]: next_due.
__global__ __launch_bounds__(256) void md_vacf_corr_kernel(const int *__restrict__ chunk, int nch, const double *__restrict__ ring, size_t sstride,
                                                           int slots, long long p, int lags, int origin_every, double *__restrict__ part,
                                                           const long long *ctl, long long n, const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double ws[VACF_GROUP][4];
    const int tid = threadIdx.x, c = blockIdx.x, k0 = blockIdx.y * VACF_GROUP;
    const int len = chunk[2 * c + 1];
    const bool in = tid < len;
    const size_t i3 = 3 * ((size_t)chunk[2 * c] + (in ? tid : 0));
    const double *cur = ring + sstride * (size_t)(p % slots) + i3;
    const double v0 = cur[0], v1 = cur[1], v2 = cur[2];
    for (int g = 0; g < VACF_GROUP; g++) {
        const long long o = p - (k0 + g);
        if (k0 + g >= lags || o < 0 || o % origin_every != 0) continue;
        const double *w = ring + sstride * (size_t)(o % slots) + i3;
        double d = (v0 * w[0] + v1 * w[1]) + v2 * w[2];
        if (!in) d = 0.0;
        const double t = fin_wave_sum(d);
        if ((tid & 63) == 0) ws[g][tid >> 6] = t;
    }
    __syncthreads();
    if (tid < VACF_GROUP) {
        const long long o = p - (k0 + tid);
        if (k0 + tid < lags && o >= 0 && o % origin_every == 0)
            part[(size_t)(k0 + tid) * nch + c] = (ws[tid][0] + ws[tid][1]) + (ws[tid][2] + ws[tid][3]);
    }
}

// coff: [S + 1] the chunks of species z are coff[z] ... coff[z + 1] - 1; nz: [S] its atoms (0: its tracer row keeps its zeros).
// vpart: [slots][nch][6]; jring: [slots][S][3], cring: [slots][3] — J and c of the samples that have been current.  tr:
// [lags][S], col: [lags][S][S]; ctl: next_due | samples | count[lags].  Dynamic LDS: 6 S + 3 doubles.  Lag 0 reads J and c of
// the current sample from LDS, a later lag those of its origin from the rings, where an earlier launch has put them.
__global__ __launch_bounds__(256) void md_vacf_fold_kernel(const int *__restrict__ coff, const int *__restrict__ nz, int nch, int S, int lags,
                                                           int origin_every, int slots, long long p, double mtot, int com,
                                                           const double *__restrict__ vpart, const double *__restrict__ part, double *jring,
                                                           double *cring, double *__restrict__ tr, double *__restrict__ col, long long *ctl,
                                                           long long n, const int *halt, int step)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    if (ctl[0] != n) return;
    extern __shared__ double vacf_sums[];   // [S][6] | c[3]
    double *cp = vacf_sums + 6 * S;
    const int tid = threadIdx.x, k0 = blockIdx.x * VACF_FOLD;
    const size_t sp = (size_t)(p % slots);
    for (int e = tid; e < 6 * S; e += 256) {
        const int z = e / 6, k = e - 6 * z;
        const double *q = vpart + sp * nch * 6 + k;
        double s = 0.0;
        for (int c = coff[z]; c < coff[z + 1]; c++) s = s + q[(size_t)c * 6];
        vacf_sums[e] = s;
    }
    __syncthreads();
    if (tid < 3) {
        double c = 0.0;
        if (com) {
            for (int z = 0; z < S; z++) c = c + vacf_sums[6 * z + 3 + tid];
            c = c / mtot;
        }
        cp[tid] = c;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int e = tid; e < 3 * S; e += 256) jring[sp * 3 * S + e] = vacf_sums[6 * (e / 3) + e % 3];
        if (tid < 3) cring[sp * 3 + tid] = cp[tid];
    }
    const double c0 = cp[0], c1 = cp[1], c2 = cp[2];
    for (int e = tid; e < VACF_FOLD * S * S; e += 256) {
        const int k = k0 + e / (S * S), a = (e / S) % S, b = e % S;
        const long long o = p - k;
        if (k >= lags || o < 0 || o % origin_every != 0) continue;
        const size_t so = (size_t)(o % slots);
        const double *Jb = k == 0 ? vacf_sums + 6 * b : jring + so * 3 * S + 3 * b;
        const double *co = k == 0 ? cp : cring + so * 3;
        const double *Ja = vacf_sums + 6 * a;
        const double fa = (double)nz[a], fb = (double)nz[b];
        const double o0 = co[0], o1 = co[1], o2 = co[2];
        const double ea0 = Ja[0] - fa * c0, ea1 = Ja[1] - fa * c1, ea2 = Ja[2] - fa * c2;
        const double eb0 = Jb[0] - fb * o0, eb1 = Jb[1] - fb * o1, eb2 = Jb[2] - fb * o2;
        double *q = col + ((size_t)k * S + a) * S + b;
        *q = *q + ((ea0 * eb0 + ea1 * eb1) + ea2 * eb2);
        if (a == b && nz[a] > 0) {
            const double *pa = part + (size_t)k * nch;
            double A = 0.0;
            for (int c = coff[a]; c < coff[a + 1]; c++) A = A + pa[c];
            const double cJo = (c0 * Jb[0] + c1 * Jb[1]) + c2 * Jb[2], oJs = (o0 * Ja[0] + o1 * Ja[1]) + o2 * Ja[2];
            const double cc = (c0 * o0 + c1 * o1) + c2 * o2;
            double *t = tr + (size_t)k * S + a;
            *t = *t + ((A - (cJo + oJs)) + fa * cc) / fa;
        }
    }
    if (tid < VACF_FOLD) {
        const int k = k0 + tid;
        const long long o = p - k;
        if (k < lags && o >= 0 && o % origin_every == 0) ctl[2 + k] += 1;
    }
}

// The sample is counted: behind the correlate launches of configuration n (corr: they ran, s > 0), one workgroup.
__global__ __launch_bounds__(64) void md_vacf_done_kernel(long long *ctl, long long n, int every, int corr, const int *halt, int step)
{
    if (*halt < step) return;
    if (threadIdx.x != 0 || ctl[0] != n) return;
    if (corr) ctl[1] += 1;
    ctl[0] = n + every;
}
