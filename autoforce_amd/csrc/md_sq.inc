// md_sq.inc — partial structure factors and coherent intermediate scattering functions accumulated inside the device MD loop
// (sgpr_md_sq).  The reference has nothing in reciprocal space: the definition is ours, workloads.SqRing is the host twin.
//   Wave vectors are vectors of the reciprocal lattice of the run's constant cell: q_j = 2 pi hkl_j inv(cell)^T, so that
// q_j . r = 2 pi hkl_j . s with s = r inv(cell) — wrapped and unwrapped positions give the same phases, and the X ring, which is
// never wrapped, is read as it is.  Sample s is configuration n = s every.  Per atom f = s - rint(s) per axis and
// e_a = exp(2 pi i f_a); per species z of the model's table
//     rho_z(q_j; s) = sum_{i in z} e_0^h e_1^k e_2^l                          (a negative index: the conjugate of the power)
// and for every lag k < lags and origin o = s - k with o >= 0 and o mod origin_every == 0
//     f[k][j][a][b] += Re(rho_a(q_j; s) conj rho_b(q_j; o)),  count[k] += 1    (the full S x S block: a != b is not symmetric at k > 0)
// and per sample mean[j][a] += rho_a(q_j; s) (complex), samples += 1.  Lag 0 is the static S_ab.
//   A configuration's positions do not depend on the model, so the sample is taken at the configuration's first evaluation and
// gated by next_due, as md_msd.inc's: the repeat behind a covloss halt or an overflow counts nothing, nothing is left pending.
//   UNLIKE the other accumulators the device is NOT held to the twin bit for bit: the device's sincospi and numpy's sin and cos
// are different libraries, and the products below may contract into fused multiply-adds.  It is held to an a-priori bound,
//     |d rho_z(q)| <= B_z = 128 hmax (1 + smax) n_z 2^-52          (hmax: the largest |index|, smax: the largest |s| fed)
//     |d f[k][j][a][b]| <= count[k] (n_a B_b + n_b B_a + count[k] n_a n_b 2^-52)
// (a phase error of 2 pi (|h| + |k| + |l|) roundings of a three-term scaled coordinate, a few roundings per power, that much on
// both sides), and to itself exactly: no float atomics, every sum in a fixed order — the tables have the same bits run after
// run and however the run is cut.  Integers (count, samples, next_due) equal the twin's.
//   Three launches behind a sampled evaluation:
//   * md_sq_part_kernel<W, P>, grid (chunks, tiles of SQ_TILE wave vectors): a chunk is at most W consecutive sorted atoms of one
//     species (md_species_chunks).  Phase 1, a thread per (atom, axis) — the atom's three axes side by side, so that the serial
//     part ahead of the barrier is a third as long as with a thread per atom: the scaled coordinate from the uploaded inverse
//     cell, f, ONE sincospi(2 f), and the powers 0 ... P - 1 by repeated complex multiplication into LDS [atom][axis][power] —
//     the Ewald way: three transcendental pairs per atom, not one per (atom, q).  Phase 2, a thread per wave vector: it walks
//     the chunk's atoms in ascending order, multiplies the three table entries (conjugating for a negative index), adds into
//     two registers and writes part[chunk][j][2].  No cross-lane reduction.  The lanes of a wave read the same atom at different
//     powers: with the power index fastest and 16 B per entry, equal powers are one address (a broadcast) and the 17 powers of
//     the wide form span 272 B — one 256-B bank row and a slot: at most two addresses on a bank within a 16-lane group of
//     ds_read_b128; the 33 powers of the narrow form span 528 B, at most three.
//     Two forms keep the tables within 64 KiB: <64, 17> where every |index| <= 16 (52 224 B), <32, 33> up to 32 (50 688 B).
//   * md_sq_fold_kernel, grid (tiles, groups of SQ_FOLD lags), a thread per wave vector: the chunk partials of every species
//     in ascending chunk order (every lag group repeats this, as md_vacf_fold_kernel repeats J) into LDS [S][2][SQ_TILE] — a
//     thread reads its own column only, LDS is the run-time indexed store that registers must not be.  Lag group 0 writes the
//     current rho into slot s mod lags of the ring [lags][nq][S][2] and adds it to mean.  Every group adds its due lags to f:
//     lag 0 from its own values, lag k >= 1 from slot (s - k) mod lags, which an earlier launch wrote; the slot being written
//     is that of s - lags, which no lag reads: no workgroup depends on another of the same launch.
//   * md_sq_done_kernel, one workgroup: count[k] of the due lags, samples += 1, next_due += every — behind the fold, so that no
//     workgroup writes ctl[0] while another of an earlier launch of the sample may still read it (md_vacf_done_kernel).
// All leave at once when the run has halted before this evaluation and when n != next_due.
#pragma once

#define SQ_TILE 256          // wave vectors per workgroup: one per thread
#define SQ_FOLD 8            // lags per workgroup of md_sq_fold_kernel
#define SQ_MAXQ 8192         // wave vectors of a table
#define SQ_MAXLAGS 8192      // lags of a table
#define SQ_MAXH 32           // |index| of a wave vector
#define SQ_WIDE_H 16         // up to here the wide form: 64 atoms per chunk
#define SQ_MAXBYTES (1ull << 30)   // bytes of f and the ring together

// chunk: [nch][2] first atom and atoms of the chunk (at most W).  x: the X slot of configuration n, sorted order.  inv: [3][3]
// with s_c = (x0 inv[0][c] + x1 inv[1][c]) + x2 inv[2][c].  hkl: [nq][3], every |index| < P.  part: [nch][nq][2].  ctl[0]: next_due.
template <int W, int P>
__global__ __launch_bounds__(256) void md_sq_part_kernel(const int *__restrict__ chunk, const double *__restrict__ x, const double *__restrict__ inv,
                                                         const int *__restrict__ hkl, int nq, double *__restrict__ part, const long long *ctl,
                                                         long long n, const int *halt, int step)
{
    static_assert(3 * W <= 256 && (size_t)W * 3 * P * sizeof(double2) <= 65536, "a thread per (atom, axis); the tables within 64 KiB");
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double2 tab[W * 3 * P];   // [atom][axis][power]
    const int tid = threadIdx.x, c = blockIdx.x;
    const int first = chunk[2 * c], len = min(chunk[2 * c + 1], W);
    if (tid < 3 * len) {
        const int a = tid / 3, ax = tid - 3 * a;
        const double *r = x + 3 * ((size_t)first + a);
        const double s = (r[0] * inv[ax] + r[1] * inv[3 + ax]) + r[2] * inv[6 + ax];
        const double f = s - rint(s);
        double sn, cs;
        sincospi(2.0 * f, &sn, &cs);
        double2 *t = tab + (a * 3 + ax) * P;
        double pr = 1.0, pi = 0.0;
        t[0] = make_double2(1.0, 0.0);
        for (int p = 1; p < P; p++) {
            const double nr = pr * cs - pi * sn, ni = pr * sn + pi * cs;
            pr = nr; pi = ni;
            t[p] = make_double2(pr, pi);
        }
    }
    __syncthreads();
    const int j = blockIdx.y * SQ_TILE + tid;
    if (j >= nq) return;
    const int h = hkl[3 * j], k = hkl[3 * j + 1], l = hkl[3 * j + 2];
    const int ah = min(abs(h), P - 1), ak = P + min(abs(k), P - 1), al = 2 * P + min(abs(l), P - 1);
    const double sh = h < 0 ? -1.0 : 1.0, sk = k < 0 ? -1.0 : 1.0, sl = l < 0 ? -1.0 : 1.0;
    double re = 0.0, im = 0.0;
    for (int a = 0; a < len; a++) {
        const double2 *t = tab + a * 3 * P;
        const double2 u = t[ah], v = t[ak], w = t[al];
        const double ui = sh * u.y, vi = sk * v.y, wi = sl * w.y;
        const double pr = u.x * v.x - ui * vi, pi = u.x * vi + ui * v.x;
        re = re + (pr * w.x - pi * wi);
        im = im + (pr * wi + pi * w.x);
    }
    double2 *out = (double2 *)part + (size_t)c * nq + j;
    *out = make_double2(re, im);
}

// coff: [S + 1] the chunks of species z are coff[z] ... coff[z + 1] - 1 (none: rho_z = 0).  part: [nch][nq][2] of this sample s;
// ring: [lags][nq][S][2], mean: [nq][S][2], f: [lags][nq][S][S].  Dynamic LDS: 2 S SQ_TILE doubles.  No barrier: a thread reads
// back only what it wrote.
__global__ __launch_bounds__(256) void md_sq_fold_kernel(const int *__restrict__ coff, int S, int nq, int lags, int origin_every, long long s,
                                                         const double *__restrict__ part, double *ring, double *__restrict__ mean,
                                                         double *__restrict__ f, const long long *ctl, long long n, const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    extern __shared__ double sq_cur[];   // [S][2][SQ_TILE]
    const int tid = threadIdx.x, j = blockIdx.x * SQ_TILE + tid, k0 = blockIdx.y * SQ_FOLD;
    if (j >= nq) return;
    const double2 *pj = (const double2 *)part + j;
    for (int z = 0; z < S; z++) {
        double re = 0.0, im = 0.0;
        for (int c = coff[z]; c < coff[z + 1]; c++) {
            const double2 v = pj[(size_t)c * nq];
            re = re + v.x; im = im + v.y;
        }
        sq_cur[(2 * z) * SQ_TILE + tid] = re;
        sq_cur[(2 * z + 1) * SQ_TILE + tid] = im;
    }
    if (blockIdx.y == 0) {
        double2 *slot = (double2 *)ring + ((size_t)(s % lags) * nq + j) * S, *mj = (double2 *)mean + (size_t)j * S;
        for (int z = 0; z < S; z++) {
            const double re = sq_cur[(2 * z) * SQ_TILE + tid], im = sq_cur[(2 * z + 1) * SQ_TILE + tid];
            slot[z] = make_double2(re, im);
            const double2 m0 = mj[z];
            mj[z] = make_double2(m0.x + re, m0.y + im);
        }
    }
    for (int g = 0; g < SQ_FOLD; g++) {
        const int k = k0 + g;
        const long long o = s - k;
        if (k >= lags || o < 0 || o % origin_every != 0) continue;
        const double2 *org = (const double2 *)ring + ((size_t)(o % lags) * nq + j) * S;   // (k = 0: not read)
        double *fk = f + ((size_t)k * nq + j) * S * S;
        for (int b = 0; b < S; b++) {
            double br, bi;
            if (k == 0) { br = sq_cur[(2 * b) * SQ_TILE + tid]; bi = sq_cur[(2 * b + 1) * SQ_TILE + tid]; }
            else { const double2 v = org[b]; br = v.x; bi = v.y; }
            for (int a = 0; a < S; a++) {
                const double ar = sq_cur[(2 * a) * SQ_TILE + tid], ai = sq_cur[(2 * a + 1) * SQ_TILE + tid];
                fk[a * S + b] = fk[a * S + b] + (ar * br + ai * bi);
            }
        }
    }
}

// The sample is counted: behind the fold of configuration n, one workgroup.  ctl: next_due | samples | count[lags].
__global__ __launch_bounds__(256) void md_sq_done_kernel(long long *ctl, long long n, int every, int lags, int origin_every, long long s,
                                                         const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    for (int k = threadIdx.x; k < lags; k += 256) {
        const long long o = s - k;
        if (o >= 0 && o % origin_every == 0) ctl[2 + k] += 1;
    }
    __syncthreads();   // (every thread has read next_due)
    if (threadIdx.x == 0) { ctl[1] += 1; ctl[0] = n + every; }
}
