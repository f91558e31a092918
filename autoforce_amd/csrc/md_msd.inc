// md_msd.inc — mean-square displacements accumulated inside the device MD loop (sgpr_md_msd): what the reference works out of
// a stored trajectory (theforce/analysis/analysis.py:109-176: `correlator` — the tracer MSD mean_i |dr_i|^2 and the collective
// "smd" |sum_i dr_i|^2 / n of a species —, get_exponential_deltas: lags in powers of two, :296-338: diffusion_constants) is
// here a table in HBM that the run fills as it goes, behind the evaluations it samples, with no host traffic until it is read.
//   Sample s is configuration n = s every of the run.  Level l (l < L) has the lag 2^l samples and keeps ONE origin O_l [N][3]
// (sorted atom order, like the X ring beside it).  At sample s every level with s mod 2^l == 0 is DUE: if s >= 2^l (s > 0: the
// due levels of a sample are l <= ctz(s), all of them old enough) it measures d_i = x_i - O_l,i — per species z of the model's
// table with n_z atoms in the frame A = sum |d_i|^2, B = sum d_i, and over all atoms c = sum m_i d_i / sum m_i (com; else 0) —
//     msd = ((A - 2 c.B) + n_z |c|^2) / n_z      (mean |d_i - c|^2)
//     smd = |B - n_z c|^2 / n_z                  (the reference's correlator of the centred displacements)
// and the row (l, z) gains msd, msd^2, smd, smd^2, count[l] gains 1; then O_l <- x.  The windows of a level do not overlap:
// its samples are independent blocks, sqrt(var / count) is an error bar.  The positions of the ring are never wrapped (the wrap
// lives in the bin records) and a held component keeps its bits, so d = 0 there.  workloads.MsdBlocks is the host twin and the
// definition: the same operations in the same order.
//   Two launches behind a sampled evaluation, whatever the number of due levels:
//   * md_msd_part_kernel, one workgroup of 256 per CHUNK — MSD_CHUNK consecutive sorted atoms of one species (the host lists the
//     chunks at the attach; a species' last chunk is ragged), one atom per thread: x from the ring once, then per due level O_l
//     read, seven partial sums (A, B[3], sum m d [3]: fin_wave_sum per wave, the four waves pairwise) and O_l <- x.  Ring and
//     origins are both in sorted order: no permutation, consecutive threads touch consecutive rows.
//   * md_msd_fold_kernel, one workgroup: the chunk partials of a species in ascending chunk order, sum m d over the species in
//     table order, c, msd, smd, the table, the counts, and the device word next_due += every.
// Both leave at once when the run has halted before this evaluation (the halt word as md_record_kernel reads it: the
// speculative evaluation behind a covloss halt stays out) and when n != next_due: a configuration that is evaluated twice — the
// repeat behind a covloss halt or an overflow — counts once.  No float atomics, no contraction, true divisions.
#pragma once

#define MSD_CHUNK 256   // atoms per chunk: one per thread of md_msd_part_kernel
#define MSD_MAXL 32     // levels (a mask of 32 bits names the due ones)
#define MSD_PART 7      // A | B[3] | sum m d [3]

// chunk: [nch][2] first atom and atoms of the chunk.  origin: [L][N][3] (lstride = 3N), part: [L][nch][MSD_PART].  due: the
// levels of this sample; acc: it measures (s > 0) — sample 0 only sets the origins.  ctl[0]: next_due.
__global__ __launch_bounds__(256) void md_msd_part_kernel(const int *__restrict__ chunk, int nch, const double *__restrict__ x,
                                                          const double *__restrict__ mass, double *__restrict__ origin, size_t lstride,
                                                          unsigned due, int acc, double *__restrict__ part, const long long *ctl, long long n,
                                                          const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double ws[MSD_MAXL][4][MSD_PART];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int len = chunk[2 * c + 1];
    const bool in = tid < len;
    const size_t i3 = 3 * ((size_t)chunk[2 * c] + (in ? tid : 0));
    const double x0 = x[i3], x1 = x[i3 + 1], x2 = x[i3 + 2];
    const double mi = mass[i3 / 3];
    for (int l = 0; l < MSD_MAXL; l++) {
        if (!((due >> l) & 1u)) continue;
        double *o = origin + lstride * l + i3;
        if (acc) {
#pragma clang fp contract(off)
            double d0 = x0 - o[0], d1 = x1 - o[1], d2 = x2 - o[2];
            if (!in) d0 = d1 = d2 = 0.0;
            double s[MSD_PART] = {(d0 * d0 + d1 * d1) + d2 * d2, d0, d1, d2, mi * d0, mi * d1, mi * d2};
#pragma unroll
            for (int k = 0; k < MSD_PART; k++) {
                const double t = fin_wave_sum(s[k]);
                if ((tid & 63) == 0) ws[l][tid >> 6][k] = t;
            }
        }
        if (in) { o[0] = x0; o[1] = x1; o[2] = x2; }
    }
    if (!acc) return;
    __syncthreads();
    if (tid < MSD_MAXL * MSD_PART) {
        const int l = tid / MSD_PART, k = tid - MSD_PART * l;
        if ((due >> l) & 1u) part[((size_t)l * nch + c) * MSD_PART + k] = (ws[l][0][k] + ws[l][1][k]) + (ws[l][2][k] + ws[l][3][k]);
    }
}


// One row of the table: species z of a due level from that level's sums sl [S][MSD_PART] (c: over the species in table order).
__device__ __forceinline__ void msd_fold_row(const double *sl, int z, int S, double fn, double mtot, int com, double *row)
{
#pragma clang fp contract(off)
    const double *sz = sl + z * MSD_PART;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (com) {
        for (int q = 0; q < S; q++) { c0 = c0 + sl[q * MSD_PART + 4]; c1 = c1 + sl[q * MSD_PART + 5]; c2 = c2 + sl[q * MSD_PART + 6]; }
        c0 = c0 / mtot; c1 = c1 / mtot; c2 = c2 / mtot;
    }
    const double cB = (c0 * sz[1] + c1 * sz[2]) + c2 * sz[3], cc = (c0 * c0 + c1 * c1) + c2 * c2;
    const double msd = ((sz[0] - 2.0 * cB) + fn * cc) / fn;
    const double e0 = sz[1] - fn * c0, e1 = sz[2] - fn * c1, e2 = sz[3] - fn * c2;
    const double smd = ((e0 * e0 + e1 * e1) + e2 * e2) / fn;
    row[0] = row[0] + msd; row[1] = row[1] + msd * msd; row[2] = row[2] + smd; row[3] = row[3] + smd * smd;
}

// coff: [S + 1] the chunks of species z are coff[z] ... coff[z + 1] - 1; nz: [S] its atoms (0: the row keeps its zeros).  table:
// [L][S][4] sums of msd, msd^2, smd, smd^2; ctl: next_due | count[L].  Dynamic LDS: L S MSD_PART doubles, the species' sums of
// the due levels.
__global__ __launch_bounds__(256) void md_msd_fold_kernel(const int *__restrict__ coff, const int *__restrict__ nz, int nch, int S, int L,
                                                          double mtot, int com, unsigned due, int acc, const double *__restrict__ part,
                                                          double *__restrict__ table, long long *ctl, long long n, int every, const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    extern __shared__ double msd_sums[];
    const int tid = threadIdx.x;
    if (acc) {
        for (int e = tid; e < L * S * MSD_PART; e += 256) {
            const int l = e / (S * MSD_PART), z = (e / MSD_PART) % S, k = e % MSD_PART;
            if (!((due >> l) & 1u)) continue;
            const double *p = part + (size_t)l * nch * MSD_PART + k;
            double s = 0.0;
#pragma unroll 8
            for (int c = coff[z]; c < coff[z + 1]; c++) s += p[(size_t)c * MSD_PART];
            msd_sums[e] = s;
        }
        __syncthreads();
        for (int e = tid; e < L * S; e += 256) {
            const int l = e / S, z = e - S * l;
            if (((due >> l) & 1u) && nz[z] > 0)
                msd_fold_row(msd_sums + (size_t)l * S * MSD_PART, z, S, (double)nz[z], mtot, com, table + 4 * (size_t)e);
        }
        if (tid < L && ((due >> tid) & 1u)) ctl[1 + tid] += 1;
    }
    __syncthreads();   // (every thread has read next_due)
    if (tid == 0) ctl[0] = n + every;
}
