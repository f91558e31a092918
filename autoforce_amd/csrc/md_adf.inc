// md_adf.inc — bond-angle and coordination distributions accumulated inside the device MD loop (sgpr_md_adf): the three-body
// structure of a run — are the tetrahedra intact, which corners do they share, how many neighbours sit around an ion — as tables
// of integers in HBM that the run fills behind the evaluations it samples.  The reference has no angular analysis
// (theforce/analysis stops at rdf and the displacements): workloads.AdfCounts is the host twin and the definition.
//   cut [S][S] is a symmetric table of bond cutoffs over the species slots of the model's table (0: the pair never bonds; every
// entry <= rc, so that the step's own neighbour list holds every candidate).  For a sampled configuration and a centre i of species
// a, its NEIGHBOURS are all (j of species b, s in Z^3) with (j, s) != (i, 0) and
//     d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),   r = sqrt((d0 d0 + d1 d1) + d2 d2),   r < cut[a][b]
// (the expression meta_ql_gather and md_rdf.inc share; s = 0 along an open direction; periodic self-images and several images of
// one atom are distinct neighbours).  For every unordered pair {t, t'} of distinct neighbours, species b <= c after ordering,
//     q = (d_t0 d_t'0 + d_t1 d_t'1) + d_t2 d_t'2,   p = r_t r_t',   k = #{ e in 1 ... bins - 1 : q <= ct[e] p },   H[a][b][c][k] += 1
// with ct[e] = cos(e pi / bins) the caller's doubles: no acos, no division, q and p symmetric in t <-> t' bit for bit.  And for
// every species b, n_ib the number of neighbours of species b:  C[a][b][min(n_ib, ADF_MAXCOORD - 1)] += 1.
//   The neighbours are read from THIS step's list (d_nn, d_nbr_j, d_nbr_shift: the forward pass has written it for the positions
// of configuration n, every image within rc, code = image triple | species slot << 24; the step's last kernel, which bins the
// next configuration, writes none of the three) — no O(N^2) sweep: the cost is linear in N.  The list's own rule (|r| < rc on a
// contracted squared distance) and r < cut can differ only for a cutoff EQUAL to rc and a distance within an ulp of it.
//   Two launches behind a sampled evaluation:
//   * md_adf_kernel, one workgroup of up to four waves per CHUNK — ADF_CHUNK consecutive sorted centres of one species (the host
//     lists the chunks at the attach; the centre species is uniform over a workgroup), one wave per centre at a time.  The wave
//     reads min(nn[i], maxnn) list entries, 64 at a time, forms d and r, selects by the cutoff row of a (in LDS) and compacts the
//     selected (d, r, b) into its LDS rows by ballot; lane b counts n_ib from the ballots.  The lanes then split the T (T - 1) / 2
//     pairs (a flat index, decoded with a float square root and corrected in integers) and find the bin by bisection over
//     ct[e] p with the edge table in LDS: the product is monotone in e (sgpr_md_adf checks that ct does not increase), so the
//     bisection's count is the linear one.  <true>: the counts go to 32-bit LDS counters [pair (b, c)][bins] and at the end the
//     non-zero ones to the 64-bit table with integer atomics; <false> (pairs x bins beyond ADF_LDS_COUNTERS): straight to the
//     table with 64-bit atomics.  The coordination counters [S][ADF_MAXCOORD] are in LDS in both forms.
//     Dynamic LDS: ct | counters | cutoff row | per wave the rows for maxnn neighbours — the list's CAPACITY at launch time, so no
//     neighbour is ever dropped; the host takes fewer waves when four do not fit 64 KB.
//   * md_adf_done_kernel: samples += 1, next_due = n + every.
// Both leave at once when the run has halted before this evaluation and when n != next_due: a configuration evaluated twice counts
// once.  And when this evaluation overflowed a capacity (the step's last kernel has just written the overflow word of its scalar
// row): its list was clamped, the run halts with code 2, and the repeat of the configuration — with the list grown — is the one
// that counts.  No float atomics, no contraction, no scratch.
#pragma once

#define ADF_CHUNK 16            // centres per workgroup: 4096 atoms give 256 workgroups or more, one per CU
#define ADF_MAXCOORD 64         // coordination numbers 0 ... 62, and 63 and above
#define ADF_MAXBINS 1024
#define ADF_LDS_COUNTERS 4096   // 32-bit LDS counters of a workgroup at most (16 KB); beyond: global atomics
#define ADF_LDS_BYTES 65536
#define ADF_ROW_BYTES 36        // per neighbour of a wave: d[3], r (doubles) and the species slot

// bytes of dynamic LDS in front of the waves' rows
static inline size_t adf_lds_fixed(int S, int bins, bool lds_counters)
{
    return sizeof(double) * (size_t)bins + sizeof(unsigned) * (lds_counters ? (size_t)(S * (S + 1) / 2) * bins : 0) +
           sizeof(unsigned) * (size_t)S * ADF_MAXCOORD + sizeof(double) * (size_t)S;
}

__device__ __forceinline__ void adf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct AdfArgs {
    const int *chunk;           // [nch][3] first centre | centres | species slot a
    const double *x, *cell;     // the ring slot of configuration n, sorted order [N][3]; the constant cell [9]
    const int *nn, *nbr_j, *nbr_code;   // this step's list
    const double *cut, *ct;     // [S][S], [bins]
    unsigned long long *angles, *coord;   // [S][S][S][bins] (b <= c filled), [S][S][ADF_MAXCOORD]
    const long long *ctl;       // next_due | samples
    const int *halt;
    const double *ov;           // this evaluation's overflow word (its scalar row, entry 10): != 0, the list was clamped
    long long n;
    int maxnn, S, bins, step;
};

template <bool LDSC>
__global__ __launch_bounds__(256) void md_adf_kernel(const AdfArgs f)
{
    if (*f.halt < f.step) return;
    if (f.ctl[0] != f.n || *f.ov != 0.0) return;
    extern __shared__ double adf_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, nwave = nthr >> 6;
    const int S = f.S, bins = f.bins, maxnn = f.maxnn, npair = S * (S + 1) / 2;
    // the layout of adf_lds: doubles first
    double *ct = adf_lds;                                   // [bins]
    double *cutrow = ct + bins;                             // [S]
    double *rows = cutrow + S;                              // [nwave][maxnn][4]
    unsigned *cnt = (unsigned *)(rows + (size_t)nwave * maxnn * 4);   // [npair][bins] (LDSC)
    unsigned *ccnt = cnt + (LDSC ? npair * bins : 0);       // [S][ADF_MAXCOORD]
    int *rowb = (int *)(ccnt + S * ADF_MAXCOORD);           // [nwave][maxnn]
    const int *ch = f.chunk + 3 * (size_t)blockIdx.x;
    const int i0 = ch[0], ni = ch[1], a = ch[2];
    for (int k = tid; k < bins; k += nthr) ct[k] = f.ct[k];
    for (int k = tid; k < S; k += nthr) cutrow[k] = f.cut[a * S + k];
    if (LDSC)
        for (int k = tid; k < npair * bins; k += nthr) cnt[k] = 0u;
    for (int k = tid; k < S * ADF_MAXCOORD; k += nthr) ccnt[k] = 0u;
    __syncthreads();
    double *rw = rows + (size_t)wave * maxnn * 4;
    int *rb = rowb + (size_t)wave * maxnn;
    const double *h = f.cell;
    unsigned long long *Ha = f.angles + (size_t)a * S * S * bins;
    for (int ci = wave; ci < ni; ci += nwave) {
        const int i = i0 + ci;
        const int nn = min(f.nn[i], maxnn);
        const double xi0 = f.x[3 * (size_t)i], xi1 = f.x[3 * (size_t)i + 1], xi2 = f.x[3 * (size_t)i + 2];
        int T = 0, mine = 0;   // mine: n_ib of species b = lane
        for (int c0 = 0; c0 < nn; c0 += 64) {
            const int t = c0 + lane;
            bool hit = false;
            double d0 = 0.0, d1 = 0.0, d2 = 0.0, len = 1.0;
            int b = 0;
            if (t < nn) {
#pragma clang fp contract(off)
                const size_t e = (size_t)i * maxnn + t;
                const int code = f.nbr_code[e], j = f.nbr_j[e];
                b = (code >> 24) & 0xff;
                const double s0 = (double)(int)(int8_t)(code & 0xff), s1 = (double)(int)(int8_t)((code >> 8) & 0xff),
                             s2 = (double)(int)(int8_t)((code >> 16) & 0xff);
                d0 = (f.x[3 * (size_t)j] - xi0) + ((s0 * h[0] + s1 * h[3]) + s2 * h[6]);
                d1 = (f.x[3 * (size_t)j + 1] - xi1) + ((s0 * h[1] + s1 * h[4]) + s2 * h[7]);
                d2 = (f.x[3 * (size_t)j + 2] - xi2) + ((s0 * h[2] + s1 * h[5]) + s2 * h[8]);
                len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                hit = b < S && len < cutrow[b];
            }
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int pos = T + __popcll(m & ((1ull << lane) - 1ull));
                rw[4 * pos] = d0; rw[4 * pos + 1] = d1; rw[4 * pos + 2] = d2; rw[4 * pos + 3] = len;
                rb[pos] = b;
            }
            for (int s = 0; s < S; s++) {
                const int c = __popcll(__ballot(hit && b == s));
                if (lane == s) mine += c;
            }
            T += __popcll(m);
        }
        if (lane < S) atomicAdd(&ccnt[lane * ADF_MAXCOORD + min(mine, ADF_MAXCOORD - 1)], 1u);
        adf_wave_sync();   // (the rows of the wave are in LDS)
        const int P = T * (T - 1) / 2;
        for (int pi = lane; pi < P; pi += 64) {
#pragma clang fp contract(off)
            // pair pi = hi (hi - 1) / 2 + lo, lo < hi
            int hi = (int)((1.0f + sqrtf(8.0f * (float)pi + 1.0f)) * 0.5f);
            while (hi * (hi - 1) / 2 > pi) hi--;
            while ((hi + 1) * hi / 2 <= pi) hi++;
            const int lo = pi - hi * (hi - 1) / 2;
            const double q = (rw[4 * lo] * rw[4 * hi] + rw[4 * lo + 1] * rw[4 * hi + 1]) + rw[4 * lo + 2] * rw[4 * hi + 2];
            const double p = rw[4 * lo + 3] * rw[4 * hi + 3];
            int kl = 0, kh = bins - 1;
            while (kl < kh) {
                const int mid = (kl + kh + 1) >> 1;
                if (q <= ct[mid] * p) kl = mid; else kh = mid - 1;
            }
            const int bl = rb[lo], bh = rb[hi], b = min(bl, bh), c = max(bl, bh);
            if (LDSC)
                atomicAdd(&cnt[(b * S - b * (b - 1) / 2 + (c - b)) * bins + kl], 1u);
            else
                atomicAdd(&Ha[((size_t)b * S + c) * bins + kl], 1ull);
        }
        adf_wave_sync();   // (the rows are written again for the wave's next centre)
    }
    __syncthreads();
    if (LDSC)
        for (int b = 0, pr = 0; b < S; b++)
            for (int c = b; c < S; c++, pr++)
                for (int k = tid; k < bins; k += nthr) {
                    const unsigned v = cnt[pr * bins + k];
                    if (v) atomicAdd(&Ha[((size_t)b * S + c) * bins + k], (unsigned long long)v);
                }
    unsigned long long *Ca = f.coord + (size_t)a * S * ADF_MAXCOORD;
    for (int k = tid; k < S * ADF_MAXCOORD; k += nthr) {
        const unsigned v = ccnt[k];
        if (v) atomicAdd(&Ca[k], (unsigned long long)v);
    }
}

// ctl: next_due | samples.  ov: as AdfArgs.
__global__ __launch_bounds__(64) void md_adf_done_kernel(long long *ctl, long long n, int every, const int *halt, int step, const double *ov)
{
    if (*halt < step) return;
    if (ctl[0] != n || *ov != 0.0) return;
    if (threadIdx.x == 0) { ctl[1] = ctl[1] + 1; ctl[0] = n + every; }
}
