// md_rdf.inc — radial distribution functions accumulated inside the device MD loop (sgpr_md_rdf): what the reference works out
// of a stored trajectory (theforce/analysis/rdf.py `rdf`: per species pair a histogram of the distances in every atom's
// neighbour list at cutoff rmax) is here a table of integers in HBM that the run fills behind the evaluations it samples.
//   For a sampled configuration, species slots a, b of the model's table and k < bins, H[a][b][k] gains the number of triples
// (i of a, j of b, s in Z^3) with (j, s) != (i, 0) — periodic self-images count, as in the reference's list — whose distance
//     d = (x_j - x_i) + ((s0 h0 + s1 h1) + s2 h2),   r = sqrt((d0 d0 + d1 d1) + d2 d2),   rmin <= r < rmax
// falls in bin k = (int)(((r - rmin) / (rmax - rmin)) bins) (torch.histc's rule; a quotient that rounds up to `bins` stays in the
// last bin, as there).  s is 0 along an open direction.  The positions of the ring are never wrapped, so a pair is first taken to
// its nearest image by rounding its fractional difference, n_k = rint((dx0 inv[k] + dx1 inv[3 + k]) + dx2 inv[6 + k]), and the
// images s = t - n with |t_k| <= R_k = floor(rmax / height_k + 1/2) are enumerated: every image that can come within rmax.  d is
// a function of (i, j, s) alone and the counts are integers: the table depends neither on how a pair was wrapped nor on any
// order of summation.  workloads.RdfCounts is the host twin and the definition.  H is symmetric in (a, b) bit for bit (i <-> j
// negates every intermediate exactly): only a <= b is stored, sgpr_md_rdf_read fills the table out.
//   Two launches behind a sampled evaluation:
//   * md_rdf_pair_kernel, one workgroup of 256 per TILE PAIR (I <= J): the sorted atoms of one species are cut into tiles of
//     RDF_TILE = 128 (the host lists the tile pairs at the attach; a species' last tile is ragged), so a workgroup serves one
//     species pair.  Tile J is staged in LDS; thread t keeps atom t & 127 of tile I in registers and takes the j of parity
//     t >> 7 — two threads share an i-atom's j-loop, j is uniform over a wave and the LDS reads are broadcasts.  A small frame
//     has too few tile pairs to fill the chip: the host cuts tile J into gridDim.y equal parts, one workgroup each (the counts
//     are integers: the table does not know).  The R = 0 form
//     (<false>) measures one image per pair, the other the whole block.  A squared distance beyond rmax^2 (1 + 2^-30) is
//     dropped before the square root (it cannot pass r < rmax); the rest goes through the definition and an LDS integer atomic
//     on one of `bins` 32-bit counters.  At the end the non-zero counters go to the 64-bit table with integer atomics, twice
//     for an off-diagonal tile pair of one species.  A diagonal tile pair sweeps all ordered i != j (and the self-images).
//   * md_rdf_done_kernel: samples += 1, next_due = n + every.
// Both leave at once when the run has halted before this evaluation (the halt word as md_record_kernel reads it) and when
// n != next_due: a configuration evaluated twice — the repeat behind a covloss halt or an overflow — counts once.  No float
// atomics, no contraction, true divisions and square roots.
#pragma once

#define RDF_TILE 128       // atoms per tile: two threads of md_rdf_pair_kernel per i-atom
#define RDF_MAXBINS 2048   // 32-bit LDS counters of a workgroup
#define RDF_MAXR 2         // image block |s_k| <= 2: at most 125 shifts
#define RDF_SPLIT_MAX 8    // parts a tile J is cut into at most (16 atoms each), while the tile pairs alone are fewer than
#define RDF_WORKGROUPS 2048   // this many workgroups (eight waves per SIMD of 256 CUs)
#define RDF_PAIR 6         // ints per tile pair: first i | atoms i | first j | atoms j | slot a S + b | weight 1 or 2

// One image of one pair: the definition from d on.
__device__ __forceinline__ void rdf_count(double d0, double d1, double d2, double rmin, double rmax, double width, double fbins, double cut2,
                                          int bins, unsigned *cnt)
{
#pragma clang fp contract(off)
    const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!(r2 < cut2)) return;
    const double r = sqrt(r2);
    if (r >= rmin && r < rmax) {
        int k = (int)(((r - rmin) / width) * fbins);
        k = k < bins ? k : bins - 1;
        atomicAdd(&cnt[k], 1u);
    }
}

// pair: [npairs][RDF_PAIR]; grid (npairs, parts of tile J).  x: the ring slot of configuration n, sorted order [N][3].  table: [S][S][bins].  ctl[0]: next_due.
template <bool IMG>
__global__ __launch_bounds__(256) void md_rdf_pair_kernel(const int *__restrict__ pair, const double *__restrict__ x, const RdfGeom g,
                                                          unsigned long long *__restrict__ table, const long long *ctl, long long n,
                                                          const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double xj[RDF_TILE * 3];
    __shared__ unsigned cnt[RDF_MAXBINS];
    const int tid = threadIdx.x;
    const int *p = pair + RDF_PAIR * (size_t)blockIdx.x;
    const int i0 = p[0], ni = p[1], j0 = p[2], nj = p[3], slot = p[4], wgt = p[5];
    const int bins = g.bins;
    // (the j of this workgroup: part blockIdx.y of gridDim.y equal parts of tile J, the last ones ragged or empty)
    const int jpart = (nj + (int)gridDim.y - 1) / (int)gridDim.y, jlo = min(nj, (int)blockIdx.y * jpart), jhi = min(nj, jlo + jpart);
    for (int k = tid; k < bins; k += 256) cnt[k] = 0u;
    for (int e = 3 * jlo + tid; e < 3 * jhi; e += 256) xj[e] = x[3 * (size_t)j0 + e];
    __syncthreads();
    const int li = tid & (RDF_TILE - 1), half = tid >> 7;
    if (li < ni) {
#pragma clang fp contract(off)
        const bool diag = i0 == j0;
        const size_t i3 = 3 * ((size_t)i0 + li);
        const double xi0 = x[i3], xi1 = x[i3 + 1], xi2 = x[i3 + 2];
        const double width = g.rmax - g.rmin, fbins = (double)bins, cut2 = (g.rmax * g.rmax) * (1.0 + 0x1p-30);
        for (int jj = jlo + half; jj < jhi; jj += 2) {
            const bool self = diag && jj == li;
            if (!IMG && self) continue;
            const double dx0 = xj[3 * jj] - xi0, dx1 = xj[3 * jj + 1] - xi1, dx2 = xj[3 * jj + 2] - xi2;
            const double n0 = g.pbc[0] ? rint((dx0 * g.inv[0] + dx1 * g.inv[3]) + dx2 * g.inv[6]) : 0.0;
            const double n1 = g.pbc[1] ? rint((dx0 * g.inv[1] + dx1 * g.inv[4]) + dx2 * g.inv[7]) : 0.0;
            const double n2 = g.pbc[2] ? rint((dx0 * g.inv[2] + dx1 * g.inv[5]) + dx2 * g.inv[8]) : 0.0;
            if (!IMG) {
                const double s0 = 0.0 - n0, s1 = 0.0 - n1, s2 = 0.0 - n2;
                rdf_count(dx0 + ((s0 * g.h[0] + s1 * g.h[3]) + s2 * g.h[6]), dx1 + ((s0 * g.h[1] + s1 * g.h[4]) + s2 * g.h[7]),
                          dx2 + ((s0 * g.h[2] + s1 * g.h[5]) + s2 * g.h[8]), g.rmin, g.rmax, width, fbins, cut2, bins, cnt);
            } else {
                for (int t0 = -g.R[0]; t0 <= g.R[0]; t0++)
                    for (int t1 = -g.R[1]; t1 <= g.R[1]; t1++)
                        for (int t2 = -g.R[2]; t2 <= g.R[2]; t2++) {
                            if (self && t0 == 0 && t1 == 0 && t2 == 0) continue;
                            const double s0 = (double)t0 - n0, s1 = (double)t1 - n1, s2 = (double)t2 - n2;
                            rdf_count(dx0 + ((s0 * g.h[0] + s1 * g.h[3]) + s2 * g.h[6]), dx1 + ((s0 * g.h[1] + s1 * g.h[4]) + s2 * g.h[7]),
                                      dx2 + ((s0 * g.h[2] + s1 * g.h[5]) + s2 * g.h[8]), g.rmin, g.rmax, width, fbins, cut2, bins, cnt);
                        }
            }
        }
    }
    __syncthreads();
    unsigned long long *row = table + (size_t)slot * bins;
    for (int k = tid; k < bins; k += 256) {
        const unsigned c = cnt[k];
        if (c) atomicAdd(&row[k], (unsigned long long)c * (unsigned long long)wgt);
    }
}

// ctl: next_due | samples.
__global__ __launch_bounds__(64) void md_rdf_done_kernel(long long *ctl, long long n, int every, const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    if (threadIdx.x == 0) { ctl[1] = ctl[1] + 1; ctl[0] = n + every; }
}
