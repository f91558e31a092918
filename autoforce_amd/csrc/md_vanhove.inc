// md_vanhove.inc — van Hove correlation functions accumulated inside the device MD loop (sgpr_md_vanhove).  The self part is what
// the reference takes from a stored trajectory at one lag (theforce/analysis/analysis.py:178-210 `hist_rtp_displacements`: a
// histogram of the displacements over (r, theta, phi)); the reference has no distinct part.  Both are tables of integers in HBM
// that the run fills behind the evaluations it samples.  workloads.VanHoveCounts is the host twin and the definition.
//   Samples and levels are md_msd.inc's: sample s is configuration n = s every, level l < L has the lag 2^l samples and ONE
// origin O_l [N][3] (sorted order, never wrapped); at sample s every level with s mod 2^l == 0 is DUE, measures if s > 0
// (count[l] += 1) and then O_l <- x.
//   Self: atom i of species slot z, d = x_i - O_l,i, q = d0 d0 + d1 d1, r = sqrt(q + d2 d2) (the reference's cart_coord_to_sph).
// r >= rmax: over[l][z] += 1.  Else Hs[l][z][kr][kt][kp] += 1 with kr = min((int)((r / rmax) rbins), rbins - 1), kt the number
// of k in 1 ... tbins - 1 with d2 <= ct[k] r, kp the number of k in 1 ... pbins - 1 whose edge f_k = -pi + 2 pi k / pbins the
// azimuth has passed — by the sign of d1 and of cu[k] d1 - su[k] d0, see vh_self_bin —; r == 0 (a held atom) is bin
// (0, 0, pbins / 2), where atan2(0, 0) = 0 lands.  ct, cu, su are tables of doubles the host uploads: the twin compares with the
// same ones, and no acos or atan2 decides a bin on either side.
//   Distinct (dbins > 0): Hd[l][a][b][k] gains the triples (i of a, j of b, s in Z^3), (j, s) != (i, 0), with
// d = (x_j - O_l,i) + ((s0 h0 + s1 h1) + s2 h2), 0 <= r < dmax, k by rdf_count with rmin = 0: md_rdf.inc's enumeration, the pair
// taken to its nearest image by n = rint(dx inv) and s = t - n over the block |t_k| <= R_k.  For j == i the image left out is
// s == 0, that is t == n: an atom that has moved more than half a cell has n != 0.  Origin and present are not interchangeable:
// all ORDERED tile pairs are swept, the full S x S is stored.
//   At most three launches behind a sampled evaluation, in this order:
//   * md_vh_pair_kernel<IMG> (dbins > 0, s > 0), grid (tile pairs, parts of tile J, due levels): md_rdf_pair_kernel's sweep with
//     row i from O_l and tile J from the ring slot of n in LDS; LDS 32-bit counters, then 64-bit integer atomics into Hd.  It
//     reads the origins the next launch overwrites.
//   * md_vh_self_kernel, one workgroup of 256 per chunk of MSD_CHUNK sorted atoms of one species, one atom per thread: x once,
//     per due level O_l, the bin rule, one integer atomic on Hs or over, O_l <- x.  The edge tables sit in LDS.
//   * md_vh_done_kernel: count[l] += 1 for the due levels (s > 0), samples += 1, next_due = n + every.
// All leave at once when the run has halted before this evaluation and when n != next_due: a configuration evaluated twice — the
// repeat behind a covloss halt or an overflow — counts once.  No float atomics, no contraction, true divisions and square roots.
#pragma once

#define VH_MAXRBINS 2048   // radial bins of the self part
#define VH_MAXABINS 64     // polar and azimuthal bins: the edge tables of md_vh_self_kernel in LDS
#define VH_CHUNK 3         // ints per chunk: first atom | atoms | species slot
#define VH_CTL 2           // ctl: next_due | samples | count[L]

// The level that workgroup z of the due ones serves.
__device__ __forceinline__ int vh_due_level(unsigned due, int z)
{
    int l = 0;
    for (;; l++)
        if (((due >> l) & 1u) && z-- == 0) break;
    return l;
}

// pair: [npairs][RDF_PAIR] all ordered tile pairs (weight 1); grid (npairs, parts of tile J, due levels).  origin: [L][N][3]
// (lstride = 3N), x: the ring slot of configuration n.  table: [L][S][S][bins] (tstride = S S bins).  ctl[0]: next_due.
template <bool IMG>
__global__ __launch_bounds__(256) void md_vh_pair_kernel(const int *__restrict__ pair, const double *__restrict__ origin, size_t lstride,
                                                         const double *__restrict__ x, const RdfGeom g, unsigned due,
                                                         unsigned long long *__restrict__ table, size_t tstride, const long long *ctl, long long n,
                                                         const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double xj[RDF_TILE * 3];
    __shared__ unsigned cnt[RDF_MAXBINS];
    const int tid = threadIdx.x;
    const int l = vh_due_level(due, (int)blockIdx.z);
    const int *p = pair + RDF_PAIR * (size_t)blockIdx.x;
    const int i0 = p[0], ni = p[1], j0 = p[2], nj = p[3], slot = p[4];
    const int bins = g.bins;
    const int jpart = (nj + (int)gridDim.y - 1) / (int)gridDim.y, jlo = min(nj, (int)blockIdx.y * jpart), jhi = min(nj, jlo + jpart);
    for (int k = tid; k < bins; k += 256) cnt[k] = 0u;
    for (int e = 3 * jlo + tid; e < 3 * jhi; e += 256) xj[e] = x[3 * (size_t)j0 + e];
    __syncthreads();
    const int li = tid & (RDF_TILE - 1), half = tid >> 7;
    if (li < ni) {
#pragma clang fp contract(off)
        const bool diag = i0 == j0;
        const double *o = origin + lstride * l + 3 * ((size_t)i0 + li);
        const double xi0 = o[0], xi1 = o[1], xi2 = o[2];
        const double width = g.rmax - g.rmin, fbins = (double)bins, cut2 = (g.rmax * g.rmax) * (1.0 + 0x1p-30);
        for (int jj = jlo + half; jj < jhi; jj += 2) {
            const bool self = diag && jj == li;
            const double dx0 = xj[3 * jj] - xi0, dx1 = xj[3 * jj + 1] - xi1, dx2 = xj[3 * jj + 2] - xi2;
            const double n0 = g.pbc[0] ? rint((dx0 * g.inv[0] + dx1 * g.inv[3]) + dx2 * g.inv[6]) : 0.0;
            const double n1 = g.pbc[1] ? rint((dx0 * g.inv[1] + dx1 * g.inv[4]) + dx2 * g.inv[7]) : 0.0;
            const double n2 = g.pbc[2] ? rint((dx0 * g.inv[2] + dx1 * g.inv[5]) + dx2 * g.inv[8]) : 0.0;
            if (!IMG) {
                const double s0 = 0.0 - n0, s1 = 0.0 - n1, s2 = 0.0 - n2;
                if (self && s0 == 0.0 && s1 == 0.0 && s2 == 0.0) continue;
                rdf_count(dx0 + ((s0 * g.h[0] + s1 * g.h[3]) + s2 * g.h[6]), dx1 + ((s0 * g.h[1] + s1 * g.h[4]) + s2 * g.h[7]),
                          dx2 + ((s0 * g.h[2] + s1 * g.h[5]) + s2 * g.h[8]), g.rmin, g.rmax, width, fbins, cut2, bins, cnt);
            } else {
                for (int t0 = -g.R[0]; t0 <= g.R[0]; t0++)
                    for (int t1 = -g.R[1]; t1 <= g.R[1]; t1++)
                        for (int t2 = -g.R[2]; t2 <= g.R[2]; t2++) {
                            const double s0 = (double)t0 - n0, s1 = (double)t1 - n1, s2 = (double)t2 - n2;
                            if (self && s0 == 0.0 && s1 == 0.0 && s2 == 0.0) continue;
                            rdf_count(dx0 + ((s0 * g.h[0] + s1 * g.h[3]) + s2 * g.h[6]), dx1 + ((s0 * g.h[1] + s1 * g.h[4]) + s2 * g.h[7]),
                                      dx2 + ((s0 * g.h[2] + s1 * g.h[5]) + s2 * g.h[8]), g.rmin, g.rmax, width, fbins, cut2, bins, cnt);
                        }
            }
        }
    }
    __syncthreads();
    unsigned long long *row = table + tstride * l + (size_t)slot * bins;
    for (int k = tid; k < bins; k += 256) {
        const unsigned c = cnt[k];
        if (c) atomicAdd(&row[k], (unsigned long long)c);
    }
}

// The bin rule of the self part: the flat bin (kr tbins + kt) pbins + kp of a displacement, -1 beyond rmax.
__device__ __forceinline__ int vh_self_bin(double d0, double d1, double d2, double rmax, int rbins, int tbins, int pbins, const double *ct,
                                           const double *cu, const double *su)
{
#pragma clang fp contract(off)
    const double q = d0 * d0 + d1 * d1;
    const double r = sqrt(q + d2 * d2);
    if (r >= rmax) return -1;
    if (r == 0.0) return pbins / 2;
    int kr = (int)((r / rmax) * (double)rbins);
    kr = kr < rbins ? kr : rbins - 1;
    int kt = 0, kp = 0;
    for (int k = 1; k < tbins; k++) kt += d2 <= ct[k] * r ? 1 : 0;
    const bool up = d1 >= 0.0;
    for (int k = 1; k < pbins; k++) {
        const bool cross = cu[k] * d1 - su[k] * d0 >= 0.0;
        const bool pass = 2 * k < pbins ? (up || cross) : 2 * k == pbins ? up : (up && cross);
        kp += pass ? 1 : 0;
    }
    return (kr * tbins + kt) * pbins + kp;
}

// chunk: [nch][VH_CHUNK].  origin: [L][N][3] (lstride = 3N).  edges: ct [tbins] | cu [pbins] | su [pbins].  hs: [L][S][rbins tbins
// pbins] (zstride = rbins tbins pbins), over: [L][S].  due: the levels of this sample; acc: it measures (s > 0).  ctl[0]: next_due.
__global__ __launch_bounds__(256) void md_vh_self_kernel(const int *__restrict__ chunk, const double *__restrict__ x, double *__restrict__ origin,
                                                         size_t lstride, const double *__restrict__ edges, double rmax, int rbins, int tbins, int pbins,
                                                         int S, unsigned due, int acc, unsigned long long *__restrict__ hs, size_t zstride,
                                                         unsigned long long *__restrict__ over, const long long *ctl, long long n, const int *halt,
                                                         int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    __shared__ double ct[VH_MAXABINS], cu[VH_MAXABINS], su[VH_MAXABINS];
    const int tid = threadIdx.x;
    const int *c = chunk + VH_CHUNK * (size_t)blockIdx.x;
    const int len = c[1], z = c[2];
    if (acc) {
        if (tid < tbins) ct[tid] = edges[tid];
        if (tid >= 64 && tid < 64 + pbins) cu[tid - 64] = edges[tbins + tid - 64];
        if (tid >= 128 && tid < 128 + pbins) su[tid - 128] = edges[tbins + pbins + tid - 128];
        __syncthreads();
    }
    if (tid >= len) return;
    const size_t i3 = 3 * ((size_t)c[0] + tid);
    const double x0 = x[i3], x1 = x[i3 + 1], x2 = x[i3 + 2];
    for (int l = 0; l < MSD_MAXL; l++) {
        if (!((due >> l) & 1u)) continue;
        double *o = origin + lstride * l + i3;
        if (acc) {
#pragma clang fp contract(off)
            const int b = vh_self_bin(x0 - o[0], x1 - o[1], x2 - o[2], rmax, rbins, tbins, pbins, ct, cu, su);
            const size_t lz = (size_t)l * S + z;
            atomicAdd(b < 0 ? &over[lz] : &hs[lz * zstride + b], 1ull);
        }
        o[0] = x0; o[1] = x1; o[2] = x2;
    }
}

// ctl: next_due | samples | count[L].
__global__ __launch_bounds__(64) void md_vh_done_kernel(long long *ctl, long long n, int every, unsigned due, int acc, const int *halt, int step)
{
    if (*halt < step) return;
    if (ctl[0] != n) return;
    const int tid = threadIdx.x;
    if (acc && tid < MSD_MAXL && ((due >> tid) & 1u)) ctl[VH_CTL + tid] += 1;
    if (tid == 0) { ctl[1] = ctl[1] + 1; ctl[0] = n + every; }
}
