// The bin grid of a cell (NlGrid, sgpr_internal.h), made on the device: by the binning kernel (neighbor.hip) for the cell
// of its step, and by md_npt_kernel (md_npt.inc) for the cell a moving-cell MD step will bin its atoms in — one
// definition, so that both make the same grid of the same cell.  And the rule that places an atom in that grid
// (nl_place_axis, nl_bin_index) with the record a bin keeps of it (nl_store_rec): one definition for the binning kernel and
// for every last kernel that bins the next step's atoms itself (finalize_next_kernel, finalize_scatter_next_kernel,
// shard_next_kernel).
#pragma once

__device__ __forceinline__ double det3d(const double *h)
{
    return h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
}

__device__ inline void nl_make_grid(const double *cell, const int *pbc, double rc, NlGrid &g, int *stat)
{
    double h[9];
    for (int k = 0; k < 9; k++) h[k] = cell[k];
    // Slabs and wires may come with a zero vector along an open direction (cell = [a, b, 0], pbc = TTF is
    // valid in ASE): complete such vectors orthogonally to the others before inverting (ase.geometry
    // complete_cell, which ASE's neighbour list applies), so the periodic directions keep their images.
    // A zero vector along a PERIODIC direction is an input error (stat[3] = 2).
    {
        int zero[3], nz = 0;
        for (int k = 0; k < 3; k++) {
            zero[k] = h[3 * k] * h[3 * k] + h[3 * k + 1] * h[3 * k + 1] + h[3 * k + 2] * h[3 * k + 2] < 1e-24;
            nz += zero[k];
            if (zero[k] && pbc[k] && stat) atomicMax(&stat[3], 2);
        }
        if (nz > 0 && nz < 3) {
            for (int k = 0; k < 3; k++) {
                if (!zero[k] || pbc[k]) continue;
                const double *p = h + 3 * ((k + 1) % 3), *q = h + 3 * ((k + 2) % 3);
                double v[3];
                if (!zero[(k + 1) % 3] && !zero[(k + 2) % 3]) {
                    v[0] = p[1] * q[2] - p[2] * q[1]; v[1] = p[2] * q[0] - p[0] * q[2]; v[2] = p[0] * q[1] - p[1] * q[0];
                } else {
                    // one vector only: any direction perpendicular to it (the other open axis follows next)
                    const double *w = zero[(k + 1) % 3] ? q : p;
                    const int a = fabs(w[0]) <= fabs(w[1]) && fabs(w[0]) <= fabs(w[2]) ? 0 : (fabs(w[1]) <= fabs(w[2]) ? 1 : 2);
                    double e[3] = {0.0, 0.0, 0.0};
                    e[a] = 1.0;
                    v[0] = w[1] * e[2] - w[2] * e[1]; v[1] = w[2] * e[0] - w[0] * e[2]; v[2] = w[0] * e[1] - w[1] * e[0];
                }
                const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                if (nv > 1e-12) {
                    h[3 * k] = v[0] / nv; h[3 * k + 1] = v[1] / nv; h[3 * k + 2] = v[2] / nv;
                    zero[k] = 0;
                }
            }
        }
    }
    const double dt = det3d(h);
    if (fabs(dt) > 1e-12) {
        const double *p = h, *q = h + 3, *r = h + 6;
        const double bc[3] = {q[1] * r[2] - q[2] * r[1], q[2] * r[0] - q[0] * r[2], q[0] * r[1] - q[1] * r[0]};
        const double ca[3] = {r[1] * p[2] - r[2] * p[1], r[2] * p[0] - r[0] * p[2], r[0] * p[1] - r[1] * p[0]};
        const double ab[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
        for (int k = 0; k < 3; k++) {
            g.inv[3 * k + 0] = bc[k] / dt;
            g.inv[3 * k + 1] = ca[k] / dt;
            g.inv[3 * k + 2] = ab[k] / dt;
        }
        const double V = fabs(dt);
        const double hgt[3] = {V / sqrt(bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]),
                               V / sqrt(ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2]),
                               V / sqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2])};
        for (int k = 0; k < 3; k++) {
            if (pbc[k]) {
                int nb = (int)floor(hgt[k] / rc);
                nb = nb < 1 ? 1 : (nb > 16 ? 16 : nb);
                g.nb[k] = nb;
                g.rng[k] = (int)ceil(rc * nb / hgt[k]);
            } else {
                g.nb[k] = 1;  // open direction: one slab, no images
                g.rng[k] = 0;
            }
            g.w[k] = hgt[k] / g.nb[k];
        }
        // plane normals bc, ca, ab: orthogonal cells let the sweep bound the distance to a bin by the
        // Euclidean norm of the three plane gaps (otherwise only by the largest gap)
        const double d01 = bc[0] * ca[0] + bc[1] * ca[1] + bc[2] * ca[2], d02 = bc[0] * ab[0] + bc[1] * ab[1] + bc[2] * ab[2],
                     d12 = ca[0] * ab[0] + ca[1] * ab[1] + ca[2] * ab[2];
        const double n0 = bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2], n1 = ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2],
                     n2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
        g.ortho = (d01 * d01 < 1e-20 * n0 * n1 && d02 * d02 < 1e-20 * n0 * n2 && d12 * d12 < 1e-20 * n1 * n2) ? 1 : 0;
    } else {
        // no usable cell (cluster): everything in one bin, no images
        for (int k = 0; k < 9; k++) g.inv[k] = 0.0;
        for (int k = 0; k < 3; k++) { g.nb[k] = 1; g.rng[k] = 0; g.w[k] = 0.0; }
        g.ortho = 0;
    }
    g.nbins = g.nb[0] * g.nb[1] * g.nb[2];
}

// Direction k of the rule that places position (X, Y, Z) in grid g: the index of its bin along k, and w: how many cells it
// was wrapped by (the floor of the fractional coordinate; 0 along an open direction or without a cell).
__device__ __forceinline__ int nl_place_axis(const NlGrid &g, int k, int periodic, double X, double Y, double Z, int &w)
{
    double fr = X * g.inv[k] + Y * g.inv[3 + k] + Z * g.inv[6 + k];
    w = 0;
    if (!(periodic && (g.inv[k] != 0.0 || g.inv[3 + k] != 0.0 || g.inv[6 + k] != 0.0))) return 0;
    const double fl = floor(fr);
    w = (int)fl;
    fr -= fl;
    const int b = (int)(fr * g.nb[k]);
    return b >= g.nb[k] ? g.nb[k] - 1 : (b < 0 ? 0 : b);
}

// The bin of the three indices.  A caller places an atom with
//     for (k = 0 .. 2) bidx[k] = nl_place_axis(g, k, pbc[k], X, Y, Z, w[k]);   bin = nl_bin_index(g, bidx);
// The loop over the directions stays in the kernel on purpose: `pbc` lives in the kernel's argument record, and indexing that
// record by the loop counter is what keeps the compiler from reading the whole record ahead of the kernel's first instruction
// (with the loop inside a function here: 16 to 50 more SGPRs in three of the four kernels, one to four more VGPRs in two).
__device__ __forceinline__ int nl_bin_index(const NlGrid &g, const int (&bidx)[3])
{
    return (bidx[0] * g.nb[1] + bidx[1]) * g.nb[2] + bidx[2];
}

// What bin `bin` keeps of the atom (sorted index idx, species slot `slot`) that nl_place_axis / nl_bin_index put there and whose returning atomic
// on the bin's population handed out slot k — the atomic itself stays with the caller, who knows where its round trip hides.
// stat[3]: a wrap beyond int16; stat[1]: the population of a bin beyond its capacity (rare: the host grows it and reruns).
__device__ __forceinline__ void nl_store_rec(BinRec *b_rec, BinAux *b_aux, int cap, int *stat, int bin, int k, double X, double Y, double Z,
                                             int idx, const int (&w)[3], int slot)
{
    if (max(max(abs(w[0]), abs(w[1])), abs(w[2])) > 32767) atomicMax(&stat[3], 1);  // atoms > 32767 cells away
    if (k < cap) {
        const size_t e = (size_t)bin * cap + k;
        BinRec r;
        r.x = X; r.y = Y; r.z = Z; r.idx = idx; r.pad = 0;
        b_rec[e] = r;
        BinAux ax;
        ax.w0 = (short)w[0]; ax.w1 = (short)w[1]; ax.w2 = (short)w[2]; ax.slot = (short)slot;
        b_aux[e] = ax;
    } else
        atomicMax(&stat[1], k + 1);
}
