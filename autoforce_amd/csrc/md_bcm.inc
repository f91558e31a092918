// md_bcm.inc — the Bayesian committee inside the device MD loop (sgpr_md_committee): K frozen members and the live model are
// evaluated at the same positions and combined with the reference's weights (calculator/active_bcm.py:589-633, restated in
// autoforce_amd/calculator_bcm.py::update_results), members k = 0 ... K - 1 in the order they were attached, the live model
// last (k = K):
//     covmax_k = max_i beta_k(i),   b_k = -ln(covmax_k) if covmax_k < 1 else 0,   s_k = b_k / covmax_k  (covmax_k = 0: +inf)
//     any s_k infinite:  w_k = 1 where it is, 0 elsewhere;      sum_k s_k <= 0:  w = e_K (the live model answers alone)
//     w <- w / sum_k w_k,    E = sum_k w_k E_k  (member order; every force component and the nine virial entries alike)
//     beta_tot(i) = min_k beta_k(i)  (get_covloss_total, :885-894);  the covloss that gates the run is max_i beta_tot(i)
// The weights need the largest covloss of EVERY member at THIS configuration before a single force can be combined, so — as
// in a relaxation (md_relax.inc) — the integrator cannot sit in an evaluation's last kernel.  Behind the K + 1 plain steps of
// an evaluation (each member's own binning kernel and plain last kernel, results in K + 1 packed scratch buffers):
//   * md_bcm_kernel, ONE workgroup: the K + 1 maxima and max_i beta_tot (thread t takes the atoms t, t + 256, ...), the weights,
//     the overflow word as the maximum over the members, the halts — covloss gate and capacity overflow, decided on the
//     evaluation itself with nothing moved yet: no speculative evaluation, no lag —, the combined E and virial, the
//     evaluation's row of scalars and its mark;
//   * md_bcm_move_kernel, a quad of lanes per atom: the combined force and beta_tot into the run's packed ring slot (caller
//     order: what sgpr_md_state returns), then the integrator with the combined force — the functions
//     finalize_next_kernel<2> calls: md_baoab_advance (BAOAB Langevin with uploaded or counter-based deviates, velocity
//     Verlet) or md_nh_advance (Nose-Hoover), the kinetic terms through fin_store_ke — writing the next ring slot (sorted
//     order) and the caller-order copy the members read;
//   * md_bcm_ke_kernel, ONE workgroup: the two kinetic sums of the evaluation in md_nh_kernel's fixed order (no lag: the row
//     of an evaluation is complete behind its own launches); under Nose-Hoover md_nh_kernel follows as in the fused loop.
// With a barostat (sgpr_md_barostat; md_npt.inc has the scheme) the K + 1 plain steps run in the cell h_n of the evaluation,
// md_bcm_move_kernel<true> moves the atoms in scaled coordinates — md_npt_advance, the function finalize_next_kernel<3> calls; no
// binning here: every handle bins through its own binning kernel in the next evaluation — and md_npt_kernel takes md_nh_kernel's
// place, reading the combined virial md_bcm_kernel wrote into the run's ring slot: the barostat integrates the committee's stress.
// No float atomics, no contraction in the combination: two runs give the same bits.
#pragma once

#define BCM_MAX 16      // members of a committee, the live model included
#define BCM_INFO 32     // doubles per evaluation of the committee record: w[BCM_MAX] | covmax[BCM_MAX]

// Behind the K1 = K + 1 plain steps of an evaluation.  P: their packed results, `plen` doubles apart (caller atom order, the
// live model last); packed: the run's ring slot, whose eleven scalars are written here; info: this evaluation's committee record.
__global__ __launch_bounds__(256) void md_bcm_kernel(int N, int K1, size_t plen, const double *P, double *packed, double *info, double ediff,
                                                     int *halt, int *halt_host, int step, double *scal_row, int *mark)
{
#pragma clang fp contract(off)
    if (*halt < step) return;
    __shared__ double wmax[BCM_MAX + 1][4];
    __shared__ double sw[BCM_MAX];
    const int tid = threadIdx.x;
    double cm[BCM_MAX], bt = 0.0;
#pragma unroll
    for (int k = 0; k < BCM_MAX; k++) cm[k] = 0.0;
    for (int i = tid; i < N; i += 256) {
        double mn = 1e300;
#pragma unroll
        for (int k = 0; k < BCM_MAX; k++)
            if (k < K1) {
                const double b = P[(size_t)k * plen + 3 * (size_t)N + i];
                cm[k] = fmax(cm[k], b);
                mn = fmin(mn, b);
            }
        bt = fmax(bt, mn);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < BCM_MAX; k++) cm[k] = fmax(cm[k], __shfl_xor(cm[k], o, 64));
        bt = fmax(bt, __shfl_xor(bt, o, 64));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < BCM_MAX; k++) wmax[k][tid >> 6] = cm[k];
        wmax[BCM_MAX][tid >> 6] = bt;
    }
    __syncthreads();
    if (tid == 0) {
        double *s = sw, tot = 0.0;   // (the scales, then in place the weights)
        bool any_inf = false;
        for (int k = 0; k < K1; k++) {
            const double c = fmax(fmax(wmax[k][0], wmax[k][1]), fmax(wmax[k][2], wmax[k][3]));
            const double b = c < 1.0 ? -log(c) : 0.0;
            s[k] = c > 0.0 ? __ddiv_rn(b, c) : INFINITY;
            any_inf |= isinf(s[k]);
            info[BCM_MAX + k] = c;
        }
        if (any_inf)   // a member with zero covloss everywhere is certain: it alone decides
            for (int k = 0; k < K1; k++) s[k] = isinf(s[k]) ? 1.0 : 0.0;
        for (int k = 0; k < K1; k++) tot = tot + s[k];
        if (!(tot > 0.0)) {   // every member is out of its depth: the live model answers
            for (int k = 0; k < K1; k++) s[k] = 0.0;
            s[K1 - 1] = 1.0;
            tot = 1.0;
        }
        for (int k = 0; k < K1; k++) {
            const double w = __ddiv_rn(s[k], tot);
            s[k] = w;
            info[k] = w;
        }
    }
    __syncthreads();
    if (tid < 10) {   // E and the nine virial entries, accumulated in member order
        double acc = 0.0;
        for (int k = 0; k < K1; k++) acc = acc + sw[k] * P[(size_t)k * plen + 4 * (size_t)N + tid];
        scal_row[tid] = acc;
        packed[4 * (size_t)N + tid] = acc;
    } else if (tid == 10) {
        double ov = 0.0;
        for (int k = 0; k < K1; k++) ov = fmax(ov, P[(size_t)k * plen + 4 * (size_t)N + 10]);
        const double bmax = fmax(fmax(wmax[BCM_MAX][0], wmax[BCM_MAX][1]), fmax(wmax[BCM_MAX][2], wmax[BCM_MAX][3]));
        scal_row[10] = ov;
        scal_row[11] = bmax;
        packed[4 * (size_t)N + 10] = ov;
        // the halts, with nothing moved yet (halt_host word: 0 the covloss gate, 1 a capacity overflow)
        const int why = ov != 0.0 ? 1 : (bmax >= ediff ? 0 : -1);
        if (why >= 0) {
            atomicMin(halt, step);
            halt_host[why] = step;
        }
        *mark = 1;
    }
}

// The combination per atom and the move out of the evaluation: lanes 0..2 of a quad take the three components of sorted atom
// i (caller atom c = perm[i]).  w: the weights md_bcm_kernel left in this evaluation's committee record.  x: the integrator's
// part of the FinNext record sgpr_md_run fills for the fused loop (the same fields with the same meaning).  A run that halted
// BEFORE this evaluation is left untouched; at the halting evaluation itself, and where `stay` is set (the last evaluation of
// a `final` call), the results are written and the kinetic terms of the evaluation with them — Nose-Hoover: its centred
// velocity too, which IS the evaluation's velocity — but no position or velocity of the next configuration.
//   CELL (its own instantiation: the constant-cell one stays the code it was): the moving cell.  q_n, q_(n-1) from the ring of
// scaled coordinates and column l3 of h_n^-1, B - 1, (B + 1)^-1, h_n, h_(n+1) from the ring of NptSlots (wave-uniform addresses),
// requested with everything else; the centred velocity v_n and the kinetic terms are written wherever the results are — md_state
// and md_npt_kernel read them at a halting evaluation too —, q_(n+1), x_(n+1) in the cell h_(n+1) and its caller-order copy only
// when the run moves on.
template <bool CELL>
__global__ __launch_bounds__(256) void md_bcm_move_kernel(int N, int K1, size_t plen, const double *P, const double *w, double *packed, double *x_caller,
                                                          const int *perm, FinNext x, int stay)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 3, l3 = lane < 3 ? lane : 2;
    const int i = blockIdx.x * 64 + (tid >> 2);
    const bool act = i < N;
    const int ia = act ? i : 0;
    // requests: one round trip (unconditional loads with clamped indices), then the one behind the permutation
    const int halt_w = *x.halt;
    const int c = perm[ia];
    const double xc = x.x_cur[3 * (size_t)ia + l3], vc = x.v_cur[3 * (size_t)ia + l3];
    const double ms = x.mass[ia], sg = x.sig[ia];
    const double nz = x.noise ? x.noise[3 * (size_t)ia + l3] : 0.0;   // (uniform condition)
    double xpv = 0.0, zeta = 0.0;
    if (!CELL && x.nh) { xpv = x.x_prev[3 * (size_t)ia + l3]; zeta = *x.nh_zeta; }   // (uniform condition)
    // CELL: q_n, q_(n-1), and column l3 of h_n^-1, B - 1, (B + 1)^-1, h_n of this evaluation's slot and of h_(n+1) (uniform addresses)
    double qc = 0.0, qp = 0.0, c_hinv[3], c_bm1[3], c_bp1[3], c_h[3], c_hn[3];
    if (CELL) {
        const NptSlot *nc = x.npt_cur, *nn = x.npt_next;
        qc = x.q_cur[3 * (size_t)ia + l3];
        qp = x.q_prev[3 * (size_t)ia + l3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            c_hinv[j] = nc->hinv[3 * j + l3]; c_bm1[j] = nc->bm1[3 * j + l3]; c_bp1[j] = nc->bp1inv[3 * j + l3];
            c_h[j] = nc->h[3 * j + l3]; c_hn[j] = nn->h[3 * j + l3];
        }
    }
    double F = 0.0, bmin = 1e300;
#pragma unroll
    for (int k = 0; k < BCM_MAX; k++)
        if (k < K1) {
            const double *pk = P + (size_t)k * plen;
            F = F + w[k] * pk[3 * (size_t)c + l3];
            bmin = fmin(bmin, pk[3 * (size_t)N + c]);
        }
    if (halt_w < x.step) return;
    const bool move = halt_w > x.step && !stay;
    if (act && lane < 3) packed[3 * (size_t)c + lane] = F;
    if (act && lane == 3) packed[3 * (size_t)N + c] = bmin;
    double ke, kp, xn;
    if (CELL) {
        // (every lane of the quad takes part in the row products; lane 3 holds lane 2's values and stores nothing)
        double qn;
        const double vnow = md_npt_advance(x, F, ms, qc, qp, vc, c_hinv, c_bm1, c_bp1, c_h, c_hn, qn, xn);
        ke = ms * (vnow * vnow);
        kp = ke;
        if (act && lane < 3) {
            x.v_now[3 * (size_t)i + lane] = vnow;
            if (move) {
                x.q_next[3 * (size_t)i + lane] = qn;
                x.x_next[3 * (size_t)i + lane] = xn;
            }
        }
    } else if (x.nh) {
        const double vnow = md_nh_advance(x, false, F, ms, xc, vc, xpv, zeta, xn);
        ke = ms * (vnow * vnow);
        kp = ke;
        if (act && lane < 3) {
            x.v_now[3 * (size_t)i + lane] = vnow;
            if (move) x.x_next[3 * (size_t)i + lane] = xn;
        }
    } else {
        double v3;
        xn = md_baoab_advance(x, false, F, ms, sg, nz, xc, vc, c, l3, v3, ke, kp);
        if (act && lane < 3 && move) {
            x.x_next[3 * (size_t)i + lane] = xn;
            x.v_next[3 * (size_t)i + lane] = v3;
        }
    }
    fin_store_ke(ke, kp, act && lane == 0, x.ke_cur, i);
    if (act && lane < 3 && move) x_caller[3 * (size_t)c + lane] = xn;
}

// sum m v^2 of an evaluation, after its closing half kick | before it (ke: [N][2], sorted order), into its row of scalars: the
// fixed order of md_nh_kernel — thread t adds the atoms t, t + 256, ..., then a pairwise tree
__global__ __launch_bounds__(256) void md_bcm_ke_kernel(int N, const double *ke, const int *halt, int step, double *scal_row)
{
    if (*halt < step) return;
    __shared__ double wsum[2][4];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int k = tid; k < N; k += 256) {
        const double2 v = *(const double2 *)(ke + 2 * (size_t)k);
        a += v.x;
        b += v.y;
    }
    a = fin_wave_sum(a);
    b = fin_wave_sum(b);
    if ((tid & 63) == 0) { wsum[0][tid >> 6] = a; wsum[1][tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) {
        scal_row[12] = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
        scal_row[13] = (wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3]);
    }
}
