// gemm_tile.inc — one tile of the fp64 MFMA GEMM family as a device function (see gemm.hip for the family, its
// epilogues and what was measured).  Included by gemm.hip (the GEMM launches) and by descriptor.hip (the reverse kernel
// runs the covloss tiles of a step in its own launch: MFMA-bound tiles beside VALU-bound waves, one launch less
// on the critical path).
// The three tile bodies differ in their main loops; around them they share row_sum16 / wave_sum64, the kernel value
// (kernel_pm1 + KERNEL_VALUE), the tile entry (TILE_ENTRY_OR_RETURN), the stamps (stamp_entry / stamp_record) and the metadata
// prefetch (fetch_row_meta / fetch_col_meta).  Every kernel's VGPR / SGPR / scratch / LDS figures (tools/kres.py) are those of
// the copies these replaced; the shapes that were not neutral: k and kp from functions — gemm_nt_kernel<EPI_FUSED, 1, 16>
// 24 B and gemm_nt_kernel8r64x3<EPI_KERNEL> 36 B of scratch per lane, gemm_nt_kernel8r64<EPI_KERNEL> 110 -> 118 VGPRs; the
// tile entry as a function — gemm_nt_kernel<EPI_ROWSQ, 1, 32> 120 -> 124; the prefetch helpers in gemm_tile_body8 —
// gemm_nt_kernel8<EPI_KERNEL> 70 -> 72 SGPRs, and with the four rows in one call 84 -> 86 VGPRs (in the other bodies that
// form kept the figures and reordered 600 lines of the fused kernel); stamp_record testing g.stamps itself —
// gemm_nt_kernel8r64<EPI_WCOV> 44 -> 48 SGPRs.
#pragma once
typedef double v4d __attribute__((ext_vector_type(4)));

#define BM 64
#define BN 64
#define KT 32
#define LDS_LD 17

struct GemmArgs {
    GemmParams p;
    GemmParams p2;   // EPI_WCOV: second problem of the group (tile table entries with bit 16 of .x set)
    GemmParams p3;   // EPI_FUSED: the K_nm product whose row panels the other two consume (entries with bit 17 set)
    int *panel_cnt;  // EPI_FUSED: [row tiles x 32: one counter per 128-byte line] K tiles finished per row panel, never reset (epoch * need is the target)
    int epoch;       //            launches so far, this one included
    int *fuse_err;   //            set when a consumer gave up waiting (the host then repeats the step unfused)
    int ieta;        // integer exponent or -1
    const int *row_slot, *col_slot;
    double *Epart;
    int row_tiles, rows_pad, col_tiles;
    long long *stamps;  // diagnostic only (SGPR_STAMPS=1): [block][8] s_memtime stamps
};

// the value a DPP control hands to this lane (row = 16 lanes): 0xB1 / 0x4E swap inside quads, 0x141 / 0x140 mirror
// half rows / rows — a sum over the 16 lanes of a row without LDS round trips (four ds_bpermute chains per row sum
// made the covloss epilogue 3.7k cycles long)
template <int CTRL>
__device__ __forceinline__ double row_dpp(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// 16 bytes of the A operand.  COHERENT (EPI_FUSED): the bytes were written by ANOTHER workgroup of the SAME launch — a
// K_nm tile — with device-scope write-through stores; they are read with device-scope loads (`sc1`: past the CU's L1,
// which nobody invalidates inside a launch, and coherent in L2), 8 bytes each (MI355X_MICROARCH.md, "Workgroup dispatch,
// XCD placement & inter-workgroup visibility").
template <bool COHERENT>
__device__ __forceinline__ double2 load_a2(const double *q)
{
    if constexpr (COHERENT) {
        double *w = const_cast<double *>(q);
        return make_double2(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    } else
        return *(const double2 *)q;
}

// the sum over the 16 lanes of a row, in every lane of it: the same pairs, in the same order, as xor 1, 2, 4, 8
__device__ __forceinline__ double row_sum16(double s)
{
    s += row_dpp<0xB1>(s);
    s += row_dpp<0x4E>(s);
    s += row_dpp<0x141>(s);
    s += row_dpp<0x140>(s);
    return s;
}

// the sum over the wave, in every lane: the row sums, then the four of them through SGPRs
__device__ __forceinline__ double wave_sum64(double s)
{
    s = row_sum16(s);
    const int lo = __double2loint(s), hi = __double2hiint(s);
    double r4[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
        r4[q] = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * q), __builtin_amdgcn_readlane(lo, 16 * q));
    return (r4[0] + r4[1]) + (r4[2] + r4[3]);
}

// ---- the kernel value of EPI_KERNEL: k = v^eta and kp = eta v^(eta - 1) of a dot product v, with the lone-atom rule of
// similarity.py:94-103 (rl / cl: the row's / the column's atom has no neighbour).  ieta: the integer exponent or -1.
// v^(eta - 1): the reference's default exponent 4 without a loop, the other integers by multiplication, the rest by pow
__device__ __forceinline__ double kernel_pm1(double v, int ieta, double eta)
{
    if (ieta == 4) return v * v * v;
    if (ieta >= 1) {
        double pm1 = 1.0;
        for (int q = 1; q < ieta; q++) pm1 *= v;
        return pm1;
    }
    return pow(v, eta - 1.0);
}

// Declares K and KP from the dot product V; IETA = g.ieta, P = the product's GemmParams.  (A macro: functions for the
// selects spilled, see the head of this file.)
// (pow branch, exponent below 1: pm1 = +inf at v = 0, an orthogonal pair; k = 0^eta = 0, kp stays unbounded)
#define KERNEL_VALUE(K, KP, V, RL, CL, IETA, P)                                                                      \
    const double pm1_ = kernel_pm1(V, IETA, (P).eta);                                                                \
    const double eta_d_ = (IETA) >= 1 ? (double)(IETA) : (P).eta;                                                    \
    const double K = (!(RL) && !(CL)) ? (((IETA) < 1 && (V) == 0.0) ? 0.0 : pm1_ * (V))                              \
                                      : (((RL) && (CL)) ? 1.0 + (P).lone_m1 : 0.0);                                  \
    const double KP = (!(RL) && !(CL)) ? eta_d_ * pm1_ : 0.0;

// ---- tile entry.  With a host-built tile table (species-sorted operands: K_nm, K_mm, choli are block-diagonal) only the
// working tiles are launched, each with its trimmed reduction range; the table is ordered so that list position p sits on
// XCD p % 8 together with the other column tiles of the same row panel of A (one L2 fetches the panel once).  Without a
// table the grid is dense, row tile fastest (same XCD property), and the reduction runs over 0 .. K.
// Declares rt, ct, kbeg, kend of tile `bid` of the tile function it stands in, and LEAVES that function at a padding entry.
// TABLE_ONLY: a form that is never launched without a table carries no dense branch.
// (A macro: as a function — returning a struct, or filling references and returning "live" or "leave" — it moved the
// registers of gemm_nt_kernel<EPI_ROWSQ, 1, 32> and <EPI_SUBLOWER, 2, 32>, see the head of this file.)
#define TILE_ENTRY_OR_RETURN(TABLE_ONLY)                                                         \
    int rt, ct, kbeg = 0, kend = p.K;                                                            \
    if ((TABLE_ONLY) || g.p.tiles) {                                                             \
        const int4 t = g.p.tiles[bid];                                                           \
        rt = t.x & 0xffff; ct = t.y & 0xffff; kbeg = t.z; kend = t.w;                            \
        if (kend <= kbeg) return;  /* padding entry */                                           \
    } else {                                                                                     \
        rt = bid % g.rows_pad;                                                                   \
        ct = bid / g.rows_pad;                                                                   \
        if (rt >= g.row_tiles) return;                                                           \
    }

// SGPR_STAMPS=1 (diagnostic): the s_memtime stamp taken once the tile entry has arrived (`dep` = rt + ct)
__device__ __forceinline__ long long stamp_entry(const GemmArgs &g, int dep)
{
    long long t = 0;
    if (g.stamps) asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(dep));
    return t;
}

// ... and the tile's record of eight words at `o` (tools/stamps_*.py): start, end of the main loop, now,
// `klen_flags` (reduction length | second-problem flag << 20) | XCC_ID << 24 | HW_ID << 32, tile entry, end of the prologue
__device__ __forceinline__ void stamp_record(long long *o, long long t_start, long long t_entry, long long t_pro, long long t_loop,
                                             long long klen_flags)
{
    o[4] = t_entry; o[5] = t_pro;
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11));
    o[0] = t_start; o[1] = t_loop; o[2] = (long long)__builtin_amdgcn_s_memtime();
    o[3] = klen_flags | ((long long)xcc << 24) | ((long long)hw << 32);
}

// ---- EPI_KERNEL metadata, requested in front of the main loop so that the latency hides under it (all arrays are padded
// to whole tiles by the allocator).  Species slot / neighbour count of a row (a lane has four per 16-row block) ...
__device__ __forceinline__ void fetch_row_meta(const GemmArgs &g, const GemmParams &pk, int row, int &rs, int &rn)
{
    rs = g.row_slot[row];
    rn = pk.row_nn ? pk.row_nn[row] : 1;
}

// ... and slot / count / weight of a column (one per 16-column block)
__device__ __forceinline__ void fetch_col_meta(const GemmArgs &g, const GemmParams &pk, int col, int &cs, int &cn, double &mu)
{
    cs = g.col_slot[col];
    cn = pk.col_nn ? pk.col_nn[col] : 1;
    mu = pk.mu ? pk.mu[col] : 0.0;
}

// TM = MFMA row tiles per wave: 2 -> 64-row workgroup tiles, 1 -> 32-row tiles.
// __launch_bounds__(256, 2): two workgroups per CU = two waves per SIMD = a budget of 256 registers, which makes the
// compiler pick the VGPR form of the MFMAs; with the full 512 it picks the AGPR form and copies the sixteen
// accumulator registers to VGPRs and back around every trip of the stage loop (16 v_accvgpr_write + 16 _read each
// draining the matrix pipe).
// KD = depth of a stage of the 32-row form: 32 (two workgroups per CU) or 16 (36 KB of LDS, <= 128 registers: FOUR
// workgroups per CU — for launches of many short reductions, where the fixed cost of a tile (tile entry, first loads,
// epilogue: ~4 us, measured with per-tile stamps) is what the other resident workgroups have to cover).
template <int EPI, int TM = 2, int KD = 32>
struct GemmLds {
    static constexpr bool SWZ = KD == 16;
    static constexpr int LDR = SWZ ? KD : KD + 2;
    static constexpr int NBUF = TM == 1 ? 3 : 2, ASZ = 32 * TM * LDR, BSZ = BN * LDR;
    static constexpr int DOUBLES = NBUF * (ASZ + BSZ);  // LDS of one workgroup
};

// One tile of the family, as a device function: `bid` is the tile's position in the launch (the block index of a
// GEMM launch; descriptor.hip's reverse kernel hands its first workgroups to the covloss tiles this way), As / Bs the
// workgroup's LDS (GemmLds<...>::DOUBLES doubles in all).
template <int EPI, int TM = 2, int KD = 32>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs &g, const int bid, double *const As, double *const Bs)
{
    constexpr int BMT = 32 * TM;
    // EPI_WCOV: one launch serves two independent products that share the row dimension (W = Aw.Pm with
    // a plain store, covloss = K.choli^T with the row-square epilogue); the tile table says which.
    static_assert(EPI != EPI_FUSED || (TM == 1 && KD == 16), "the fused launch runs on the 32-row, 16-deep form");
    constexpr bool FUSED = EPI == EPI_FUSED;
    const int kind = (EPI == EPI_WCOV || FUSED) ? ((g.p.tiles[bid].x >> 16) & 3) : 0;   // 0 W, 1 covloss, 2 K_nm (FUSED only)
    const bool second = kind == 1;
    const bool third = FUSED && kind == 2;
    const GemmParams &p = third ? g.p3 : (second ? g.p2 : g.p);
    const bool do_store = EPI == EPI_STORE || ((EPI == EPI_WCOV || FUSED) && kind == 0);
    const bool do_kern = EPI == EPI_KERNEL || third;
    // 64-row tiles: two stages of A and B (68 KB, two workgroups per CU); 32-row tiles: three (76.5 KB, two per CU)
    // LDS rows: 32-deep stages are padded by two doubles (conflict-free fragment reads); 16-deep stages are XOR-swizzled
    // instead (16-B chunk c of row r sits at chunk c ^ ((r >> 1) & 7)): 36 KB for three stages, four workgroups per CU
    using L = GemmLds<EPI, TM, KD>;
    constexpr bool SWZ = L::SWZ;
    constexpr int LDR = L::LDR, ASZ = L::ASZ, BSZ = L::BSZ;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const long long t_start = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    TILE_ENTRY_OR_RETURN(false)
    const long long t_entry = stamp_entry(g, rt + ct);
    long long t_pro = 0;
    const int row0 = rt * BMT, col0 = ct * BN;
    const bool skip = (EPI == EPI_SUBLOWER && col0 > row0);  // symmetric update: lower tiles only

    v4d acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    if constexpr (FUSED) {
        // A W or covloss tile consumes the K / Aw rows of its row panel: it waits until every K_nm tile of that panel —
        // `need` of them, earlier in this launch's tile list, hence dispatched before it — has counted itself in.  One lane
        // polls (device-scope load, s_sleep between polls), the barrier holds the others; a poll that never succeeds (it
        // cannot, unless the dispatcher starts blocks out of order) gives up and flags the launch.
        if (!third) {
            if (tid == 0) {
                const int need = (g.p.tiles[bid].x >> 20) & 0xff, target = g.epoch * need;
                int spins = 0;
                while (__hip_atomic_load(g.panel_cnt + rt * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                    __builtin_amdgcn_s_sleep(16);
                    if (++spins > (1 << 20)) { *g.fuse_err = 4; break; }
                }
            }
            __syncthreads();
            // (no acquire fence: buffer_inv sc1 here throws the B panels out of the XCD's L2 with everything else — measured
            // 81 us for the launch against 62 with the A operand read past the caches instead, load_a2<true>)
        }
    }
    int e_rs[TM][4], e_rn[TM][4], e_cs[2], e_cn[2];
    double e_mu[2];
    if (EPI == EPI_KERNEL || FUSED) {
        // (FUSED: requested by every tile, with indices clamped for the tiles that do not use them — a load behind a
        // run-time condition would make the wait counts of the main loop collapse to vmcnt(0))
        const GemmParams &pk = FUSED ? g.p3 : p;
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
            for (int r = 0; r < 4; r++) fetch_row_meta(g, pk, row0 + wr * 16 * TM + tm * 16 + (lane >> 4) + 4 * r, e_rs[tm][r], e_rn[tm][r]);
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
            fetch_col_meta(g, pk, (FUSED && !third) ? 0 : col0 + wc * 32 + tn * 16 + (lane & 15), e_cs[tn], e_cn[tn], e_mu[tn]);
    }

    if constexpr (TM == 2) {
    if (!skip) {
        // LDS-staged main loop, KS = 32 deep stages, double-buffered in LDS and fetched TWO stages
        // ahead through registers: every stage touches new cache lines (compulsory L2 misses,
        // ~2000+ cycles under load) while its 32 MFMAs per wave issue in 2048 cycles.
        // Global side: thread t moves 64 contiguous bytes of row t/4 (full-line coalescing: the
        // four lanes of a quad cover two whole 128-B lines; fragment-shaped direct loads measured
        // TA-bound at 4x the cycles).  LDS side: row stride 34 doubles -> conflict-free ds_read_b64
        // fragment reads and 16-B aligned ds_write_b128 stores.
        constexpr int KS = 32, LD = KS + 2;
        const int lr = tid >> 2, lk = (tid & 3) * 8;
        const double *Ag = p.A + (size_t)(row0 + lr) * p.lda + lk;
        const double *Bg = p.B + (size_t)(col0 + lr) * p.ldb + lk;
        // register stages as plain named values (a struct taken by reference in a lambda ended up
        // in scratch: 272 B/lane of spills and a 45 us kernel)
        double2 pa0, pa1, pa2, pa3, pb0, pb1, pb2, pb3;  // stage "p"
        double2 qa0, qa1, qa2, qa3, qb0, qb1, qb2, qb3;  // stage "q"
#define GLOAD(S, K0)                                                                             \
    if ((K0) < kend) {                                                                           \
        if (TM == 2 || lr < BMT) {                                                               \
        S##a0 = *(const double2 *)(Ag + (K0)); S##a1 = *(const double2 *)(Ag + (K0) + 2);        \
        S##a2 = *(const double2 *)(Ag + (K0) + 4); S##a3 = *(const double2 *)(Ag + (K0) + 6);    \
        }                                                                                        \
        S##b0 = *(const double2 *)(Bg + (K0)); S##b1 = *(const double2 *)(Bg + (K0) + 2);        \
        S##b2 = *(const double2 *)(Bg + (K0) + 4); S##b3 = *(const double2 *)(Bg + (K0) + 6);    \
    }
#define LSTORE(S, BUF)                                                                           \
    {                                                                                            \
        double *da = &As[(BUF) * ASZ + lr * LD + lk], *db = &Bs[(BUF) * BSZ + lr * LD + lk];                       \
        if (TM == 2 || lr < BMT) {                                                               \
        *(double2 *)(da) = S##a0; *(double2 *)(da + 2) = S##a1;                                  \
        *(double2 *)(da + 4) = S##a2; *(double2 *)(da + 6) = S##a3;                              \
        }                                                                                        \
        *(double2 *)(db) = S##b0; *(double2 *)(db + 2) = S##b1;                                  \
        *(double2 *)(db + 4) = S##b2; *(double2 *)(db + 6) = S##b3;                              \
    }
        const int fa = (wr * 16 * TM + (lane & 15)) * LD + (lane >> 4);
        const int fb = (wc * 32 + (lane & 15)) * LD + (lane >> 4);
        auto compute = [&](int buf) {
#pragma unroll
            for (int kk = 0; kk < KS; kk += 4) {
                const double b0 = Bs[buf * BSZ + fb + kk], b1 = Bs[buf * BSZ + fb + 16 * LD + kk];
#pragma unroll
                for (int tm = 0; tm < TM; tm++) {
                    const double a0 = As[buf * ASZ + fa + tm * 16 * LD + kk];
                    acc[tm][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[tm][0], 0, 0, 0);
                    acc[tm][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[tm][1], 0, 0, 0);
                }
            }
        };
        // prologue: stage 0 -> LDS buffer 0, stage 1 and 2 in flight in registers
        pa0 = pa1 = pa2 = pa3 = pb0 = pb1 = pb2 = pb3 = make_double2(0.0, 0.0);
        qa0 = qa1 = qa2 = qa3 = qb0 = qb1 = qb2 = qb3 = make_double2(0.0, 0.0);
        GLOAD(p, kbeg);
        GLOAD(q, kbeg + KS);
        LSTORE(p, 0);
        GLOAD(p, kbeg + 2 * KS);
        __syncthreads();
        // steady state, unrolled by two so the register stages keep static names
        for (int k0 = kbeg; k0 < kend; k0 += 2 * KS) {
            // buffer 0 holds stage k0; s1 = stage k0+KS; s0 = stage k0+2KS
            if (k0 + KS < kend) LSTORE(q, 1);
            GLOAD(q, k0 + 3 * KS);
            compute(0);
            __syncthreads();
            if (k0 + KS >= kend) break;
            // buffer 1 holds stage k0+KS; s0 = stage k0+2KS; s1 = stage k0+3KS
            if (k0 + 2 * KS < kend) LSTORE(p, 0);
            GLOAD(p, k0 + 4 * KS);
            compute(1);
            __syncthreads();
        }
    }

    } else {
        // 32-row tiles.  Stage s lives in LDS buffer s % 3 (cur / nxt / stb rotate).  One barrier at the TOP of a
        // stage: behind it every wave is done reading stage s-1, whose buffer now takes stage s+2, and the stores of
        // stage s+1 (issued during stage s-1) are visible — so the first fragments of stage s+1 are read before the
        // next barrier and the MFMA stream does not stop at the stage boundary.  The stage body is straight-line:
        // eight k-steps of two MFMAs, the fragments one step ahead, and in the shadow of the MFMAs the six
        // ds_write_b128 of stage s+2 (steps 0-2) and the six global loads of stage s+4 (steps 3-5);
        // __builtin_amdgcn_sched_barrier keeps them there.  The steady-state loop has no conditions and is entered
        // from an unconditional prologue, so the compiler counts vmcnt exactly (vmcnt(10) / vmcnt(6): a conditional
        // load anywhere before the loop made it wait for vmcnt(0), i.e. a prefetch distance of one stage).
        // tools/ubench_gemm4.hip, dense 4096 x 512 x 320: 12.8 -> 10.2 us for two tiles per CU (MFMA bound 8.5).
        if constexpr (KD == 16) {
        // 16-deep stages: FOUR register sets (one double2 of A, two of B per thread and set), set k = stages k mod 4.
        // At the top of stage s the LDS holds s and s + 1, the sets s + 2 .. s + 5; stage s stores s + 2 and reloads
        // that set with s + 6 (3.5 stages to land; the two-set form below gave a load 1.5 stages, and the loop ran at
        // the miss latency, not at the MFMA rate: s_memtime stamps).  Loads past the last stage re-read the last one
        // (clamped: in bounds, never consumed), so no load is conditional and the compiler's vmcnt stays exact.
        constexpr int KS = 16, LD = 16, NJ = 4;
        const int lrb = tid >> 2, lra = tid >> 3;
        const double *Ag = p.A + (size_t)(row0 + lra) * p.lda + (tid & 7) * 2 + kbeg;
        const double *Bg = p.B + (size_t)(col0 + lrb) * p.ldb + (tid & 3) * 4 + kbeg;
        const int ga = (lra >> 1) & 7, gb = (lrb >> 1) & 7;
        const int la = lra * LD + (((tid & 7) ^ ga) << 1);
        const int lb = lrb * LD + ((((tid & 3) << 1) ^ gb) << 1);
        const int lb1 = lrb * LD + (((((tid & 3) << 1) | 1) ^ gb) << 1);
        const int fra_r = wr * 16 + (lane & 15), frb_r = wc * 32 + (lane & 15);
        int oa[4], ob[4];
#ifdef SGPR_WCOV_SPLIT_READS
        int ob2[4];
#endif
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = 2 * j + (lane >> 5), lo = (lane >> 4) & 1;
            oa[j] = fra_r * LD + ((c ^ ((fra_r >> 1) & 7)) << 1) + lo;
            ob[j] = frb_r * LD + ((c ^ ((frb_r >> 1) & 7)) << 1) + lo;  // row + 16 has the same key
#ifdef SGPR_WCOV_SPLIT_READS
            ob2[j] = ob[j] + 16 * LD;
            asm volatile("" : "+v"(ob2[j]));   // (an address of its own: the two reads cannot be merged into one ds_read2st64_b64)
#endif
        }
        // (The two column blocks' fragments — rows r and r + 16, same swizzle key — are merged by the compiler into one
        // ds_read2st64_b64, which is banked modulo 32 in 16-lane groups (MI355X_MICROARCH.md, LDS): rows r and r + 1 share a key
        // and a 128-byte row is 32 banks, so the merged read is 2-way conflicted where two ds_read_b64 (modulo 64, 32-lane
        // groups) are not.  Measured both ways with the counters (-DSGPR_WCOV_SPLIT_READS keeps the reads apart): merged
        // SQ_LDS_BANK_CONFLICT 2.49 M of 5.83 M LDS-active cycles per launch, apart 0.91 M of 3.46 M (what is left: the
        // ds_write_b128 stores) — and the launch 22.96 -> 23.53 us (hip events), 128 instead of 117 VGPRs.  The LDS is not what this
        // kernel waits for (a CU's four tiles need 10 us of MFMA time; entry, first loads and epilogue of tiles that all start
        // together are the rest): left merged.)
        double2 xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3, xc0, xc1, xc2, xc3;  // (named: indexed arrays went to scratch)
        double fra[2], frb[2][2];
        const int nst = (kend - kbeg + KS - 1) / KS, last = nst - 1;
#define GL4(K, ST) { const int st_ = min((ST), last) * KS; xa##K = load_a2<FUSED>(Ag + st_); xb##K = *(const double2 *)(Bg + st_); xc##K = *(const double2 *)(Bg + st_ + 2); }
#define LS4A(K, BUF) { *(double2 *)(As + (BUF) * ASZ + la) = xa##K; }
#define LS4B(K, BUF) { *(double2 *)(Bs + (BUF) * BSZ + lb) = xb##K; *(double2 *)(Bs + (BUF) * BSZ + lb1) = xc##K; }
#ifdef SGPR_WCOV_SPLIT_READS
#define RDF4(SL, BUF, J) { frb[SL][0] = Bs[(BUF) * BSZ + ob[J]]; frb[SL][1] = Bs[(BUF) * BSZ + ob2[J]]; fra[SL] = As[(BUF) * ASZ + oa[J]]; }
#else
#define RDF4(SL, BUF, J) { frb[SL][0] = Bs[(BUF) * BSZ + ob[J]]; frb[SL][1] = Bs[(BUF) * BSZ + ob[J] + 16 * LD]; fra[SL] = As[(BUF) * ASZ + oa[J]]; }
#endif
#define STAGE4(K, DO_LD, SLD)                                                                    \
    {                                                                                            \
        __syncthreads();                                                                         \
        _Pragma("unroll") for (int j = 0; j < NJ; j++) {                                         \
            const int sl = j & 1;                                                                \
            if (j < NJ - 1) RDF4(sl ^ 1, cur, j + 1) else RDF4(sl ^ 1, nxt, 0)                   \
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][0], acc[0][0], 0, 0, 0); \
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][1], acc[0][1], 0, 0, 0); \
            if (j == 0) LS4A(K, stb)                                                             \
            if (j == 1) LS4B(K, stb)                                                             \
            if (DO_LD) { if (j == 2) GL4(K, SLD) }                                               \
            __builtin_amdgcn_sched_barrier(0);                                                   \
        }                                                                                        \
        const int t_ = cur; cur = nxt; nxt = stb; stb = t_;                                      \
    }
        int cur = 0, nxt = 1, stb = 2, s = 0;
        GL4(0, 0) GL4(1, 1)
        __builtin_amdgcn_sched_barrier(0);
        GL4(2, 2) GL4(3, 3)
        __builtin_amdgcn_sched_barrier(0);
        LS4A(0, 0) LS4B(0, 0)
        GL4(0, 4)
        __builtin_amdgcn_sched_barrier(0);
        LS4A(1, 1) LS4B(1, 1)
        GL4(1, 5)
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
        RDF4(0, 0, 0)
        for (; s + 4 <= nst; s += 4) {
            STAGE4(2, 1, s + 6)
            STAGE4(3, 1, s + 7)
            STAGE4(0, 1, s + 8)
            STAGE4(1, 1, s + 9)
        }
        {
            const int rem = nst - s;  // at most three stages left: stores only
            if (rem > 0) STAGE4(2, 0, 0)
            if (rem > 1) STAGE4(3, 0, 0)
            if (rem > 2) STAGE4(0, 0, 0)
        }
#undef GL4
#undef LS4A
#undef LS4B
#undef RDF4
#undef STAGE4
        } else {
        constexpr int KS = KD, LD = LDR, NJ = KS / 4, NA = KS / 16, NB = KS / 8;
        // global side: 64 B (KS = 32) or 32 B (16) per thread of B (4 threads per row), half of that of A (8 per row)
        const int lrb = tid >> 2, lkb = (tid & 3) * (KS / 4);
        const int lra = tid >> 3, lka = (tid & 7) * (KS / 8);
        const double *Ag = p.A + (size_t)(row0 + lra) * p.lda + lka + kbeg;
        const double *Bg = p.B + (size_t)(col0 + lrb) * p.ldb + lkb + kbeg;
        const int ga = (lra >> 1) & 7, gb = (lrb >> 1) & 7;  // swizzle keys of the rows this thread stores
        const int la = SWZ ? lra * LD + (((tid & 7) ^ ga) << 1) : lra * LD + lka;
        const int lb = SWZ ? lrb * LD + ((((tid & 3) << 1) ^ gb) << 1) : lrb * LD + lkb;
        const int lb1 = SWZ ? lrb * LD + (((((tid & 3) << 1) | 1) ^ gb) << 1) : lb + 2;  // second chunk of B
        const int fra_r = wr * 16 + (lane & 15), frb_r = wc * 32 + (lane & 15);
        const int fa = fra_r * LD + (lane >> 4);
        const int fb = frb_r * LD + (lane >> 4);
        // swizzled fragment offsets of the four k-steps: chunk 2j + (lane >> 5), low double (lane >> 4) & 1
        int oa[4], ob[4];
        if (SWZ) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = 2 * j + (lane >> 5), lo = (lane >> 4) & 1;
                oa[j] = fra_r * LD + ((c ^ ((fra_r >> 1) & 7)) << 1) + lo;
                ob[j] = frb_r * LD + ((c ^ ((frb_r >> 1) & 7)) << 1) + lo;  // row + 16 has the same key
            }
        }
        double2 pa[2], pb[4], qa[2], qb[4];  // KS = 16 uses the first 1 / 2 of them
        double fra[2], frb[2][2];
        const int nst = (kend - kbeg + KS - 1) / KS;
#define GLA(S, ST, I0, I1) _Pragma("unroll") for (int i = I0; i < I1; i++) S##a[i] = *(const double2 *)(Ag + (ST) * KS + 2 * i);
#define GLB(S, ST, I0, I1) _Pragma("unroll") for (int i = I0; i < I1; i++) S##b[i] = *(const double2 *)(Bg + (ST) * KS + 2 * i);
#define LSA(S, BUF, I0, I1) _Pragma("unroll") for (int i = I0; i < I1; i++) *(double2 *)(As + (BUF) * ASZ + la + 2 * i) = S##a[i];
#define LSB(S, BUF, I0, I1) _Pragma("unroll") for (int i = I0; i < I1; i++) *(double2 *)(Bs + (BUF) * BSZ + (SWZ ? (i ? lb1 : lb) : lb + 2 * i)) = S##b[i];
#define RDF(SL, BUF, KK)                                                                         \
    {                                                                                            \
        if (SWZ) {                                                                               \
            frb[SL][0] = Bs[(BUF) * BSZ + ob[((KK) / 4) & 3]]; frb[SL][1] = Bs[(BUF) * BSZ + ob[((KK) / 4) & 3] + 16 * LD]; \
            fra[SL] = As[(BUF) * ASZ + oa[((KK) / 4) & 3]];                                      \
        } else {                                                                                 \
            frb[SL][0] = Bs[(BUF) * BSZ + fb + (KK)]; frb[SL][1] = Bs[(BUF) * BSZ + fb + 16 * LD + (KK)]; \
            fra[SL] = As[(BUF) * ASZ + fa + (KK)];                                               \
        }                                                                                        \
    }
#define STAGE(R, DO_ST, DO_LD, SLD)                                                              \
    {                                                                                            \
        __syncthreads();                                                                         \
        _Pragma("unroll") for (int j = 0; j < NJ; j++) {                                         \
            const int sl = j & 1;                                                                \
            if (j < NJ - 1) RDF(sl ^ 1, cur, 4 * (j + 1)) else RDF(sl ^ 1, nxt, 0)               \
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][0], acc[0][0], 0, 0, 0); \
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][1], acc[0][1], 0, 0, 0); \
            if (KS == 32) {                                                                      \
                if (DO_ST) { if (j == 0) LSA(R, stb, 0, 2) if (j == 1) LSB(R, stb, 0, 2) if (j == 2) LSB(R, stb, 2, 4) } \
                if (DO_LD) { if (j == 3) GLA(R, SLD, 0, 2) if (j == 4) GLB(R, SLD, 0, 2) if (j == 5) GLB(R, SLD, 2, 4) } \
            } else {                                                                             \
                if (DO_ST) { if (j == 0) LSA(R, stb, 0, 1) if (j == 1) LSB(R, stb, 0, 2) }       \
                if (DO_LD) { if (j == 2) GLA(R, SLD, 0, 1) if (j == 3) GLB(R, SLD, 0, 2) }       \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                   \
        }                                                                                        \
        const int t_ = cur; cur = nxt; nxt = stb; stb = t_;                                      \
    }
        for (int i = 0; i < NA; i++) pa[i] = qa[i] = make_double2(0.0, 0.0);
        for (int i = 0; i < NB; i++) pb[i] = qb[i] = make_double2(0.0, 0.0);
        int cur = 0, nxt = 1, stb = 2, s = 0;
        if (nst >= 6) {
            GLA(p, 0, 0, NA) GLB(p, 0, 0, NB)
            GLA(q, 1, 0, NA) GLB(q, 1, 0, NB)
            LSA(p, 0, 0, NA) LSB(p, 0, 0, NB)
            GLA(p, 2, 0, NA) GLB(p, 2, 0, NB)
            LSA(q, 1, 0, NA) LSB(q, 1, 0, NB)
            GLA(q, 3, 0, NA) GLB(q, 3, 0, NB)
            __syncthreads();
            if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
            RDF(0, 0, 0)
            for (; s + 5 < nst; s += 2) {  // both stages of the pair store (s+2, s+3) and load (s+4, s+5)
                STAGE(p, 1, 1, s + 4)
                STAGE(q, 1, 1, s + 5)
            }
        } else {
            GLA(p, 0, 0, NA) GLB(p, 0, 0, NB)
            if (nst > 1) { GLA(q, 1, 0, NA) GLB(q, 1, 0, NB) }
            LSA(p, 0, 0, NA) LSB(p, 0, 0, NB)
            if (nst > 2) { GLA(p, 2, 0, NA) GLB(p, 2, 0, NB) }
            LSA(q, 1, 0, NA) LSB(q, 1, 0, NB)
            if (nst > 3) { GLA(q, 3, 0, NA) GLB(q, 3, 0, NB) }
            __syncthreads();
            if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
            RDF(0, 0, 0)
        }
        // at most five stages left; one of them may still load
        for (; s < nst; s += 2) {
            if (s + 4 < nst) STAGE(p, 1, 1, s + 4)
            else if (s + 2 < nst) STAGE(p, 1, 0, 0)
            else STAGE(p, 0, 0, 0)
            if (s + 1 >= nst) break;
            if (s + 3 < nst) STAGE(q, 1, 0, 0)
            else STAGE(q, 0, 0, 0)
        }
#undef GLA
#undef GLB
#undef LSA
#undef LSB
#undef RDF
#undef STAGE
        }
    }

#undef GLOAD
#undef LSTORE
    const long long t_loop = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    // ------------------------------------------------------------------ epilogues
    // C/D map of v_mfma_f64_16x16x4_f64: col = lane&15, row = (lane>>4) + 4*reg
    double esum = 0.0;
    if (!skip) {
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
            double rsq[4] = {0, 0, 0, 0};
#pragma unroll
            for (int tn = 0; tn < 2; tn++) {
                const int col = col0 + wc * 32 + tn * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = row0 + wr * 16 * TM + tm * 16 + (lane >> 4) + 4 * r;
                    const double v = acc[tm][tn][r];
                    if (do_store) {
                        if (row < p.M && col < p.N) {
                            // (W of the grouped launch is read by the reverse kernel only: write-through, sgpr_internal.h)
                            if constexpr (EPI == EPI_WCOV) st_wt(&p.C[(size_t)row * p.ldc + col], v);
                            else p.C[(size_t)row * p.ldc + col] = v;
                        }
                    } else if (EPI == EPI_SUBLOWER) {
                        if (row < p.M && col < p.N) p.C[(size_t)row * p.ldc + col] -= v;
                    } else if (do_kern) {
                        // branch-free: per-row / per-column metadata was fetched before the main
                        // loop (a load inside a data-dependent branch cost one L2 round trip per
                        // element: 24.7k cycles of epilogue, measured with s_memtime stamps)
                        const bool same = e_rs[tm][r] == e_cs[tn];
                        const bool rl = e_rn[tm][r] == 0, cl = e_cn[tn] == 0;
                        KERNEL_VALUE(k, kp, v, rl, cl, g.ieta, p)
                        if (same && row < p.M && col < p.N) {
                            if constexpr (FUSED) {
                                // (write-through, device scope: read by other workgroups of this launch)
                                __hip_atomic_store(&p.C[(size_t)row * p.ldc + col], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (p.Aw) __hip_atomic_store(&p.Aw[(size_t)row * p.ldc + col], e_mu[tn] * kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            } else {
                                p.C[(size_t)row * p.ldc + col] = k;
                                if (p.Aw) p.Aw[(size_t)row * p.ldc + col] = e_mu[tn] * kp;
                            }
                            esum += k * e_mu[tn];
                        }
                    } else {  // EPI_ROWSQ
                        if (col < p.N) rsq[r] += v * v;
                    }
                }
            }
            if (EPI == EPI_ROWSQ || ((EPI == EPI_WCOV || FUSED) && second)) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double s = row_sum16(rsq[r]);
                    const int row = row0 + wr * 16 * TM + tm * 16 + (lane >> 4) + 4 * r;
                    if ((lane & 15) == 0 && row < p.M && s != 0.0) {
                        if constexpr (EPI == EPI_WCOV) st_wt(&p.rowsq[(size_t)row * p.rowsq_ld + 2 * ct + wc], s);
                        else p.rowsq[(size_t)row * p.rowsq_ld + 2 * ct + wc] = s;
                    }
                }
            }
        }
    }
    if (do_kern && g.Epart) {
        // one energy partial per WAVE (no workgroup barrier: the waves retire independently)
        esum = wave_sum64(esum);
        if (lane == 0) g.Epart[(size_t)(g.p.tiles ? bid : rt * g.col_tiles + ct) * 4 + wave] = esum;
    }
    if constexpr (FUSED) {
        // a K_nm tile counts itself in: every wave has drained its stores, the barrier collects the waves, one lane adds
        if (third) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_fetch_add(g.panel_cnt + rt * 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (g.stamps && threadIdx.x == 0)
        stamp_record(g.stamps + (size_t)bid * 8, t_start, t_entry, t_pro, t_loop, (long long)(kend - kbeg) | ((long long)second << 20));
}


// ---------------------------------------------------------------------------------------------------------------
// EIGHT waves on one 32 x 64 tile (512 threads): wave (wr = wave >> 2, wc = wave & 3) owns ONE 16 x 16 block of the
// result and runs every k-step of every stage, so each element still accumulates k-step after k-step in the same
// order as in the four-wave form (bit-identical results).  A stage is three doubles per thread (one of A, a double2
// of B), so SIX stages fit in registers beside the three in LDS (78 VGPRs; the four-wave form holds four sets in 117).
// Per-tile s_memtime stamps of the K_nm launch at 4096 / 512 (416 tiles on 256 CUs), cycles per 32-deep stage of the
// main loop: four waves, two register sets 2527 — eight waves, two sets 2475 (more waves did not help: the loop was
// waiting for loads issued 1.5 stages earlier, every first touch of a stage being a miss) — eight waves, six sets 1690,
// which is the MFMA rate of the CUs that hold two tiles (64 cycles per MFMA: 1024 per tile and stage).  What is left
// of the launch outside the loop: tile entry 0.9k, the first stages' arrival 6.7k, epilogue 2.6k cycles.
// Same LDS image as the four-wave form (three 16-deep stages, XOR-swizzled 16-byte chunks, 36 KB).
// HALF: the same tile cut in two — FOUR waves on 16 x 64 (256 threads), still one 16 x 16 block per wave, now ONE wave per
// SIMD.  For launches with fewer tiles than CUs (a rank's share of a sharded frame, frames of a few hundred atoms): a tile
// alone on its CU is bound by its own chain of dependent MFMAs — two waves per SIMD alternate on the matrix pipe, 1024 cycles
// per 32-deep stage — and a half tile on twice as many CUs runs that chain at 512 (K_nm of rank 0's share at world 8: 10.0 ->
// 7.9 us).  With the grouped W + covloss launch too (EPI_WCOV / EPI_ROWSQ, HALF only): the row-square sums of a 32-column
// half are formed lane by lane from the two waves' blocks (through LDS) and reduced as in the other forms — the same bits.
template <int EPI, bool HALF = false>
__device__ __forceinline__ void gemm_tile_body8(const GemmArgs &g, const int bid, double *const As, double *const Bs)
{
    static_assert(EPI == EPI_KERNEL || EPI == EPI_STORE || (HALF && (EPI == EPI_WCOV || EPI == EPI_ROWSQ)), "eight-wave form: K_nm and W");
    constexpr int KS = 16, LD = 16, ASZ = 32 * LD, BSZ = BN * LD, NJ = KS / 4, BMT = HALF ? 16 : 32;
    const bool second = (EPI == EPI_WCOV) && ((g.p.tiles[bid].x >> 16) & 1);
    const GemmParams &p = second ? g.p2 : g.p;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = HALF ? 0 : wave >> 2, wc = wave & 3;
    const long long t_start = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    TILE_ENTRY_OR_RETURN(false)
    const long long t_entry = stamp_entry(g, rt + ct);
    long long t_pro = 0;
    const int row0 = rt * BMT, col0 = ct * BN;
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
    int e_rs[4], e_rn[4], e_cs = 0, e_cn = 1;
    double e_mu = 0.0;
    if (EPI == EPI_KERNEL) {
        // (this form's own text: through fetch_row_meta / fetch_col_meta its two EPI_KERNEL kernels changed their registers)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = row0 + wr * 16 + (lane >> 4) + 4 * r;
            e_rs[r] = g.row_slot[row];
            e_rn[r] = p.row_nn ? p.row_nn[row] : 1;
        }
        const int col = col0 + wc * 16 + (lane & 15);
        e_cs = g.col_slot[col];
        e_cn = p.col_nn ? p.col_nn[col] : 1;
        e_mu = p.mu ? p.mu[col] : 0.0;
    }
    // global side: A (32 rows x 16 doubles) one double per thread, B (64 rows x 16 doubles) one 16-byte chunk per thread
    const int ara = tid >> 4, aca = tid & 15;
    const int brb = tid >> 3, bcb = tid & 7;
    const double *Ag = p.A + (size_t)(row0 + ara) * p.lda + aca + kbeg;
    const double *Bg = p.B + (size_t)(col0 + brb) * p.ldb + 2 * bcb + kbeg;
    const int la = ara * LD + ((((aca >> 1) ^ ((ara >> 1) & 7)) << 1) | (aca & 1));
    const int lb = brb * LD + ((bcb ^ ((brb >> 1) & 7)) << 1);   // (HALF: a thread also moves row brb + 32 of B — the same swizzle key)
    const int fra_r = wr * 16 + (lane & 15), frb_r = wc * 16 + (lane & 15);
    int oa[4], ob[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = 2 * j + (lane >> 5), lo = (lane >> 4) & 1;
        oa[j] = fra_r * LD + ((c ^ ((fra_r >> 1) & 7)) << 1) + lo;
        ob[j] = frb_r * LD + ((c ^ ((frb_r >> 1) & 7)) << 1) + lo;
    }
    // Register stages: NSET sets of (one double of A, one double2 of B) per thread; set k carries the stages = k mod NSET.
    // At the top of stage s the LDS holds stages s and s + 1 and the sets hold s + 2 .. s + NSET + 1; stage s stores
    // s + 2 and reloads that set with s + NSET + 2: a load has NSET - 1/2 stages (of 256 MFMA cycles per tile on the CU)
    // to land.  Every first touch of a stage is a compulsory miss (all tiles of a row panel start together), ~2000
    // cycles under load: with two sets (1.5 stages ahead) the loop ran at 1240 cycles per stage whatever the number
    // of waves (s_memtime stamps).  Loads past the last stage re-read the last one (clamped, in bounds, never consumed):
    // no conditional load anywhere, the compiler's vmcnt stays exact.
    constexpr int NSET = 6;
    double ra0, ra1, ra2, ra3, ra4, ra5;  // (named: an indexed array of them was placed in scratch)
    double2 rb0, rb1, rb2, rb3, rb4, rb5;
    double2 rd0, rd1, rd2, rd3, rd4, rd5;   // HALF: the second row of B
    double fra[2], frb[2];
    const int nst = (kend - kbeg + KS - 1) / KS, last = nst - 1;
#define GL8(K, ST) { const int st_ = min((ST), last) * KS; ra##K = Ag[st_]; rb##K = *(const double2 *)(Bg + st_); \
                     if constexpr (HALF) rd##K = *(const double2 *)(Bg + (size_t)32 * p.ldb + st_); }
#define LS8(K, BUF) { As[(BUF) * ASZ + la] = ra##K; *(double2 *)(Bs + (BUF) * BSZ + lb) = rb##K; \
                      if constexpr (HALF) *(double2 *)(Bs + (BUF) * BSZ + lb + 32 * LD) = rd##K; }
#define RDF8(SL, BUF, KK) { frb[SL] = Bs[(BUF) * BSZ + ob[((KK) / 4) & 3]]; fra[SL] = As[(BUF) * ASZ + oa[((KK) / 4) & 3]]; }
#define STAGE8(K, DO_LD, SLD)                                                                    \
    {                                                                                            \
        __syncthreads();                                                                         \
        _Pragma("unroll") for (int j = 0; j < NJ; j++) {                                         \
            const int sl = j & 1;                                                                \
            if (j < NJ - 1) RDF8(sl ^ 1, cur, 4 * (j + 1)) else RDF8(sl ^ 1, nxt, 0)             \
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl], acc, 0, 0, 0);          \
            if (j == 0) LS8(K, stb)                                                              \
            if (DO_LD) { if (j == 2) GL8(K, SLD) }                                               \
            __builtin_amdgcn_sched_barrier(0);                                                   \
        }                                                                                        \
        const int t_ = cur; cur = nxt; nxt = stb; stb = t_;                                      \
    }
    int cur = 0, nxt = 1, stb = 2, s = 0;
    // (pinned in this order: the compiler otherwise issues stages 0 and 1 last and the first store waits for all)
    GL8(0, 0) GL8(1, 1)
    __builtin_amdgcn_sched_barrier(0);
    GL8(2, 2) GL8(3, 3) GL8(4, 4) GL8(5, 5)
    __builtin_amdgcn_sched_barrier(0);
    LS8(0, 0)
    GL8(0, 6)
    __builtin_amdgcn_sched_barrier(0);
    LS8(1, 1)
    GL8(1, 7)
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
    RDF8(0, 0, 0)
    for (; s + NSET <= nst; s += NSET) {
        STAGE8(2, 1, s + 8)
        STAGE8(3, 1, s + 9)
        STAGE8(4, 1, s + 10)
        STAGE8(5, 1, s + 11)
        STAGE8(0, 1, s + 12)
        STAGE8(1, 1, s + 13)
    }
    {
        const int rem = nst - s;  // at most five stages left: stores only
        if (rem > 0) STAGE8(2, 0, 0)
        if (rem > 1) STAGE8(3, 0, 0)
        if (rem > 2) STAGE8(4, 0, 0)
        if (rem > 3) STAGE8(5, 0, 0)
        if (rem > 4) STAGE8(0, 0, 0)
    }
#undef GL8
#undef LS8
#undef RDF8
#undef STAGE8
    const long long t_loop = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    // epilogue: C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
    double esum = 0.0;
    {
        const int col = col0 + wc * 16 + (lane & 15);
        double rsq[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = row0 + wr * 16 + (lane >> 4) + 4 * r;
            const double v = acc[r];
            if (EPI == EPI_STORE || (EPI == EPI_WCOV && !second)) {
                if (row < p.M && col < p.N) p.C[(size_t)row * p.ldc + col] = v;
            } else if (EPI == EPI_KERNEL) {
                const bool same = e_rs[r] == e_cs;
                const bool rl = e_rn[r] == 0, cl = e_cn == 0;
                KERNEL_VALUE(k, kp, v, rl, cl, g.ieta, p)
                if (same && row < p.M && col < p.N) {
                    // (K and Aw are read by the next launch only: write-through, sgpr_internal.h)
                    st_wt(&p.C[(size_t)row * p.ldc + col], k);
                    if (p.Aw) st_wt(&p.Aw[(size_t)row * p.ldc + col], e_mu * kp);
                    esum += k * e_mu;
                }
            } else {  // row squares (covloss): the value itself; squared below
                rsq[r] = col < p.N ? v : 0.0;
            }
        }
        if constexpr (HALF && (EPI == EPI_ROWSQ || EPI == EPI_WCOV)) {
            // A 32-column half is two waves' blocks here (one wave's two blocks in the four-wave form, which adds them lane by
            // lane — block 0 first — before the row sum): the odd wave hands its squares over through LDS.  The tile's stages are
            // done with (the barrier below is reached by every wave of the tile: `second` is uniform over the workgroup).
            if (EPI == EPI_ROWSQ || second) {
                __syncthreads();
                double *xs = As;   // [2][64][4]
                if (wc & 1) {
#pragma unroll
                    for (int r = 0; r < 4; r++) xs[((wc >> 1) * 64 + lane) * 4 + r] = rsq[r];
                }
                __syncthreads();
                if (!(wc & 1)) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        // (rsq += v * v of the other forms is a fused multiply-add: block 0 squared, block 1 fused onto it)
                        const double v1 = xs[((wc >> 1) * 64 + lane) * 4 + r];
                        const double sq = row_sum16(fma(v1, v1, rsq[r] * rsq[r]));
                        const int row = row0 + (lane >> 4) + 4 * r;
                        if ((lane & 15) == 0 && row < p.M && sq != 0.0) p.rowsq[(size_t)row * p.rowsq_ld + 2 * ct + (wc >> 1)] = sq;
                    }
                }
            }
        }
    }
    if (EPI == EPI_KERNEL && g.Epart) {
        esum = wave_sum64(esum);
        if (lane == 0) {
            double *ep = g.Epart + (size_t)(g.p.tiles ? bid : rt * g.col_tiles + ct) * 8;
            st_wt(&ep[wave], esum);
            if constexpr (HALF) st_wt(&ep[wave + 4], 0.0);   // (the reducer sums eight partials per tile)
        }
    }
    if (g.stamps && threadIdx.x == 0)   // (this form's record carries no second-problem flag)
        stamp_record(g.stamps + (size_t)bid * 8, t_start, t_entry, t_pro, t_loop, (long long)(kend - kbeg));
}

// ---------------------------------------------------------------------------------------------------------------
// EIGHT waves on one 64 x 64 tile (512 threads, waves as 4 x 2, two 16 x 16 blocks per wave: the four-wave 32-row form
// with twice the rows).  Why: the stamps of both GEMM launches show the chip delivering 10 - 16 bytes per cycle and CU
// to them, whatever the prefetch depth — a 32 x 64 tile asks for 12 KB per 16-deep stage, and the 23.6 stage-pairs a CU
// works through in the grouped W + covloss launch are 580 KB: 36k cycles at 16 B per cycle, which IS the launch
// (CU finish p50 37k cycles against 24k of MFMA work).  A 64 x 64 tile moves 16 KB per stage for twice the flops:
// two thirds of the bytes.  Same LDS image (three 16-deep stages, XOR-swizzled chunks, now 48 KB: two workgroups per
// CU = the same sixteen waves), six register stages of one double2 of A and one of B per thread, every dot product
// accumulated k-step after k-step as in the other forms (bit-identical results).
// NSET = register stage sets: 6 (two workgroups per CU, <= 128 VGPRs) or 3 (THREE workgroups per CU, <= 80 VGPRs: a tile's
// entry, first arrival and epilogue — 9k cycles in which it issues no MFMA — are then covered by two other tiles instead of
// one; with three tiles on the matrix pipe a stage lasts 3k cycles, so 2.5 stages of look-ahead still cover a miss).
template <int EPI, int NSET = 6>
__device__ __forceinline__ void gemm_tile_body8r64(const GemmArgs &g, const int bid, double *const As, double *const Bs)
{
    static_assert(NSET == 6 || NSET == 3, "register stage sets");
    constexpr int KS = 16, LD = 16, ASZ = 64 * LD, BSZ = BN * LD, NJ = KS / 4;
    const bool second = (EPI == EPI_WCOV) && ((g.p.tiles[bid].x >> 16) & 1);
    const GemmParams &p = second ? g.p2 : g.p;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const long long t_start = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    TILE_ENTRY_OR_RETURN(true)   // (always launched with a table)
    const long long t_entry = stamp_entry(g, rt + ct);
    long long t_pro = 0;
    const int row0 = rt * 64, col0 = ct * BN;
    v4d acc[2];
    acc[0] = acc[1] = (v4d){0.0, 0.0, 0.0, 0.0};
    int e_rs[4], e_rn[4], e_cs[2], e_cn[2];
    double e_mu[2];
    if (EPI == EPI_KERNEL) {
#pragma unroll
        for (int r = 0; r < 4; r++) fetch_row_meta(g, p, row0 + wr * 16 + (lane >> 4) + 4 * r, e_rs[r], e_rn[r]);
#pragma unroll
        for (int tn = 0; tn < 2; tn++) fetch_col_meta(g, p, col0 + wc * 32 + tn * 16 + (lane & 15), e_cs[tn], e_cn[tn], e_mu[tn]);
    }
    // global side: 64 rows x 16 doubles of A and of B per stage, one 16-byte chunk of each per thread
    const int lr = tid >> 3, lc = tid & 7;
    const double *Ag = p.A + (size_t)(row0 + lr) * p.lda + 2 * lc + kbeg;
    const double *Bg = p.B + (size_t)(col0 + lr) * p.ldb + 2 * lc + kbeg;
    const int ll = lr * LD + ((lc ^ ((lr >> 1) & 7)) << 1);
    const int fra_r = wr * 16 + (lane & 15), frb_r = wc * 32 + (lane & 15);
    int oa[4], ob[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = 2 * j + (lane >> 5), lo = (lane >> 4) & 1;
        oa[j] = fra_r * LD + ((c ^ ((fra_r >> 1) & 7)) << 1) + lo;
        ob[j] = frb_r * LD + ((c ^ ((frb_r >> 1) & 7)) << 1) + lo;  // row + 16 has the same key
    }
    double2 ra0, ra1, ra2, ra3, ra4, ra5, rb0, rb1, rb2, rb3, rb4, rb5;  // (named: an indexed array of them was placed in scratch)
    double fra[2], frb[2][2];
    const int nst = (kend - kbeg + KS - 1) / KS, last = nst - 1;
#define GL6(K, ST) { const int st_ = min((ST), last) * KS; ra##K = *(const double2 *)(Ag + st_); rb##K = *(const double2 *)(Bg + st_); }
#define LS6(K, BUF) { *(double2 *)(As + (BUF) * ASZ + ll) = ra##K; *(double2 *)(Bs + (BUF) * BSZ + ll) = rb##K; }
#define RDF6(SL, BUF, J) { frb[SL][0] = Bs[(BUF) * BSZ + ob[J]]; frb[SL][1] = Bs[(BUF) * BSZ + ob[J] + 16 * LD]; fra[SL] = As[(BUF) * ASZ + oa[J]]; }
#define STAGE6(K, DO_LD, SLD)                                                                    \
    {                                                                                            \
        __syncthreads();                                                                         \
        _Pragma("unroll") for (int j = 0; j < NJ; j++) {                                         \
            const int sl = j & 1;                                                                \
            if (j < NJ - 1) RDF6(sl ^ 1, cur, j + 1) else RDF6(sl ^ 1, nxt, 0)                   \
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][0], acc[0], 0, 0, 0); \
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fra[sl], frb[sl][1], acc[1], 0, 0, 0); \
            if (j == 0) LS6(K, stb)                                                              \
            if (DO_LD) { if (j == 2) GL6(K, SLD) }                                               \
            __builtin_amdgcn_sched_barrier(0);                                                   \
        }                                                                                        \
        const int t_ = cur; cur = nxt; nxt = stb; stb = t_;                                      \
    }
    int cur = 0, nxt = 1, stb = 2, s = 0;
    if constexpr (NSET == 6) {
    GL6(0, 0) GL6(1, 1)
    __builtin_amdgcn_sched_barrier(0);
    GL6(2, 2) GL6(3, 3) GL6(4, 4) GL6(5, 5)
    __builtin_amdgcn_sched_barrier(0);
    LS6(0, 0)
    GL6(0, 6)
    __builtin_amdgcn_sched_barrier(0);
    LS6(1, 1)
    GL6(1, 7)
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
    RDF6(0, 0, 0)
    for (; s + NSET <= nst; s += NSET) {
        STAGE6(2, 1, s + 8)
        STAGE6(3, 1, s + 9)
        STAGE6(4, 1, s + 10)
        STAGE6(5, 1, s + 11)
        STAGE6(0, 1, s + 12)
        STAGE6(1, 1, s + 13)
    }
    {
        const int rem = nst - s;  // at most five stages left: stores only
        if (rem > 0) STAGE6(2, 0, 0)
        if (rem > 1) STAGE6(3, 0, 0)
        if (rem > 2) STAGE6(4, 0, 0)
        if (rem > 3) STAGE6(5, 0, 0)
        if (rem > 4) STAGE6(0, 0, 0)
    }
    } else {
    // three sets: at the top of stage s the LDS holds s and s + 1, the sets s + 2, s + 3, s + 4
    GL6(0, 0) GL6(1, 1) GL6(2, 2)
    __builtin_amdgcn_sched_barrier(0);
    LS6(0, 0)
    GL6(0, 3)
    __builtin_amdgcn_sched_barrier(0);
    LS6(1, 1)
    GL6(1, 4)
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (g.stamps) t_pro = (long long)__builtin_amdgcn_s_memtime();
    RDF6(0, 0, 0)
    for (; s + 3 <= nst; s += 3) {
        STAGE6(2, 1, s + 5)
        STAGE6(0, 1, s + 6)
        STAGE6(1, 1, s + 7)
    }
    {
        const int rem = nst - s;  // at most two stages left: stores only
        if (rem > 0) STAGE6(2, 0, 0)
        if (rem > 1) STAGE6(0, 0, 0)
    }
    }
#undef GL6
#undef LS6
#undef RDF6
#undef STAGE6
    const long long t_loop = g.stamps ? (long long)__builtin_amdgcn_s_memtime() : 0;
    // epilogues, as in gemm_tile_body (C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg)
    double esum = 0.0;
    {
        double rsq[4] = {0, 0, 0, 0};
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
            const int col = col0 + wc * 32 + tn * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = row0 + wr * 16 + (lane >> 4) + 4 * r;
                const double v = acc[tn][r];
                if (EPI == EPI_STORE || (EPI == EPI_WCOV && !second)) {
                    if (row < p.M && col < p.N) p.C[(size_t)row * p.ldc + col] = v;
                } else if (EPI == EPI_KERNEL) {
                    const bool same = e_rs[r] == e_cs[tn];
                    const bool rl = e_rn[r] == 0, cl = e_cn[tn] == 0;
                    KERNEL_VALUE(k, kp, v, rl, cl, g.ieta, p)
                    if (same && row < p.M && col < p.N) {
                        p.C[(size_t)row * p.ldc + col] = k;
                        if (p.Aw) p.Aw[(size_t)row * p.ldc + col] = e_mu[tn] * kp;
                        esum += k * e_mu[tn];
                    }
                } else {  // EPI_ROWSQ
                    if (col < p.N) rsq[r] += v * v;
                }
            }
        }
        if (EPI == EPI_ROWSQ || (EPI == EPI_WCOV && second)) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double sq = row_sum16(rsq[r]);
                const int row = row0 + wr * 16 + (lane >> 4) + 4 * r;
                if ((lane & 15) == 0 && row < p.M && sq != 0.0) p.rowsq[(size_t)row * p.rowsq_ld + 2 * ct + wc] = sq;
            }
        }
    }
    if (EPI == EPI_KERNEL && g.Epart) {
        esum = wave_sum64(esum);
        if (lane == 0) g.Epart[(size_t)bid * 8 + wave] = esum;
    }
    if (g.stamps && threadIdx.x == 0)
        stamp_record(g.stamps + (size_t)bid * 8, t_start, t_entry, t_pro, t_loop, (long long)(kend - kbeg) | ((long long)second << 20));
}
