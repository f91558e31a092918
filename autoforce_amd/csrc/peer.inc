// peer.inc — the library's own exchange between the ranks of one node, and what consumes it (included by api.hip).
//
// The reference combines the ranks' partial sums with four MPI all-reduces per step (calculator/active.py:562, :600-602,
// :770-777: energy, forces, cell gradient, the zero-padded covloss — an all-reduce of zero-padded arrays IS an
// all-gather; util/parallel.py, _mpi4py.py:47-56).  Here every rank PUSHES its packed partial sums into a slice of every
// peer's receive buffer (hipIpc-mapped device memory: posted writes, one hop on the fully connected xGMI mesh), releases
// them with one flag store per peer, and sums the `world` slices locally IN RANK ORDER: every rank gets the same bits
// whatever the arrival order (RCCL's reduction order is its own business).  Processes that share ONE device can be peers
// too — RCCL refuses that — so the multi-rank path runs on a one-GPU test box.
//
// Exchange layout of a sharded step (`xp`, 3N + 4C + 11 words with C = ceil(N / world), peer_xlen):
//   [0, 3N)            the fixed-point force sums of the scatter-form reverse pass, as 64-bit INTEGERS (SGPR_FIX_SCALE),
//                      caller atom order: every rank contributes to every atom
//   [3N, 3N + 3C)      the own part of the forces of THIS rank's atoms, in the rank's own order: its il-th atom is the sorted
//                      atom rank + il * world (sharding.py), so a consumer finds atom i in slice i % world at il = i / world
//   [3N + 3C, + C)     covloss of this rank's atoms, same order
//   [3N + 4C, + 11)    energy, virial (9), overflow word
// (Round 6: the own part and the covloss travelled as N-long arrays that are zero outside the rank's share — the reference's
// all-reduces of zero-padded arrays, calculator/active.py:600-602, :770-777, word for word; 7N + 11 words per peer instead of
// 3N + 4N / world + 11: at world 8 half the bytes on every link and in every consumer.)
// The integer part is summed as integers, the rest has exactly one source per entry (energy and virial aside): the total
// force on an atom is the same bits for every number of ranks, so a trajectory does not depend on how it was sharded.
//
// Two epochs' parities: rank A may push exchange e + 1 while rank B still reads exchange e; it cannot push e + 2 before it
// has seen B's flag of e + 1, which B sets after its own sum of e (stream order).

struct PeerPtrs { double *recv[SGPR_PEER_MAX]; int *flag[SGPR_PEER_MAX]; };
static inline size_t peer_cmax(int N, int world) { return ((size_t)std::max(N, 0) + std::max(world, 1) - 1) / std::max(world, 1); }
static inline size_t peer_xlen(int N, int world) { return 3 * (size_t)N + 4 * peer_cmax(N, world) + 11; }
#define SGPR_PEER_CTL_ERR (SGPR_PEER_MAX * 32)
#define SGPR_PEER_CTL_DEAD ((SGPR_PEER_MAX + 1) * 32)

// grid (chunks, world): this rank's `len` words into slice `rank` of peer blockIdx.y; the last workgroup of a peer
// releases the slice with the epoch in that peer's flag of this rank
__global__ __launch_bounds__(256) void peer_push_kernel(PeerPtrs p, const double *src, size_t len, size_t cap, int rank, int world,
                                                        int parity, int epoch, int *ctl, const int *halt, int step)
{
    if (halt && *halt < step) return;   // (an MD run that has halted: every rank skips alike, api.hip::sgpr_md_run)
    const int peer = blockIdx.y, nb = gridDim.x;
    double *d1 = p.recv[peer] + ((size_t)parity * world + rank) * cap;
    if (((uintptr_t)src & 15) == 0) {   // (slices are 16-byte aligned; a caller's buffer of sgpr_comm_allreduce need not be)
        double2 *dst = (double2 *)d1;
        const double2 *s2 = (const double2 *)src;
        const size_t n2 = len / 2;      // whole pairs only: the source may END on an odd word
        for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n2; k += (size_t)nb * 256) dst[k] = s2[k];
        if ((len & 1) && blockIdx.x == 0 && threadIdx.x == 0) d1[len - 1] = src[len - 1];
    } else {
        for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < len; k += (size_t)nb * 256) d1[k] = src[k];
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        int *c = ctl + peer * 32;
        if (atomicAdd(c, 1) == nb - 1) {
            *c = 0;
            __threadfence_system();
            __hip_atomic_store(p.flag[peer] + rank * 32, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ONE wave: lane r waits for the flag of source rank r.  A separate launch (not a poll at the top of the consumer): on a
// box where the peers share one device a grid of spinning workgroups would starve the very kernels it waits for.
// Bounded: a peer that never arrives is an error word for the host, not a hang.
__global__ void peer_wait_kernel(const int *flag, int world, int epoch, int *ctl, long long max_ticks, const int *halt, int step)
{
    if (halt && *halt < step) return;
    const int lane = threadIdx.x;
    if (lane >= world) return;
    if (__hip_atomic_load(ctl + SGPR_PEER_CTL_DEAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const long long t0 = wall_clock64();
    while ((int)(__hip_atomic_load(flag + lane * 32, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0) {
        if (wall_clock64() - t0 > max_ticks) {
            atomicMax(ctl + SGPR_PEER_CTL_ERR, lane + 1);
            __hip_atomic_store(ctl + SGPR_PEER_CTL_DEAD, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(4);
    }
}

// totals of a sharded step in the packed layout of sgpr_step_dev ([F 3N | beta N | E | virial 9 | overflow]) from the
// `n` slices of the exchange layout
struct ShardSrc { const double *base; int n; size_t stride; const int *ctl; int cmax; /* C of the layout; n slices = the sharding's world */ };

// (`ctl`: the exchange's control words, or null for a single slice.  A wait that gave up leaves the slices of an EARLIER
// exchange behind: the consumer then puts the poison value into the overflow word, so that the host — which reads this word
// after every step — cannot take the stale sums for results.)
// (`iperm`: caller atom -> sorted index: the owner of sorted atom i is rank i % world, where it is the (i / world)-th atom)
__global__ __launch_bounds__(256) void peer_sum_xp_kernel(ShardSrc s, int N, double *out, const int *ctl, const int *iperm)
{
    const size_t tot = 4 * (size_t)N + 11, n3 = 3 * (size_t)N, n4 = 4 * (size_t)N;
    const size_t own0 = n3, beta0 = n3 + 3 * (size_t)s.cmax, scal0 = n3 + 4 * (size_t)s.cmax;
    const bool dead = ctl && __hip_atomic_load(ctl + SGPR_PEER_CTL_DEAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
        if (e < n4) {
            const int c = e < n3 ? (int)(e / 3) : (int)(e - n3), k = e < n3 ? (int)(e % 3) : 0;
            const int i = iperm[c];
            const double *po = s.base + (size_t)(i % s.n) * s.stride;
            const size_t il = (size_t)(i / s.n);
            if (e < n3) {
                long long fx = 0;
                for (int r = 0; r < s.n; r++) fx += ((const long long *)(s.base + r * s.stride))[e];
                out[e] = (double)fx * (1.0 / SGPR_FIX_SCALE) + po[own0 + 3 * il + k];
            } else
                out[e] = po[beta0 + il];
        } else {
            double v = 0.0;
            for (int r = 0; r < s.n; r++) v += s.base[r * s.stride + scal0 + (e - n4)];
            out[e] = (dead && e == tot - 1) ? SGPR_PEER_POISON : v;
        }
    }
}

// plain buffers (sgpr_comm_allreduce): SUM or MAX over the slices, rank order
// (a wait that gave up: NaN everywhere — there is no status word in a caller's buffer, and a stale sum must not pass for one)
__global__ __launch_bounds__(256) void peer_sum_kernel(ShardSrc s, size_t len, int op_max, double *out, const int *ctl)
{
    const bool dead = ctl && __hip_atomic_load(ctl + SGPR_PEER_CTL_DEAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (size_t)gridDim.x * 256) {
        double v = s.base[e];
        for (int r = 1; r < s.n; r++) {
            const double w = s.base[r * s.stride + e];
            v = op_max ? fmax(v, w) : v + w;
        }
        out[e] = dead ? __longlong_as_double(0x7ff8000000000000ll) : v;
    }
}

// The consumer of a sharded step that also OPENS THE NEXT ONE (the sharded counterpart of finalize_next_kernel): thread =
// (sorted atom, component | covloss).  It sums the slices (totals out in the packed layout, caller order), takes the atom
// to its next position — MODE 1: read from the next resident frame; MODE 2: integrated from the TOTAL force, every rank
// integrating every atom: after the exchange every rank holds the same bits, the deviates are counter-based or uploaded
// alike, so the ranks' states stay identical without ever being compared —, bins it, takes part in the rebuild decision
// and clears the accumulators of the next step's reverse pass.  MODE 4: MODE 2 with held components (FinNext::fixed), the
// rules of finalize_next_kernel<4>.  Grid: ceil(N / 64) + 2 lagged reducers (MODE 2) + 1
// workgroup for the eleven scalars.
template <int MODE>
__global__ __launch_bounds__(256) void shard_next_kernel(FinArgs f, ShardSrc s)
{
    const FinNext &x = f.nx;
    constexpr bool MD = MODE >= 2;   // the integrator (MODE 4: with held components, as finalize_next_kernel<4>)
    const int tid = threadIdx.x, b = blockIdx.x, nA = gridDim.x - 3;
    const int N = f.N;
    const int halt_w = MD ? *x.halt : 0x7fffffff;
    if (halt_w < x.step) return;
    if (b >= nA) {
        const int q = b - nA;
        if (q < 2) {
            if (MD && x.packed_prev) finalize_reduce_prev(f, q);
            return;
        }
        if (tid < 11) {
            double v = 0.0;
            for (int r = 0; r < s.n; r++) v += s.base[r * s.stride + 3 * (size_t)N + 4 * (size_t)s.cmax + tid];
            // a wait of this exchange that gave up: the slices are an earlier exchange's — the step is void (poison in the
            // overflow word: the MD loop halts on it, the host's sgpr_md_run / sgpr_compute report the time-out)
            if (tid == 10 && s.ctl && __hip_atomic_load(s.ctl + SGPR_PEER_CTL_DEAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) v = SGPR_PEER_POISON;
            f.packed[4 * (size_t)N + tid] = v;
            if (MD) {
                x.scal_cur[tid] = tid == 10 ? (v != 0.0 ? 1.0 : 0.0) : v;
                if (tid == 10) {
                    *x.mark_cur = 1;
                    if (v != 0.0) {   // some rank's lists were clamped: the step is void on every rank alike
                        atomicMin(&x.halt[0], x.step);
                        x.halt_host[1] = x.step;
                    }
                }
            }
        }
        return;
    }
    const int s1 = x.step + 1;
    if (b == 0 && tid == 0) {
        if (x.force) atomicMax(&x.flags[s1 & 3], 1);
        x.flags[(s1 + 2) & 3] = 0;
        fin_cell_guard(f, *f.flag, s1);
    }
    const int i = b * 64 + (tid >> 2), k = tid & 3;
    const bool act = i < N;
    const int ia = act ? i : 0, kk = k < 3 ? k : 2;
    // ---- requests
    const int c = f.perm[ia];
    const NlGrid g = *f.grid;
    const int slot_i = f.slot[ia];
    const double p0 = f.pos0[3 * (size_t)ia + kk];
    double xc = 0.0, vc = 0.0, ms = 1.0, sg = 0.0, nz = 0.0, xn = 0.0;
    const bool held = MODE == 4 ? x.fixed[3 * (size_t)ia + kk] != 0 : false;
    if (MD) {
        xc = x.x_cur[3 * (size_t)ia + kk];
        vc = x.v_cur[3 * (size_t)ia + kk];
        ms = x.mass[ia];
        sg = x.sig[ia];
        nz = x.noise ? x.noise[3 * (size_t)ia + kk] : 0.0;
    }
    double xpv = 0.0, zeta = 0.0;
    if (MD && x.nh) { xpv = x.x_prev[3 * (size_t)ia + kk]; zeta = *x.nh_zeta; }
    if (MODE == 1) xn = x.pos_in[3 * (size_t)c + kk];
    // the totals: lanes 0..2 a force component (integer part summed over the ranks + the owner's own part), lane 3 the covloss
    // (the owner's): sorted atom i belongs to rank i % world, where it is atom i / world
    const size_t e1 = 3 * (size_t)c + kk;
    const double *po = s.base + (size_t)(ia % s.n) * s.stride;
    const size_t il_o = (size_t)(ia / s.n);
    const double own = po[k < 3 ? 3 * (size_t)N + 3 * il_o + k : 3 * (size_t)N + 3 * (size_t)s.cmax + il_o];
    long long acc_i = 0;
    for (int r = 0; r < s.n; r++) acc_i += ((const long long *)(s.base + r * s.stride))[e1];
    const double tot = k < 3 ? (double)acc_i * (1.0 / SGPR_FIX_SCALE) + own : own;
    if (!act) return;
    if (k < 3) {
        f.packed[3 * (size_t)c + k] = tot;
        ((long long *)f.Fnbr)[3 * (size_t)i + k] = 0;     // (the stand-alone binning kernel clears these)
    } else {
        f.packed[3 * (size_t)N + c] = tot;
        const int il = (i - f.first) / f.stride;
        if (f.has_beta && i >= f.first && (i - f.first) % f.stride == 0 && il < f.cnt)
            for (int j = 0; j < f.csq_slots; j++) x.csq_rw[(size_t)il * f.csq_slots + j] = 0.0;
    }
    // ---- the next step
    double ke = 0.0, kp = 0.0, v3 = 0.0;
    if (MD && x.nh) {
        if (k < 3) {
            const double vnow = md_nh_advance(x, held, tot, ms, xc, vc, xpv, zeta, xn);
            ke = ms * (vnow * vnow);
            kp = ke;
            x.v_now[3 * (size_t)i + k] = vnow;
        }
    } else if (MD && k < 3)
        xn = md_baoab_advance(x, held, tot, ms, sg, nz, xc, vc, c, k, v3, ke, kp);
    // the quad's three components
    const double X = fin_quad_lane<0>(xn), Y = fin_quad_lane<1>(xn), Z = fin_quad_lane<2>(xn);
    if (MD) {
        fin_store_ke(ke, kp, k == 0, x.ke_cur, i);
        if (k < 3) {
            x.x_next[3 * (size_t)i + k] = xn;
            if (!x.nh) x.v_next[3 * (size_t)i + k] = v3;
        }
    }
    if (k < 3) x.pos[3 * (size_t)i + k] = xn;
    const double dd = k < 3 ? xn - p0 : 0.0;
    const double d0 = fin_quad_lane<0>(dd), d1 = fin_quad_lane<1>(dd), d2v = fin_quad_lane<2>(dd);
    if (k != 0) return;
    const double d2 = d0 * d0 + d1 * d1 + d2v * d2v;
    int bidx[3], w[3];
#pragma unroll
    for (int a = 0; a < 3; a++) bidx[a] = nl_place_axis(g, a, x.pbc[a], X, Y, Z, w[a]);
    const int bin = nl_bin_index(g, bidx);
    int kb = -1;
    if (slot_i < x.S) kb = atomicAdd(&x.bc_next[(size_t)bin * SGPR_BIN_STRIDE], 1);
    if (!(d2 <= x.thr2)) atomicMax(&x.flags[s1 & 3], 1);
    x.bin_of[i] = bin;
    x.kslot[i] = kb;
    if (slot_i < x.S) nl_store_rec(x.b_rec, x.b_aux, x.cap, f.stat, bin, kb, X, Y, Z, i, w, slot_i);
}

// ---------------------------------------------------------------------------- host side
static bool peer_on(const sgpr_model *h) { return h->peer.attached && h->peer.world > 1; }

static PeerPtrs peer_ptrs(const PeerXchg &x)
{
    PeerPtrs p = {};
    for (int r = 0; r < x.world; r++) {
        p.recv[r] = (double *)x.peer_base[r];
        p.flag[r] = (int *)(x.peer_base[r] + x.flag_off);
    }
    return p;
}

// push `len` words of `src` to every rank and wait for everybody's: afterwards slice r of parity (*parity_out) holds
// rank r's words.  halt / step: the halt word of an MD run (a halted run skips its exchanges on every rank alike).
static int peer_exchange(sgpr_model *h, const double *src, size_t len, hipStream_t st, int *parity_out, const int *halt = nullptr,
                         int step = 0)
{
    PeerXchg &x = h->peer;
    if (len > x.cap)
        return fail(SGPR_E_INVALID, "the exchange buffers hold %zu doubles per rank, this step needs %zu: export and attach again "
                    "(sgpr_peer_export) with a larger capacity", x.cap, len);
    if (x.any_st && x.last_st != st) {   // (a caller-supplied stream after the handle's own, or the other way round)
        if (!x.ev && hipEventCreateWithFlags(&x.ev, hipEventDisableTiming) != hipSuccess) { x.ev = nullptr; return fail(SGPR_E_NODEVICE, "hipEventCreate failed"); }
        if (hipEventRecord(x.ev, x.last_st) == hipSuccess) HIPCHK(hipStreamWaitEvent(st, x.ev, 0));
        else (void)hipGetLastError();     // (the earlier stream no longer exists: nothing of it can still be running)
    }
    x.last_st = st; x.any_st = true;
    const int epoch = (int)++x.epoch, parity = epoch & 1;
    static const bool trace = getenv("SGPR_PEER_TRACE") != nullptr;   // diagnostic: the sequence of exchanges of every rank on stderr
    if (trace) fprintf(stderr, "[sgpr peer] rank %d epoch %d len %zu step %d %s\n", x.rank, epoch, len, step, halt ? "md" : "plain");
    const int nb = (int)std::min<size_t>(16, std::max<size_t>(1, (len / 2 + 2047) / 2048));
    hipLaunchKernelGGL(peer_push_kernel, dim3(nb, x.world), dim3(256), 0, st, peer_ptrs(x), src, len, x.cap, x.rank, x.world, parity, epoch,
                       x.ctl.p, halt, step);
    hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, st, (const int *)(x.base + x.flag_off), x.world, epoch, x.ctl.p,
                       x.timeout_ticks, halt, step);
    *parity_out = parity;
    return SGPR_OK;
}

static ShardSrc peer_src(const PeerXchg &x, int parity)
{
    ShardSrc s;
    s.base = x.slice(parity, 0); s.n = x.world; s.stride = x.cap; s.ctl = x.ctl.p; s.cmax = 0;   // (cmax: the caller, who knows N)
    return s;
}

// after a synchronisation: did a wait of this handle give up?
static int peer_check(sgpr_model *h)
{
    if (!h->peer.attached || !h->peer.ctl.p) return SGPR_OK;
    int err = 0;
    HIPCHK(hipMemcpy(&err, h->peer.ctl.p + SGPR_PEER_CTL_ERR, sizeof(int), hipMemcpyDeviceToHost));
    if (err)
        return fail(SGPR_E_NODEVICE, "the exchange between the ranks timed out waiting for rank %d (of %d; this is rank %d): that process "
                    "has failed or left the step; results since are invalid", err - 1, h->peer.world, h->peer.rank);
    return SGPR_OK;
}

/* handle blob: [0, 64) hipIpcMemHandle_t | [64] capacity (int64) | [72] world, rank, pid (int32 x 3) | [88] own base address
 * (uint64: ranks that live in ONE process — several handles, threads — use the pointer itself) */
extern "C" int sgpr_peer_export(sgpr_model *h, int rank, int world, int64_t capacity, void *handle_out)
{
    if (!h || !handle_out || world < 1 || world > SGPR_PEER_MAX || rank < 0 || rank >= world || capacity < 1)
        return fail(SGPR_E_INVALID, "sgpr_peer_export: bad arguments (world <= %d)", SGPR_PEER_MAX);
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "hipIpcMemHandle_t size");
    HIPCHK(hipSetDevice(h->device));
    const int rd = sgpr_peer_destroy(h);
    if (rd) return rd;
    PeerXchg &x = h->peer;
    x.world = world; x.rank = rank;
    x.cap = ((size_t)capacity + 15) / 16 * 16;
    x.flag_off = (sizeof(double) * 2 * world * x.cap + 255) / 256 * 256;
    x.bytes = x.flag_off + sizeof(int) * 32 * SGPR_PEER_MAX;
    // fine-grained device memory: peers' stores and this device's loads meet at the memory side, not in a stale L2 line
    if (hipExtMallocWithFlags((void **)&x.base, x.bytes, hipDeviceMallocFinegrained) != hipSuccess) {
        x.base = nullptr;
        return fail(SGPR_E_NODEVICE, "sgpr_peer_export: no device memory for the exchange buffers (%zu bytes)", x.bytes);
    }
    HIPCHK(hipMemset(x.base, 0, x.bytes));
    if (x.ctl.alloc((SGPR_PEER_MAX + 2) * 32)) return fail(SGPR_E_NODEVICE, "sgpr_peer_export: device allocation failed");
    HIPCHK(hipDeviceSynchronize());
    if (const char *e = getenv("SGPR_PEER_TIMEOUT_MS")) x.timeout_ticks = std::max(1LL, atoll(e)) * 100000LL;
    unsigned char *o = (unsigned char *)handle_out;
    memset(o, 0, SGPR_PEER_HANDLE_BYTES);
    hipIpcMemHandle_t hnd;
    const hipError_t e = hipIpcGetMemHandle(&hnd, x.base);
    if (e != hipSuccess) {
        (void)sgpr_peer_destroy(h);
        return fail(SGPR_E_NODEVICE, "hipIpcGetMemHandle: %s (is HSA_ENABLE_IPC_MODE_LEGACY=0 exported?)", hipGetErrorString(e));
    }
    memcpy(o, &hnd, sizeof(hnd));
    const int64_t cap64 = (int64_t)x.cap;
    const int32_t meta[3] = {world, rank, (int32_t)getpid()};
    const uint64_t addr = (uint64_t)(uintptr_t)x.base;
    memcpy(o + 64, &cap64, 8);
    memcpy(o + 72, meta, 12);
    memcpy(o + 88, &addr, 8);
    return SGPR_OK;
}

extern "C" int sgpr_peer_attach(sgpr_model *h, const void *handles)
{
    if (!h || !handles) return fail(SGPR_E_INVALID, "sgpr_peer_attach: bad arguments");
    PeerXchg &x = h->peer;
    if (!x.base) return fail(SGPR_E_INVALID, "sgpr_peer_attach: call sgpr_peer_export first");
    HIPCHK(hipSetDevice(h->device));
    const unsigned char *in = (const unsigned char *)handles;
    for (int r = 0; r < x.world; r++) {
        const unsigned char *o = in + (size_t)r * SGPR_PEER_HANDLE_BYTES;
        int64_t cap64;
        int32_t meta[3];
        uint64_t addr;
        memcpy(&cap64, o + 64, 8);
        memcpy(meta, o + 72, 12);
        memcpy(&addr, o + 88, 8);
        if (meta[0] != x.world || meta[1] != r || (size_t)cap64 != x.cap) {
            (void)sgpr_peer_destroy(h);
            return fail(SGPR_E_INVALID, "sgpr_peer_attach: handle %d is of rank %d of %d with capacity %lld, expected rank %d of %d "
                        "with %zu", r, meta[1], meta[0], (long long)cap64, r, x.world, x.cap);
        }
        if (r == x.rank) { x.peer_base[r] = x.base; continue; }
        if (meta[2] == (int32_t)getpid()) { x.peer_base[r] = (char *)(uintptr_t)addr; continue; }   // a rank of this very process
        hipIpcMemHandle_t hnd;
        memcpy(&hnd, o, sizeof(hnd));
        void *p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, hnd, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)sgpr_peer_destroy(h);
            return fail(SGPR_E_NODEVICE, "hipIpcOpenMemHandle (rank %d): %s", r, hipGetErrorString(e));
        }
        x.peer_base[r] = (char *)p;
        x.opened[r] = true;
    }
    x.attached = true;
    x.epoch = 0;
    drop_graph(h);
    return SGPR_OK;
}

extern "C" int sgpr_peer_destroy(sgpr_model *h)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_peer_destroy: bad arguments");
    PeerXchg &x = h->peer;
    if (x.base || x.attached) {
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (int r = 0; r < SGPR_PEER_MAX; r++) {
            if (x.opened[r] && x.peer_base[r]) (void)hipIpcCloseMemHandle(x.peer_base[r]);
            x.opened[r] = false;
            x.peer_base[r] = nullptr;
        }
        if (x.base) (void)hipFree(x.base);
        x.base = nullptr;
        if (x.ev) (void)hipEventDestroy(x.ev);
        x.ev = nullptr; x.any_st = false; x.last_st = nullptr;
        x.ctl.release();
    }
    x.attached = false;
    x.world = 1; x.rank = 0; x.cap = 0; x.epoch = 0;
    return SGPR_OK;
}
