// data.inc — included at the end of api.hip: the RESIDENT training set.
//
// The reference keeps the design matrix of the regression, K = [K_e; K_f; K_v] (one energy row, 3N force rows
// and 6 virial rows per stored frame, regression/gppotential.py:484-509), as torch tensors next to the model and
// edits it in step with the data (`add_data` :730-743, `pop_1data` :793-813) and with the inducing set
// (`add_inducing` :745-772 appends a column, `pop_1inducing` :782-791 drops one).  Every edit is followed by
// `make_munu` (:548-605).  Here the matrix lives in HBM for the life of the model: frames are pushed once
// (their rows are computed on the device and never leave it), the inducing-set entry points keep the columns
// in step, and sgpr_data_solve factors it where it lies.  A 16384-atom frame at m = 1024 is 0.4 GB — three
// orders of magnitude below the 288 GB of one MI355X — so nothing is ever recomputed or moved over PCIe except
// the targets (one double per row) and K·v products (one double per row).
//
// Layout: column-major in the CALLER's column order, design[c * rcap + r]: appending an inducing LCE appends a
// column, popping the last one is free, and the QR's transposed work array is a strided copy.  Rows are
// frame-major: frame f owns [row0, row0 + 1 + 3N + nv): its energy row, its 3N force rows, its nv (0 or 6)
// virial rows (Voigt order xx yy zz yz xz xy, regression/gppotential.py:76-83).

// design[(q_first + c) * rcap + row0 + ...] <- packed rows of column c (rows_compute)
__global__ void design_store_kernel(int N, int nv, int q_first, const double *rows, size_t rowlen, const double *ke,
                                    const int *cols, double *design, size_t rcap, size_t row0)
{
    const int c = blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int nrows = 1 + 3 * N + nv;
    if (r >= nrows) return;
    const double *src = rows + rowlen * c;
    double v;
    if (r == 0)
        v = ke[cols[c]];
    else if (r <= 3 * N)
        v = src[r - 1];
    else {
        const int voigt[6] = {0, 4, 8, 5, 2, 1};
        v = src[4 * (size_t)N + 1 + voigt[r - 1 - 3 * N]];
    }
    design[(size_t)(q_first + c) * rcap + row0 + r] = v;
}

// At[k][r] = design[k][r] (energy rows zeroed on request), At[m][r] = Y[r]
__global__ void design_to_qr_kernel(int64_t rows, int m, const double *design, size_t rcap,
                                    const double *Y, const unsigned char *is_e, int with_energies, double *At, int ldr)
{
    const int k = blockIdx.y;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const bool drop = !with_energies && is_e[r];
        const double v = k < m ? design[(size_t)k * rcap + r] : Y[r];
        At[(size_t)k * ldr + r] = drop ? 0.0 : v;
    }
}

// out[r] = sum_c design[c][r] v[c]: lanes along the rows (coalesced), columns in a fixed order
__global__ __launch_bounds__(256) void design_matvec_kernel(int64_t rows, int m, const double *design, size_t rcap,
                                                            const double *v, double *out)
{
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = 0;
    for (; c + 4 <= m; c += 4) {
        s0 += design[(size_t)c * rcap + r] * v[c];
        s1 += design[(size_t)(c + 1) * rcap + r] * v[c + 1];
        s2 += design[(size_t)(c + 2) * rcap + r] * v[c + 2];
        s3 += design[(size_t)(c + 3) * rcap + r] * v[c + 3];
    }
    for (; c < m; c++) s0 += design[(size_t)c * rcap + r] * v[c];
    out[r] = (s0 + s1) + (s2 + s3);
}

// dst[c'][r] = src[idx[c']][r]
__global__ void design_gather_kernel(int64_t rows, const double *src, size_t rcap_s, const int *idx, double *dst,
                                     size_t rcap_d)
{
    const int c = blockIdx.y;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x)
        dst[(size_t)c * rcap_d + r] = src[(size_t)idx[c] * rcap_s + r];
}

// capacity for `rows` x `cols`; the content ([design_rows] x [keep_cols]) moves if the buffer is replaced
static int design_reserve(sgpr_model *h, int64_t rows, int64_t cols, int64_t keep_cols)
{
    if (rows <= h->design_rcap && cols <= h->design_ccap && h->d_design.p) return SGPR_OK;
    const int64_t rcap = rows > h->design_rcap ? ((rows + rows / 2 + 63) / 64 * 64) : h->design_rcap;
    const int64_t ccap = cols > h->design_ccap ? ((cols + cols / 2 + 32 + 31) / 32 * 32) : h->design_ccap;
    DevBuf<double> nb;
    // (the second buffer of the selection pair has the OLD capacity: useless after this growth, and the first thing to give
    // back when memory is short — it is allocated again by the next selection)
    h->d_design_alt.release();
    if (nb.alloc((size_t)rcap * ccap, false)) {
        h->d_rows_bG.release();   // ... then the hand-over buffer of the sixteen-column rows form (re-sized on its next use)
        if (nb.alloc((size_t)rcap * ccap, false))
            return fail(SGPR_E_NODEVICE, "hipMalloc failed (resident design matrix, %lld x %lld)", (long long)rcap, (long long)ccap);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_design.p && h->design_rows > 0 && keep_cols > 0)
        HIPCHK(hipMemcpy2D(nb.p, sizeof(double) * rcap, h->d_design.p, sizeof(double) * h->design_rcap,
                           sizeof(double) * h->design_rows, keep_cols, hipMemcpyDeviceToDevice));
    h->d_design = std::move(nb);
    h->design_rcap = rcap;
    h->design_ccap = ccap;
    return SGPR_OK;
}

// columns [q_first, q_first + q_count) of frame f: rows on the device, scattered into the matrix
static int design_fill(sgpr_model *h, int f, int q_first, int q_count)
{
    if (q_count <= 0) return SGPR_OK;
    const sgpr_model::DataFrame &fr = h->frames[f];
    const int rc_ = rows_compute(h, fr.N, fr.numbers.data(), fr.pos.data(), fr.cell, fr.pbc, q_first, q_count);
    if (rc_) return rc_;
    const int nrows = 1 + 3 * fr.N + fr.nv;
    hipLaunchKernelGGL(design_store_kernel, dim3((nrows + 255) / 256, q_count), dim3(256), 0, h->stream, fr.N, fr.nv, q_first,
                       h->d_rows_out.p, (size_t)4 * fr.N + 11, h->d_rows_ke.p, h->d_rows_cols.p, h->d_design.p,
                       (size_t)h->design_rcap, (size_t)fr.row0);
    HIPCHK(hipStreamSynchronize(h->stream));  // the scratch rows are reused by the next call
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

// every column of every frame (after sgpr_set_inducing replaced the set)
static int design_rebuild(sgpr_model *h)
{
    if (h->frames.empty() || h->m <= 0) return SGPR_OK;
    int rc_ = design_reserve(h, h->design_rows, h->m, 0);
    for (size_t f = 0; f < h->frames.size() && !rc_; f++) rc_ = design_fill(h, (int)f, 0, h->m);
    if (!rc_) HIPCHK(hipStreamSynchronize(h->stream));
    return rc_;
}

// hooks of the inducing-set entry points ------------------------------------------------------
static int design_after_set(sgpr_model *h)
{
    if (h->design_hold) return SGPR_OK;
    h->col_ids.resize(h->m);
    for (auto &id : h->col_ids) id = h->next_id++;
    return design_rebuild(h);
}

static void design_after_pop_last(sgpr_model *h)
{
    if (!h->col_ids.empty()) h->col_ids.pop_back();
}

static int design_after_add(sgpr_model *h)
{
    h->col_ids.push_back(h->next_id++);
    if (h->frames.empty()) return SGPR_OK;
    int rc_ = design_reserve(h, h->design_rows, h->m, h->m - 1);
    for (size_t f = 0; f < h->frames.size() && !rc_; f++) rc_ = design_fill(h, (int)f, h->m - 1, 1);
    if (!rc_) HIPCHK(hipStreamSynchronize(h->stream));
    return rc_;
}

// keep columns idx[0..count) (old caller order) as the new columns 0..count
static int design_select(sgpr_model *h, int count, const int32_t *idx)
{
    {
        std::vector<int64_t> ids(std::max(count, 0));
        for (int c = 0; c < count; c++) ids[c] = idx[c] < (int)h->col_ids.size() ? h->col_ids[idx[c]] : h->next_id++;
        h->col_ids.swap(ids);
    }
    if (h->frames.empty() || !h->d_design.p || count <= 0) return SGPR_OK;
    bool prefix = true;
    for (int c = 0; c < count; c++) prefix = prefix && idx[c] == c;
    if (prefix) return SGPR_OK;  // dropping trailing columns: nothing moves
    // gathered into the second buffer of the pair, which then becomes the matrix (kept allocated: a downsize at
    // every update step would otherwise allocate and free gigabytes each time)
    DevBuf<double> &nb = h->d_design_alt;
    DevBuf<int> &d_idx = h->sc_sel_idx;
    if (nb.alloc((size_t)h->design_rcap * h->design_ccap, false)) {
        h->d_rows_bG.release();   // (memory is short: the rows form's hand-over buffer goes first, it is re-sized on its next use)
        if (nb.alloc((size_t)h->design_rcap * h->design_ccap, false))
            return fail(SGPR_E_NODEVICE, "hipMalloc failed (second buffer of the resident design matrix)");
    }
    if (d_idx.alloc(count, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (resident design matrix)");
    HIPCHK(hipMemcpy(d_idx.p, idx, sizeof(int) * count, hipMemcpyHostToDevice));
    const int gx = (int)std::min<int64_t>((h->design_rows + 255) / 256, 4096);
    hipLaunchKernelGGL(design_gather_kernel, dim3(std::max(gx, 1), count), dim3(256), 0, h->stream, h->design_rows, h->d_design.p,
                       (size_t)h->design_rcap, d_idx.p, nb.p, (size_t)h->design_rcap);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    std::swap(h->d_design, h->d_design_alt);
    return SGPR_OK;
}

// ---------------------------------------------------------------------------- entry points
extern "C" int sgpr_data_push(sgpr_model *h, int N, const int32_t *numbers, const double *positions, const double *cell,
                              const int32_t *pbc, int nv)
{
    if (!h || N <= 0 || !numbers || !positions || !cell || (nv != 0 && nv != 6))
        return fail(SGPR_E_INVALID, "sgpr_data_push: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    sgpr_model::DataFrame fr;
    fr.N = N; fr.nv = nv;
    fr.row0 = h->design_rows;
    fr.rows = 1 + 3 * (int64_t)N + nv;
    fr.numbers.assign(numbers, numbers + N);
    fr.pos.assign(positions, positions + 3 * (size_t)N);
    memcpy(fr.cell, cell, sizeof(fr.cell));
    for (int k = 0; k < 3; k++) fr.pbc[k] = pbc ? pbc[k] : 1;
    if (h->m > 0) {
        // validate before anything is committed (species, capacities): the rows are computed first
        h->frames.push_back(fr);
        int rc_ = design_reserve(h, h->design_rows + fr.rows, std::max(h->m, 1), h->m);
        if (!rc_) rc_ = design_fill(h, (int)h->frames.size() - 1, 0, h->m);
        if (!rc_ && hipStreamSynchronize(h->stream) != hipSuccess) rc_ = fail(SGPR_E_NODEVICE, "sgpr_data_push: device error");
        if (rc_) {
            h->frames.pop_back();
            return rc_;
        }
    } else {
        for (int i = 0; i < N; i++)
            if (slot_of(h, numbers[i]) < 0 && !h->ignore_unknown)
                return fail(SGPR_E_SPECIES, "sgpr_data_push: Z=%d is not in the species table", numbers[i]);
        h->frames.push_back(fr);  // no inducing LCE yet: the first sgpr_add_inducing computes its column
    }
    h->design_rows += fr.rows;
    h->frame_ids.push_back(h->next_id++);
    h->r1_valid = false;
    return SGPR_OK;
}

extern "C" int sgpr_data_pop(sgpr_model *h, int index)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_data_pop: bad arguments");
    const int n = (int)h->frames.size();
    if (index < 0) index += n;
    if (index < 0 || index >= n) return fail(SGPR_E_INVALID, "sgpr_data_pop: index outside [0, %d)", n);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t r0 = h->frames[index].row0, nr = h->frames[index].rows, tail = h->design_rows - (r0 + nr);
    if (tail > 0 && h->m > 0 && h->d_design.p) {
        // the rows behind the frame move up: through a new buffer (the ranges overlap), rare (popfirst_1data)
        DevBuf<double> nb;
        if (nb.alloc((size_t)h->design_rcap * h->design_ccap, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (resident design matrix)");
        if (r0 > 0)
            HIPCHK(hipMemcpy2D(nb.p, sizeof(double) * h->design_rcap, h->d_design.p, sizeof(double) * h->design_rcap,
                               sizeof(double) * r0, h->m, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy2D(nb.p + r0, sizeof(double) * h->design_rcap, h->d_design.p + r0 + nr, sizeof(double) * h->design_rcap,
                           sizeof(double) * tail, h->m, hipMemcpyDeviceToDevice));
        h->d_design = std::move(nb);
    }
    h->frames.erase(h->frames.begin() + index);
    h->frame_ids.erase(h->frame_ids.begin() + index);
    for (int f = index; f < n - 1; f++) h->frames[f].row0 -= nr;
    h->design_rows -= nr;
    h->r1_valid = false;
    return SGPR_OK;
}

extern "C" int sgpr_data_clear(sgpr_model *h)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_data_clear: bad arguments");
    h->frames.clear();
    h->frame_ids.clear();
    h->design_rows = 0;
    h->r1_valid = false;
    return SGPR_OK;
}

extern "C" int sgpr_data_info(sgpr_model *h, int32_t *frames, int64_t *rows)
{
    if (!h) return fail(SGPR_E_INVALID, "sgpr_data_info: bad arguments");
    if (frames) *frames = (int32_t)h->frames.size();
    if (rows) *rows = h->design_rows;
    return SGPR_OK;
}

extern "C" int sgpr_data_matvec(sgpr_model *h, const double *v, double *out)
{
    if (!h || !v || !out) return fail(SGPR_E_INVALID, "sgpr_data_matvec: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_data_matvec: no inducing set");
    const int64_t rows = h->design_rows;
    if (rows == 0) return SGPR_OK;
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> &d_v = h->sc_mv_v, &d_o = h->sc_mv_o;
    if (d_v.alloc(h->m, false) || d_o.alloc(rows, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed");
    hipStream_t st = h->stream;
    HIPCHK(hipMemcpyAsync(d_v.p, v, sizeof(double) * h->m, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(design_matvec_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, h->m, h->d_design.p,
                       (size_t)h->design_rcap, d_v.p, d_o.p);
    HIPCHK(hipMemcpyAsync(out, d_o.p, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

// (K v - Y) reduced on the device: the fit statistics of make_stats (gppotential.py:610-649) need one number per frame
// (its energy residual) and a handful of sums over the force / virial rows — not 10^5..10^6 residuals on the host.
// part[b][7] = {sum d, sum |d|, sum d^2, sum y, sum y^2, max |y|, count} over the non-energy rows of block b
__global__ __launch_bounds__(256) void design_fit_stats_kernel(int64_t rows, int m, const double *design, size_t rcap,
                                                               const double *v, const double *Y, const int64_t *erow, int nf,
                                                               double *e_pred, double *part)
{
    __shared__ double red[4][7];
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double q[7] = {0, 0, 0, 0, 0, 0, 0};
    if (r < rows) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int c = 0;
        for (; c + 4 <= m; c += 4) {
            s0 += design[(size_t)c * rcap + r] * v[c];
            s1 += design[(size_t)(c + 1) * rcap + r] * v[c + 1];
            s2 += design[(size_t)(c + 2) * rcap + r] * v[c + 2];
            s3 += design[(size_t)(c + 3) * rcap + r] * v[c + 3];
        }
        for (; c < m; c++) s0 += design[(size_t)c * rcap + r] * v[c];
        const double pred = (s0 + s1) + (s2 + s3);
        // energy row of a frame?  (erow sorted ascending)
        int lo = 0, hi = nf;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (erow[mid] < r) lo = mid + 1; else hi = mid; }
        if (lo < nf && erow[lo] == r) e_pred[lo] = pred;
        else {
            const double y = Y[r], d = pred - y;
            q[0] = d; q[1] = fabs(d); q[2] = d * d; q[3] = y; q[4] = y * y; q[5] = fabs(y); q[6] = 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double x = q[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double y = __shfl_xor(x, o, 64);
            x = k == 5 ? fmax(x, y) : x + y;
        }
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * 7 + k] = k == 5 ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                                                  : (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

__global__ __launch_bounds__(256) void design_fit_stats_final_kernel(int nb, const double *part, double *out)
{
    __shared__ double red[256];
    for (int k = 0; k < 7; k++) {
        double x = 0.0;
        for (int b = threadIdx.x; b < nb; b += 256) x = k == 5 ? fmax(x, part[(size_t)b * 7 + k]) : x + part[(size_t)b * 7 + k];
        red[threadIdx.x] = x;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) red[threadIdx.x] = k == 5 ? fmax(red[threadIdx.x], red[threadIdx.x + o]) : red[threadIdx.x] + red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = red[0];
        __syncthreads();
    }
}

// The objective of the noise search (gppotential.py:1265-1300: the mean absolute error of the FORCE rows of K mu against
// their targets) for up to sixteen weight vectors per pass over the resident matrix: part[block][b] = sum |K v_b - Y|
// over the force rows of the block.  (One sgpr_data_matvec per candidate brought rows x 8 bytes back to the host for
// one number each: 16 x 4 MB per scan at ten stored 16384-atom frames.)
#define MAE_BATCH 16
__global__ __launch_bounds__(256) void design_force_mae_kernel(int64_t rows, int m, const double *design, size_t rcap,
                                                               const double *V, int nb_v, const double *Y, const int64_t *erow,
                                                               const int64_t *fend, int nf, double *part)
{
    __shared__ double red[4][MAE_BATCH];
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double s[MAE_BATCH];
#pragma unroll
    for (int b = 0; b < MAE_BATCH; b++) s[b] = 0.0;
    bool force_row = false;
    if (r < rows) {
        // frame of the row: the last energy row at or before it (erow sorted ascending); force rows end at fend
        int lo = 0, hi = nf;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (erow[mid] <= r) lo = mid + 1; else hi = mid; }
        const int f = lo - 1;
        force_row = f >= 0 && r > erow[f] && r < fend[f];
    }
    // sixty-four columns of the sixteen vectors at a time through LDS (sV[column][vector]: a row's sixteen values are four
    // 16-byte broadcast reads); rows of V beyond nb_v are zero
    __shared__ __attribute__((aligned(16))) double sV[64][MAE_BATCH];
    for (int c0 = 0; c0 < m; c0 += 64) {
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * MAE_BATCH; e += 256) {
            const int cc = e & 63, b = e >> 6;
            sV[cc][b] = c0 + cc < m ? V[(size_t)b * m + c0 + cc] : 0.0;
        }
        __syncthreads();
        if (r < rows) {
            const int nc = min(64, m - c0);
            for (int cc = 0; cc < nc; cc++) {
                const double a = design[(size_t)(c0 + cc) * rcap + r];
#pragma unroll
                for (int b = 0; b < MAE_BATCH; b++) s[b] += a * sV[cc][b];
            }
        }
    }
    const double y = force_row ? Y[r] : 0.0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < MAE_BATCH; b++) {
        double x = force_row ? fabs(s[b] - y) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) red[wave][b] = x;
    }
    __syncthreads();
    if (threadIdx.x < MAE_BATCH)
        part[(size_t)blockIdx.x * MAE_BATCH + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void design_force_mae_final_kernel(int nb, const double *part, double *out)
{
    __shared__ double red[256];
    for (int k = 0; k < MAE_BATCH; k++) {
        double x = 0.0;
        for (int b = threadIdx.x; b < nb; b += 256) x += part[(size_t)b * MAE_BATCH + k];
        red[threadIdx.x] = x;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = red[0];
        __syncthreads();
    }
}

extern "C" int sgpr_data_force_mae(sgpr_model *h, int count, const double *V, const double *Y, double *mae_out)
{
    if (!h || count < 1 || !V || !Y || !mae_out) return fail(SGPR_E_INVALID, "sgpr_data_force_mae: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_data_force_mae: no inducing set");
    const int64_t rows = h->design_rows;
    const int nf = (int)h->frames.size(), m = h->m;
    int64_t nforce = 0;
    for (const auto &fr : h->frames) nforce += 3 * (int64_t)fr.N;
    for (int b = 0; b < count; b++) mae_out[b] = 0.0;
    if (rows == 0 || nf == 0 || nforce == 0) return SGPR_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int nb = (int)((rows + 255) / 256);
    DevBuf<double> &d_v = h->sc_mae_v, &d_y = h->sc_y, &d_o = h->sc_mv_o;
    DevBuf<int64_t> &d_fr = h->sc_mae_rows;
    std::vector<int64_t> er(2 * (size_t)nf);
    for (int f = 0; f < nf; f++) { er[f] = h->frames[f].row0; er[nf + f] = h->frames[f].row0 + 1 + 3 * (int64_t)h->frames[f].N; }
    if (d_v.alloc((size_t)MAE_BATCH * m, false) || d_y.alloc(rows, false) || d_o.alloc((size_t)nb * MAE_BATCH + MAE_BATCH, false) ||
        d_fr.alloc(2 * (size_t)nf, false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed");
    HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_fr.p, er.data(), sizeof(int64_t) * 2 * nf, hipMemcpyHostToDevice, st));
    std::vector<double> back(MAE_BATCH);
    for (int b0 = 0; b0 < count; b0 += MAE_BATCH) {
        const int nbv = std::min(MAE_BATCH, count - b0);
        HIPCHK(hipMemsetAsync(d_v.p, 0, sizeof(double) * MAE_BATCH * m, st));
        HIPCHK(hipMemcpyAsync(d_v.p, V + (size_t)b0 * m, sizeof(double) * (size_t)nbv * m, hipMemcpyHostToDevice, st));
        double *part = d_o.p, *d_out = d_o.p + (size_t)nb * MAE_BATCH;
        hipLaunchKernelGGL(design_force_mae_kernel, dim3(nb), dim3(256), 0, st, rows, m, h->d_design.p, (size_t)h->design_rcap, d_v.p,
                           nbv, d_y.p, d_fr.p, d_fr.p + nf, nf, part);
        hipLaunchKernelGGL(design_force_mae_final_kernel, dim3(1), dim3(256), 0, st, nb, part, d_out);
        HIPCHK(hipMemcpyAsync(back.data(), d_out, sizeof(double) * MAE_BATCH, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < nbv; b++) mae_out[b0 + b] = back[b] / (double)nforce;
    }
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

extern "C" int sgpr_data_fit_stats(sgpr_model *h, const double *v, const double *Y, double *e_pred, double *stats)
{
    if (!h || !v || !Y || !e_pred || !stats) return fail(SGPR_E_INVALID, "sgpr_data_fit_stats: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_data_fit_stats: no inducing set");
    const int64_t rows = h->design_rows;
    const int nf = (int)h->frames.size();
    for (int k = 0; k < 7; k++) stats[k] = 0.0;
    if (rows == 0 || nf == 0) return SGPR_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int nb = (int)((rows + 255) / 256);
    DevBuf<double> &d_v = h->sc_mv_v, &d_y = h->sc_y, &d_o = h->sc_mv_o;
    std::vector<int64_t> er(nf);
    for (int f = 0; f < nf; f++) er[f] = h->frames[f].row0;
    if (d_v.alloc(h->m, false) || d_y.alloc(rows, false) || d_o.alloc((size_t)nb * 7 + nf + 16, false) || h->sc_erow.alloc(nf, false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed");
    HIPCHK(hipMemcpyAsync(d_v.p, v, sizeof(double) * h->m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->sc_erow.p, er.data(), sizeof(int64_t) * nf, hipMemcpyHostToDevice, st));
    double *part = d_o.p, *d_e = d_o.p + (size_t)nb * 7, *d_out = d_e + nf;
    hipLaunchKernelGGL(design_fit_stats_kernel, dim3(nb), dim3(256), 0, st, rows, h->m, h->d_design.p, (size_t)h->design_rcap, d_v.p,
                       d_y.p, h->sc_erow.p, nf, d_e, part);
    hipLaunchKernelGGL(design_fit_stats_final_kernel, dim3(1), dim3(256), 0, st, nb, part, d_out);
    std::vector<double> back(nf + 8);
    HIPCHK(hipMemcpyAsync(back.data(), d_e, sizeof(double) * (nf + 7), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    for (int f = 0; f < nf; f++) e_pred[f] = back[f];
    for (int k = 0; k < 7; k++) stats[k] = back[nf + k];
    return SGPR_OK;
}

extern "C" int sgpr_data_get(sgpr_model *h, double *K)
{
    if (!h || !K) return fail(SGPR_E_INVALID, "sgpr_data_get: bad arguments");
    const int64_t rows = h->design_rows;
    const int m = h->m;
    if (rows == 0 || m <= 0) return SGPR_OK;
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> d_t;
    if (d_t.alloc((size_t)rows * m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed");
    // [m][rcap] -> [rows][m]
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((rows + 31) / 32), (m + 31) / 32), dim3(32, 8), 0, h->stream, m, (int)rows,
                       h->d_design.p, (int)h->design_rcap, d_t.p, m);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(K, d_t.p, sizeof(double) * (size_t)rows * m, hipMemcpyDeviceToHost));
    return SGPR_OK;
}

// ---------------------------------------------------------------------------- the kept factorisation
// (regression/gppotential.py:745-791 refits from scratch after every add_inducing / pop_1inducing; here the QR of
// the resident [K | Y] is kept with its reflectors, so that the LCE a trial appends is ONE column pushed through
// them — Q^T k, then its own one-column panel — and the LCE a rejection pops is that column dropped again.)
// SGPR_NANCHECK=1 (diagnostic): first non-finite entry of a device array, reported on stderr
static void nan_check(const char *what, const double *dev, size_t n)
{
    static const bool on = getenv("SGPR_NANCHECK") != nullptr;
    if (!on || !dev || !n) return;
    std::vector<double> hbuf(n);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(hbuf.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost);
    size_t bad = 0, first = n;
    double amax = 0.0;
    for (size_t i = 0; i < n; i++) {
        if (!std::isfinite(hbuf[i])) { bad++; if (first == n) first = i; }
        else amax = std::max(amax, fabs(hbuf[i]));
    }
    fprintf(stderr, "[sgpr nancheck] %s: %zu values, %zu non-finite (first at %zu), max |x| = %.3e\n", what, n, bad, first, amax);
}

#define QR_APPEND_MAX 32   // appended one-column panels before the next full factorisation

// (skip: sorted rows left out of the key — the energy rows, which the force-only fit zeroes: the mean is refitted
// with every edit and moves the energy targets, which that fit never sees)
static void y_key(const double *Y, int64_t rows, uint64_t key[2], const std::vector<int64_t> *skip = nullptr)
{
    key[0] = 1469598103934665603ull; key[1] = 0x9e3779b97f4a7c15ull;
    size_t sk = 0;
    for (int64_t r = 0; r < rows; r++) {
        if (skip && sk < skip->size() && (*skip)[sk] == r) { sk++; continue; }
        uint64_t b; memcpy(&b, Y + r, 8);
        key[0] = (key[0] ^ b) * 1099511628211ull;
        key[1] = (key[1] + b) * 0xff51afd7ed558ccdull;
        key[1] ^= key[1] >> 33;
    }
    if (!key[0] && !key[1]) key[0] = 1;
}

__global__ void zero_rows_kernel(int n, const int64_t *rows, double *vec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vec[rows[i]] = 0.0;
}

// full factorisation of the resident matrix into slot k
static int qr_keep_factor(sgpr_model *h, sgpr_model::QrKeep *k, const double *Y, int64_t rows, int with_energies)
{
    const int m = h->m;
    hipStream_t st = h->stream;
    const int R = (int)rows, ldr = rup(R, 64), cpad = rup(m + 1, 64) + 64;
    const int ccap = rup(m + QR_APPEND_MAX + 8, 32);
    k->valid = false;
    const size_t store_need = tsqr_keep_doubles(R, m, 0) + (size_t)QR_APPEND_MAX * (ldr + 8);
    DevBuf<double> &d_A = h->d_qr_A, &d_work = h->d_qr_work;
    DevBuf<unsigned char> &d_ise = h->sc_ise;
    if (d_A.alloc((size_t)cpad * ldr, false) ||
        d_work.alloc(lstsq_qr_blocked_work_doubles(R, m + QR_APPEND_MAX) + flat_part_doubles(ldr), false) ||
        k->store.alloc(store_need, false) || k->Rc.alloc((size_t)ccap * ccap) || k->yt.alloc(ldr, false) ||
        k->yraw.alloc(ldr) || k->ysnap.alloc((size_t)QR_APPEND_MAX * ldr, false) || k->vec.alloc(ldr, false) ||
        d_ise.alloc(std::max<int64_t>(rows, 1)))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, %d x %d, kept reflectors)", R, m);
    HIPCHK(hipMemsetAsync(d_A.p, 0, sizeof(double) * (size_t)cpad * ldr, st));
    HIPCHK(hipMemcpyAsync(k->yraw.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
    k->with_energies = with_energies;
    k->n_erows = (int)h->frames.size();
    {
        std::vector<int64_t> er(std::max(k->n_erows, 1), 0);
        std::vector<unsigned char> ise((size_t)std::max<int64_t>(rows, 1), 0);
        for (size_t f = 0; f < h->frames.size(); f++) { er[f] = h->frames[f].row0; ise[(size_t)er[f]] = 1; }
        if (k->erows.alloc(er.size(), false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares)");
        HIPCHK(hipMemcpy(k->erows.p, er.data(), sizeof(int64_t) * er.size(), hipMemcpyHostToDevice));
        if (!with_energies) HIPCHK(hipMemcpy(d_ise.p, ise.data(), ise.size(), hipMemcpyHostToDevice));
    }
    const int gx = (int)std::min<int64_t>((rows + 255) / 256, 8192);
    hipLaunchKernelGGL(design_to_qr_kernel, dim3(gx, m + 1), dim3(256), 0, st, rows, m, h->d_design.p, (size_t)h->design_rcap,
                       k->yraw.p, d_ise.p, with_energies, d_A.p, ldr);
    if (launch_lstsq_qr_blocked(R, m, d_A.p, ldr, nullptr, d_work.p, st, 0, k->store.p, &k->panels))
        return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    launch_qr_gather_r(m, d_A.p, ldr, k->Rc.p, ccap, k->vec.p /*z, unused: yt has it*/, st);
    HIPCHK(hipMemcpyAsync(k->yt.p, d_A.p + (size_t)m * ldr, sizeof(double) * ldr, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    k->rows = (int)rows; k->R = R; k->ldr = ldr; k->ncols = m; k->ccap = ccap;
    k->frame_ids = h->frame_ids; k->col_ids = h->col_ids;
    {
        std::vector<int64_t> er;
        for (const auto &fr : h->frames) er.push_back(fr.row0);
        y_key(Y, rows, k->ykey, with_energies ? nullptr : &er);
    }
    k->store_used = k->store_base = tsqr_keep_doubles(R, m, 0);
    k->clear_ops();
    k->valid = true;
    return SGPR_OK;
}

// vec[0:n] <- E vec[0:n] for an explicit n x n matrix (E[c * ld + r]): column chunks summed in order by each row's
// thread, then the chunks in order — the same bits every run
#define DENSE_QT_CHUNKS 32
__global__ __launch_bounds__(256) void dense_qt_part_kernel(int n, const double *E, int ld, const double *vec, double *part)
{
    const int r = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    const int per = (n + DENSE_QT_CHUNKS - 1) / DENSE_QT_CHUNKS, c0 = ch * per, c1 = min(n, c0 + per);
    if (r >= n) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = c0;
    for (; c + 3 < c1; c += 4) {
        s0 += E[(size_t)c * ld + r] * vec[c];
        s1 += E[(size_t)(c + 1) * ld + r] * vec[c + 1];
        s2 += E[(size_t)(c + 2) * ld + r] * vec[c + 2];
        s3 += E[(size_t)(c + 3) * ld + r] * vec[c + 3];
    }
    for (; c < c1; c++) s0 += E[(size_t)c * ld + r] * vec[c];
    part[(size_t)ch * n + r] = (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(256) void dense_qt_sum_kernel(int n, const double *part, double *vec)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double s = 0.0;
    for (int ch = 0; ch < DENSE_QT_CHUNKS; ch++) s += part[(size_t)ch * n + r];
    vec[r] = s;
}

// vec <- Q^T vec: the panels of the full factorisation, then what came after it in order (the reflectors of the
// appended columns, the explicit factors of the column selections)
static void qr_keep_apply_all(sgpr_model *h, sgpr_model::QrKeep *k, double *vec, hipStream_t st)
{
    tsqr_apply_panels(k->panels.data(), (int)k->panels.size(), vec, st);
    for (const auto &o : k->ops) {
        if (o.kind == 0) {
            const double *slot = k->store.p + k->store_base + o.flat_ix * (size_t)(k->ldr + 8);
            flat_reflector_apply(slot, slot + k->ldr, k->R - o.k0, vec + o.k0, h->d_qr_work.p, st);
        } else {
            hipLaunchKernelGGL(dense_qt_part_kernel, dim3((o.rows + 255) / 256, DENSE_QT_CHUNKS), dim3(256), 0, st, o.rows, o.pstore.p,
                               o.ld, vec, h->sc_dense_part.p);
            hipLaunchKernelGGL(dense_qt_sum_kernel, dim3((o.rows + 255) / 256), dim3(256), 0, st, o.rows, h->sc_dense_part.p, vec);
        }
    }
}

__global__ void identity_cols_kernel(int n, double *A, int ld)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[(size_t)i * ld + i] = 1.0;
}

// one more column (the caller's column c of the resident matrix) at the end
static int qr_keep_append(sgpr_model *h, sgpr_model::QrKeep *k, int c, int64_t id)
{
    hipStream_t st = h->stream;
    const int k0 = k->ncols;
    HIPCHK(hipMemsetAsync(k->vec.p, 0, sizeof(double) * k->ldr, st));
    HIPCHK(hipMemcpyAsync(k->vec.p, h->d_design.p + (size_t)c * h->design_rcap, sizeof(double) * k->rows, hipMemcpyDeviceToDevice, st));
    if (!k->with_energies && k->n_erows > 0)
        hipLaunchKernelGGL(zero_rows_kernel, dim3((k->n_erows + 63) / 64), dim3(64), 0, st, k->n_erows, k->erows.p, k->vec.p);
    qr_keep_apply_all(h, k, k->vec.p, st);
    const int na = k->nflat;
    HIPCHK(hipMemcpyAsync(k->ysnap.p + (size_t)na * k->ldr, k->yt.p, sizeof(double) * k->ldr, hipMemcpyDeviceToDevice, st));
    double *slot = k->store.p + k->store_base + na * (size_t)(k->ldr + 8);
    flat_reflector_make(k->vec.p + k0, k->R - k0, slot, slot + k->ldr, slot + k->ldr + 1, h->d_qr_work.p, st);
    flat_reflector_apply(slot, slot + k->ldr, k->R - k0, k->yt.p + k0, h->d_qr_work.p, st);
    // the new column of R1: what is above the diagonal as it is, alpha on it
    if (k0 > 0)
        HIPCHK(hipMemcpyAsync(k->Rc.p + (size_t)k0 * k->ccap, k->vec.p, sizeof(double) * k0, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(k->Rc.p + (size_t)k0 * k->ccap + k0, slot + k->ldr + 1, sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipGetLastError());
    sgpr_model::QrKeep::Op op;
    op.kind = 0; op.k0 = k0; op.flat_ix = na; op.snap = 1;
    k->ops.push_back(std::move(op));
    k->nflat++;
    k->store_used += (size_t)(k->ldr + 8);
    k->ncols++;
    k->col_ids.push_back(id);
    return SGPR_OK;
}

// the last column gone
static int qr_keep_pop(sgpr_model *h, sgpr_model::QrKeep *k)
{
    k->ncols--;
    k->col_ids.pop_back();
    if (!k->ops.empty() && k->ops.back().kind == 0 && k->ops.back().k0 == k->ncols) {
        const auto &o = k->ops.back();
        if (o.snap)
            HIPCHK(hipMemcpyAsync(k->yt.p, k->ysnap.p + (size_t)o.flat_ix * k->ldr, sizeof(double) * k->ldr, hipMemcpyDeviceToDevice, h->stream));
        else
            k->ykey[0] = k->ykey[1] = 0;  // Q^T Y is rebuilt from Y
        k->store_used -= (size_t)(k->ldr + 8);
        k->ops.pop_back();
        k->nflat--;
    }
    // (a column of the full factorisation or of a selection: Q stays an orthogonal factor of the remaining columns,
    // R1 and z lose their last entry)
    return SGPR_OK;
}

// At[c][r] = R1[r][idx[c]] (c < count), At[count][r] = (Q^T Y)[r]: the kept triangle with its columns selected /
// permuted, rows [0, R2) (zero below the old triangle: those rows of Q^T K are zero for every kept column)
__global__ void select_build_kernel(int m_old, int count, int R2, const double *Rc, int ccap, const int *idx, const double *yt,
                                    double *At, int ldr2)
{
    const int c = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R2 || c > count) return;
    double v;
    if (c == count) v = yt[r];
    else {
        const int j = idx[c];
        v = (r <= j && r < m_old) ? Rc[(size_t)j * ccap + r] : 0.0;
    }
    At[(size_t)c * ldr2 + r] = v;
}

#define QR_SELECT_MAX 64   // column selections folded into a kept factorisation before the next full one (9 MB each at m = 1024)

// The columns idx[0..count) of a kept factorisation become its columns 0..count (a subset, in any order):
//   K[:, idx] = Q [R1[:, idx]; 0] = Q [Q2 R1'; 0]   with   R1[:, idx] = Q2 R1'  (an m_old x count QR: 10^6 entries,
// not the 10^5..10^6 x m design matrix), so Q <- Q diag(Q2, I): Q2's panels join the chain, Q^T Y follows.
// (downsize(lii=True), gppotential.py:829-832: the reference refits from scratch after it.)
static int qr_keep_select(sgpr_model *h, sgpr_model::QrKeep *k, int count, const int32_t *idx, const std::vector<int64_t> &new_ids)
{
    hipStream_t st = h->stream;
    const int m_old = k->ncols;
    int nsel = 0;
    for (const auto &o : k->ops) nsel += o.kind == 1;
    const int R2 = std::max(m_old, count + 1);
    if (count < 1 || count > k->ccap - 1 || R2 > k->R || nsel >= QR_SELECT_MAX) { k->valid = false; return SGPR_OK; }
    const int ldr2 = rup(R2, 64), cpad = rup(count + 1 + R2, 64) + 64;
    sgpr_model::QrKeep::Op op;
    op.kind = 1; op.rows = R2; op.ld = ldr2;
    DevBuf<int> &d_idx = h->sc_sel_idx;
    DevBuf<double> &d_A = h->sc_sel_A, &d_work = h->sc_sel_work;
    if (d_idx.alloc(count, false) || d_A.alloc((size_t)cpad * ldr2, false) ||
        d_work.alloc(lstsq_qr_blocked_work_doubles(R2, count), false) || op.pstore.alloc((size_t)R2 * ldr2, false) ||
        h->sc_dense_part.alloc((size_t)DENSE_QT_CHUNKS * 2176, false)) {
        k->valid = false;  // no room: the next refit factors from scratch
        return SGPR_OK;
    }
    HIPCHK(hipMemcpyAsync(d_idx.p, idx, sizeof(int) * count, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_A.p, 0, sizeof(double) * (size_t)cpad * ldr2, st));
    hipLaunchKernelGGL(select_build_kernel, dim3((R2 + 255) / 256, count + 1), dim3(256), 0, st, m_old, count, R2, k->Rc.p, k->ccap,
                       d_idx.p, k->yt.p, d_A.p, ldr2);
    // the identity behind the targets: the factorisation carries it along and leaves Q2^T there
    double *E = d_A.p + (size_t)(count + 1) * ldr2;
    hipLaunchKernelGGL(identity_cols_kernel, dim3((R2 + 255) / 256), dim3(256), 0, st, R2, E, ldr2);
    if (launch_lstsq_qr_blocked(R2, count, d_A.p, ldr2, nullptr, d_work.p, st, 0, nullptr, nullptr, R2)) {
        k->valid = false;
        return SGPR_OK;
    }
    HIPCHK(hipMemcpyAsync(op.pstore.p, E, sizeof(double) * (size_t)R2 * ldr2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(k->Rc.p, 0, sizeof(double) * (size_t)k->ccap * k->ccap, st));
    launch_qr_gather_r(count, d_A.p, ldr2, k->Rc.p, k->ccap, k->vec.p /*unused*/, st);
    HIPCHK(hipMemcpyAsync(k->yt.p, d_A.p + (size_t)count * ldr2, sizeof(double) * R2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (idx is the caller's host memory; the scratch is reused)
    HIPCHK(hipGetLastError());
    if (getenv("SGPR_NANCHECK")) {
        fprintf(stderr, "[sgpr nancheck] select %d -> %d columns on a slot with %zu ops (%d flats), R2 = %d\n", m_old, count, k->ops.size(), k->nflat, R2);
        nan_check("selected Rc", k->Rc.p, (size_t)k->ccap * k->ccap);
        nan_check("selected yt", k->yt.p, (size_t)k->ldr);
    }
    for (auto &o : k->ops) o.snap = 0;  // the snapshots are in the basis from before the selection
    k->ops.push_back(std::move(op));
    k->selected = true;
    k->ncols = count;
    k->col_ids = new_ids;
    return SGPR_OK;
}

// [R1 | z; B | y_B] (transposed storage): the kept factor of the old frames on top of the rows of the new frame
__global__ void row_append_build_kernel(int m, int64_t rows_b, const double *Rc, int ccap, const double *zt,
                                        const double *design, size_t rcap, int64_t row0_b, const double *Y, int drop_e,
                                        double *At, int ldr)
{
    const int c = blockIdx.y;  // column; c == m: the targets
    const int64_t n = m + rows_b;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        double v;
        if (r < m)
            v = c < m ? (r <= c ? Rc[(size_t)c * ccap + r] : 0.0) : zt[r];
        else {
            const int64_t rb = r - m;
            v = c < m ? design[(size_t)c * rcap + row0_b + rb] : Y[row0_b + rb];
            if (drop_e && rb == 0) v = 0.0;  // the frame's energy row
        }
        At[(size_t)c * ldr + r] = v;
    }
}

// A frame was pushed onto a kept factorisation (add_1atoms_fast's trial, gppotential.py:898-953): R1 and z of the
// larger matrix from qr([R1 z; B y_B]) — the rows of ONE frame instead of all — left in h->d_R1 (nothing is kept:
// the trial usually ends with the frame popped again; an accepted frame gets its own factorisation when an inducing
// edit needs one).  The targets of the old frames may have moved (the mean is refitted with the data): their Q^T Y is
// redone through the kept reflectors.
static int qr_row_append(sgpr_model *h, sgpr_model::QrKeep *k, const double *Y, int64_t rows)
{
    const int m = h->m;
    hipStream_t st = h->stream;
    const int64_t rows_b = rows - k->rows;
    const int R2 = (int)(m + rows_b), ldr2 = rup(R2, 64), cpad = rup(m + 1, 64) + 64;
    DevBuf<double> &d_A = h->d_qr_A, &d_work = h->d_qr_work;
    DevBuf<double> &d_y = h->sc_ra_y, &d_t = h->sc_ra_t;
    if (d_A.alloc((size_t)cpad * ldr2, false) ||
        d_work.alloc(lstsq_qr_blocked_work_doubles(std::max(R2, k->R), m + QR_APPEND_MAX) + flat_part_doubles(k->ldr), false) ||
        d_y.alloc(rows, false) || d_t.alloc(k->ldr) || h->d_R1.alloc((size_t)m * m + m, false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, row append)");
    HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_t.p, d_y.p, sizeof(double) * k->rows, hipMemcpyDeviceToDevice, st));
    if (!k->with_energies && k->n_erows > 0)
        hipLaunchKernelGGL(zero_rows_kernel, dim3((k->n_erows + 63) / 64), dim3(64), 0, st, k->n_erows, k->erows.p, d_t.p);
    qr_keep_apply_all(h, k, d_t.p, st);
    if (getenv("SGPR_NANCHECK")) {
        fprintf(stderr, "[sgpr nancheck] row append onto a slot with %d cols, %zu ops (%d flats), rows %d -> %lld\n", k->ncols, k->ops.size(),
                k->nflat, k->rows, (long long)rows);
        nan_check("slot Rc", k->Rc.p, (size_t)k->ccap * k->ccap);
        nan_check("slot yt", k->yt.p, (size_t)k->ldr);
        nan_check("Q^T Y_old", d_t.p, (size_t)k->ldr);
    }
    HIPCHK(hipMemsetAsync(d_A.p, 0, sizeof(double) * (size_t)cpad * ldr2, st));
    const int gx = (int)std::min<int64_t>((R2 + 255) / 256, 4096);
    hipLaunchKernelGGL(row_append_build_kernel, dim3(gx, m + 1), dim3(256), 0, st, m, rows_b, k->Rc.p, k->ccap, d_t.p,
                       h->d_design.p, (size_t)h->design_rcap, (int64_t)k->rows, d_y.p, k->with_energies ? 0 : 1, d_A.p, ldr2);
    if (launch_lstsq_qr_blocked(R2, m, d_A.p, ldr2, nullptr, d_work.p, st))
        return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    launch_qr_gather_r(m, d_A.p, ldr2, h->d_R1.p, m, h->d_R1.p + (size_t)m * m, st);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    h->r1_valid = true;
    return SGPR_OK;
}

// bring a slot to the current matrix and targets; *k_out = the slot.  Returns 1 if the path does not apply.
static int qr_keep_update(sgpr_model *h, const double *Y, int64_t rows, int with_energies, sgpr_model::QrKeep **k_out,
                          const char **how, bool report_selection = true)
{
    const int m = h->m;
    if (h->qr_keep_mode == 0) return 1;  // option "qr_keep" = 0: every refit factors from scratch
    if ((int)h->col_ids.size() != m || h->frame_ids.size() != h->frames.size() || rows < (int64_t)m + QR_APPEND_MAX + 64 ||
        m + QR_APPEND_MAX + 8 > 2048)
        return 1;
    static uint64_t clock = 0;
    sgpr_model::QrKeep *k = nullptr, *victim = nullptr;
    for (auto &e : h->qr_keep) {
        if (e.valid && e.with_energies == with_energies && e.rows == rows && e.frame_ids == h->frame_ids) k = &e;
        if (!victim || (victim->valid && (!e.valid || e.age < victim->age))) victim = &e;
    }
    if (!k) {
        // one frame more than a kept factorisation with the same columns: row append (return 2: R1 is in h->d_R1)
        for (auto &e : h->qr_keep) {
            if (!e.valid || e.with_energies != with_energies || e.ncols != m || e.col_ids != h->col_ids) continue;
            if (e.frame_ids.size() + 1 != h->frame_ids.size() || rows <= e.rows) continue;
            if (!std::equal(e.frame_ids.begin(), e.frame_ids.end(), h->frame_ids.begin())) continue;
            const int rc_ = qr_row_append(h, &e, Y, rows);
            if (rc_) return rc_;
            e.age = ++clock;
            *how = "rows of the new frame appended to the kept factor";
            return 2;
        }
    }
    bool full = true;
    if (k) {
        size_t p = 0;
        while (p < k->col_ids.size() && p < h->col_ids.size() && k->col_ids[p] == h->col_ids[p]) p++;
        const size_t pops = k->col_ids.size() - p, adds = h->col_ids.size() - p;
        if (p > 0 && adds <= 8 && k->nflat + adds <= QR_APPEND_MAX && m <= k->ccap - 1 && k->R - m >= 64) {
            full = false;
            for (size_t i = 0; i < pops; i++) { const int rc_ = qr_keep_pop(h, k); if (rc_) return rc_; }
            for (size_t i = 0; i < adds; i++) { const int rc_ = qr_keep_append(h, k, (int)(p + i), h->col_ids[p + i]); if (rc_) return rc_; }
            *how = pops || adds ? "columns appended / popped through the kept reflectors"
                                : (k->selected ? "columns selected through the kept reflectors" : "kept");
            if (report_selection || pops || adds) k->selected = false;  // (a factor-only call leaves the note for the fit that follows)
        }
    }
    if (full) {
        if (!k) k = victim;
        {
            // the reflectors of a slot are rows x (m + 32) doubles: keep them only while HBM has room to spare (several
            // models on one GPU — a committee — share it); otherwise every refit factors from scratch
            size_t free_b = 0, total_b = 0;
            const size_t need = sizeof(double) * (tsqr_keep_doubles((int)rows, m, 0) + (size_t)QR_APPEND_MAX * (rup((int)rows, 64) + 8));
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > k->store.n * sizeof(double) &&
                need - k->store.n * sizeof(double) + (total_b >> 3) > free_b) {
                k->valid = false;
                return 1;
            }
        }
        const int rc_ = qr_keep_factor(h, k, Y, rows, with_energies);
        if (rc_) return rc_;
        *how = "full factorisation";
    }
    // targets
    uint64_t key[2];
    {
        std::vector<int64_t> er;
        for (const auto &fr : h->frames) er.push_back(fr.row0);
        y_key(Y, rows, key, with_energies ? nullptr : &er);
    }
    if (key[0] != k->ykey[0] || key[1] != k->ykey[1]) {
        hipStream_t st = h->stream;
        HIPCHK(hipMemsetAsync(k->yraw.p, 0, sizeof(double) * k->ldr, st));
        HIPCHK(hipMemcpyAsync(k->yraw.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(k->yt.p, k->yraw.p, sizeof(double) * k->ldr, hipMemcpyDeviceToDevice, st));
        if (!k->with_energies && k->n_erows > 0)
            hipLaunchKernelGGL(zero_rows_kernel, dim3((k->n_erows + 63) / 64), dim3(64), 0, st, k->n_erows, k->erows.p, k->yt.p);
        qr_keep_apply_all(h, k, k->yt.p, st);
        for (auto &o : k->ops) o.snap = 0;
        k->ykey[0] = key[0]; k->ykey[1] = key[1];
    }
    k->age = ++clock;
    *k_out = k;
    return SGPR_OK;
}

// [E | y_E; R1f | zf] (transposed storage): the energy rows of the stored frames on top of the force-only factor — column c
// is zero below row n + c, a band the factorisation follows (panels of n + 32 rows instead of m + n)
__global__ void energy_append_build_kernel(int m, int n, const double *R1, const double *design, size_t rcap, const int64_t *erows,
                                           const double *Y, double *At, int ldr)
{
    const int c = blockIdx.y;  // column; c == m: the targets
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m + n) return;
    double v;
    if (r >= n) { const int q = r - n; v = c < m ? (q <= c ? R1[(size_t)c * m + q] : 0.0) : R1[(size_t)m * m + q]; }
    else v = c < m ? design[(size_t)c * rcap + erows[r]] : Y[erows[r]];
    At[(size_t)c * ldr + r] = v;
}

// The same update for a handful of energy rows (n <= 16: one per stored frame) without the launch chain of a blocked QR:
// ONE workgroup walks down the columns.  Step c: the owner of column c forms the Householder reflector of
// (R[c][c]; E[:, c]) and publishes it in LDS; every thread applies it to row c of R (row-major copy Rt: a coalesced row per
// step, the next row already requested) and to the energy-row entries of its own column(s), which it keeps in registers.
// One barrier per step (the reflector buffer alternates).  m = 1024, n = 2: 0.3 ms against 1.7 ms for the 64 launches
// of the banded factorisation.
#define ER_MAX 16
template <int SLOTS, int NE>  // NE: rows held per column (>= n; 2, 4 or 16: a run with one or two stored frames does not pay for sixteen)
__global__ __launch_bounds__(1024) void energy_rows_update_kernel(int m, double *Rt, int ldt, const double *design, size_t rcap,
                                                                  const int64_t *erows, int n, const double *Y)
{
    __shared__ __attribute__((aligned(16))) double sv[2][NE + 2];
    const int t = threadIdx.x;
    double e0[NE], e1[NE];
    const int col0 = t, col1 = t + 1024;
#pragma unroll
    for (int k = 0; k < NE; k++) {
        e0[k] = (k < n && col0 <= m) ? (col0 < m ? design[(size_t)col0 * rcap + erows[k]] : Y[erows[k]]) : 0.0;
        e1[k] = (SLOTS > 1 && k < n && col1 <= m) ? (col1 < m ? design[(size_t)col1 * rcap + erows[k]] : Y[erows[k]]) : 0.0;
    }
    double n0 = col0 <= m ? Rt[col0] : 0.0, n1 = (SLOTS > 1 && col1 <= m) ? Rt[col1] : 0.0;
    for (int c = 0; c < m; c++) {
        const double r0 = n0, r1 = n1;
        if (c + 1 < m) {  // the next row of R is on its way while this one is worked on
            n0 = (col0 <= m && col0 > c) ? Rt[(size_t)(c + 1) * ldt + col0] : 0.0;
            if (SLOTS > 1) n1 = (col1 <= m) ? Rt[(size_t)(c + 1) * ldt + col1] : 0.0;
        }
        double *pv = sv[c & 1];
        const int ot = c & 1023;
        const bool own1 = SLOTS > 1 && c >= 1024;
        if (t == ot) {
            const double x0 = own1 ? r1 : r0;
            double s2 = 0.0;
#pragma unroll
            for (int k = 0; k < NE; k++) { const double x = own1 ? e1[k] : e0[k]; pv[k] = x; s2 += x * x; }
            double v0 = 0.0, tau = 0.0, alpha = x0;
            if (s2 > 0.0) {
                const double nrm = sqrt(x0 * x0 + s2);
                alpha = x0 > 0.0 ? -nrm : nrm;
                v0 = x0 - alpha;
                tau = 2.0 / (v0 * v0 + s2);
            }
            pv[NE] = v0; pv[NE + 1] = tau;
            Rt[(size_t)c * ldt + c] = alpha;
#pragma unroll
            for (int k = 0; k < NE; k++) { if (own1) e1[k] = 0.0; else e0[k] = 0.0; }
        }
        __syncthreads();
        const double v0 = pv[NE], tau = pv[NE + 1];
        if (tau != 0.0) {
            double v[NE];
#pragma unroll
            for (int k = 0; k < NE; k++) v[k] = pv[k];
            if (col0 > c && col0 <= m) {
                double w = v0 * r0;
#pragma unroll
                for (int k = 0; k < NE; k++) w += v[k] * e0[k];
                w *= tau;
                Rt[(size_t)c * ldt + col0] = r0 - w * v0;
#pragma unroll
                for (int k = 0; k < NE; k++) e0[k] -= w * v[k];
            }
            if (SLOTS > 1 && col1 > c && col1 <= m) {
                double w = v0 * r1;
#pragma unroll
                for (int k = 0; k < NE; k++) w += v[k] * e1[k];
                w *= tau;
                Rt[(size_t)c * ldt + col1] = r1 - w * v0;
#pragma unroll
                for (int k = 0; k < NE; k++) e1[k] -= w * v[k];
            }
        }
    }
}

// The fit WITH energies from the force-only factor: K = [K_f-only rows; E], so qr([R1f zf; E y_E]) — m + n_frames rows —
// gives R1 and z of the whole matrix.  One kept factorisation (the force-only one, which the noise search needs anyway,
// gppotential.py:1265-1300) serves both fits: a frame pushed by add_1atoms_fast used to be factored into both, 18 ms each
// at 49 152 rows x 1024, and the energy targets — which move with every refit of the mean — no longer send Q^T Y through
// the whole reflector chain.  h->d_R1 holds [R1f | zf] on entry, [R1 | z] on return.
static int energy_rows_append(sgpr_model *h, const double *Y)
{
    const int m = h->m, n = (int)h->frames.size();
    if (n == 0) return SGPR_OK;
    hipStream_t st = h->stream;
    const int R2 = m + n, ldr2 = rup(R2, 64), cpad = rup(m + 1, 64) + 64;
    DevBuf<double> &d_A = h->sc_sel_A, &d_work = h->sc_sel_work, &d_y = h->sc_ea_y;
    DevBuf<int64_t> &d_er = h->sc_ea_rows;
    static const bool banded_only = getenv("SGPR_ENERGY_ROWS_QR") != nullptr;  // diagnostic: always the blocked factorisation
    if (n <= ER_MAX && m + 1 <= 2048 && !banded_only) {
        // a handful of rows: one workgroup, column by column, on a row-major copy of [R1f | zf]
        const int ldt = rup(m + 1, 32);
        std::vector<int64_t> er(n);
        for (int f = 0; f < n; f++) er[f] = h->frames[f].row0;
        if (d_A.alloc((size_t)m * ldt, false) || d_er.alloc(n, false) || d_y.alloc(std::max<int64_t>(h->design_rows, 1), false))
            return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, energy rows)");
        HIPCHK(hipMemcpyAsync(d_er.p, er.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * h->design_rows, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(transpose_kernel, dim3((m + 31) / 32, (m + 1 + 31) / 32), dim3(32, 8), 0, st, m + 1, m, h->d_R1.p, m, d_A.p, ldt);
#define ER_LAUNCH(S_, N_) hipLaunchKernelGGL((energy_rows_update_kernel<S_, N_>), dim3(1), dim3(1024), 0, st, m, d_A.p, ldt, \
                                             h->d_design.p, (size_t)h->design_rcap, d_er.p, n, d_y.p)
        if (m + 1 <= 1024) { if (n <= 2) ER_LAUNCH(1, 2); else if (n <= 4) ER_LAUNCH(1, 4); else ER_LAUNCH(1, 16); }
        else { if (n <= 2) ER_LAUNCH(2, 2); else if (n <= 4) ER_LAUNCH(2, 4); else ER_LAUNCH(2, 16); }
#undef ER_LAUNCH
        hipLaunchKernelGGL(transpose_kernel, dim3((m + 1 + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, st, m, m + 1, d_A.p, ldt, h->d_R1.p, m);
        HIPCHK(hipStreamSynchronize(st));  // (er is host memory)
        HIPCHK(hipGetLastError());
        return SGPR_OK;
    }
    if (d_A.alloc((size_t)cpad * ldr2, false) || d_work.alloc(lstsq_qr_blocked_work_doubles(R2, m), false) ||
        d_er.alloc(n, false) || d_y.alloc(std::max<int64_t>(h->design_rows, 1), false))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares, energy rows)");
    std::vector<int64_t> er(n);
    for (int f = 0; f < n; f++) er[f] = h->frames[f].row0;
    HIPCHK(hipMemcpyAsync(d_er.p, er.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * h->design_rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_A.p, 0, sizeof(double) * (size_t)cpad * ldr2, st));
    hipLaunchKernelGGL(energy_append_build_kernel, dim3((R2 + 255) / 256, m + 1), dim3(256), 0, st, m, n, h->d_R1.p, h->d_design.p,
                       (size_t)h->design_rcap, d_er.p, d_y.p, d_A.p, ldr2);
    if (launch_lstsq_qr_blocked(R2, m, d_A.p, ldr2, nullptr, d_work.p, st, 1, nullptr, nullptr, 0, n))
        return fail(SGPR_E_UNSUPPORTED, "least squares: m=%d exceeds the QR kernel limit", m);
    launch_qr_gather_r(m, d_A.p, ldr2, h->d_R1.p, m, h->d_R1.p + (size_t)m * m, st);
    HIPCHK(hipStreamSynchronize(st));  // (er is host memory)
    HIPCHK(hipGetLastError());
    return SGPR_OK;
}

static int data_solve_impl(sgpr_model *h, const double *Y, int with_energies, double noise0, double *mu_out,
                           double *choli_out, double *ridge_out, double *sigma_out, bool second_stage)
{
    if (!h || !Y) return fail(SGPR_E_INVALID, "sgpr_data_solve: bad arguments");
    if (h->m <= 0) return fail(SGPR_E_NOMODEL, "sgpr_data_solve: no inducing set");
    const int64_t rows = h->design_rows;
    if (rows > 0x7fffffff - 4096) return fail(SGPR_E_UNSUPPORTED, "sgpr_data_solve: more than 2^31 rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_graph(h);
    static const bool timing = getenv("SGPR_SOLVE_TIMING") != nullptr;
    auto now = []() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; };
    const double t0 = now();
    int rc_ = solve_factor_kmm(h);
    if (rc_) return rc_;
    const double t1 = now();
    const int m = h->m;
    const bool verify = h->qr_keep_mode == 2;  // option "qr_keep" = 2: both paths, the difference of mu on stderr
    std::vector<double> mu_keep;
    const char *how_keep = "";
    {
        // the kept factorisation: appended / popped columns go through its reflectors
        sgpr_model::QrKeep *k = nullptr;
        const char *how = "";
        // (always the force-only factorisation: the energy rows join below when the fit wants them)
        const int rk = qr_keep_update(h, Y, rows, 0, &k, &how, second_stage);
        if (rk < 0) return rk;
        h->info_stage1 = (rk == 0 || rk == 2) ? how : "from scratch";
        if (rk == 0 || rk == 2) {
            if (rk == 0) {
                if (h->d_R1.alloc((size_t)m * m + m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares)");
                HIPCHK(hipMemcpy2DAsync(h->d_R1.p, sizeof(double) * m, k->Rc.p, sizeof(double) * k->ccap, sizeof(double) * m, m,
                                        hipMemcpyDeviceToDevice, h->stream));
                HIPCHK(hipMemcpyAsync(h->d_R1.p + (size_t)m * m, k->yt.p, sizeof(double) * m, hipMemcpyDeviceToDevice, h->stream));
            }
            if (with_energies) {
                rc_ = energy_rows_append(h, Y);
                if (rc_) return rc_;
            }
            h->r1_valid = true;
            if (getenv("SGPR_NANCHECK")) {
                fprintf(stderr, "[sgpr nancheck] route: %s (m = %d, rows = %lld, slot cols %d, ops %zu, flats %d)\n", how, m, (long long)rows,
                        k ? k->ncols : -1, k ? k->ops.size() : (size_t)0, k ? k->nflat : -1);
                nan_check("R1 | z", h->d_R1.p, (size_t)m * m + m);
                nan_check("L", h->d_L.p, (size_t)h->m_rows * h->m_pad);
                nan_check("choli", h->d_choli.p, (size_t)h->m_rows * h->m_pad);
                if (k) { nan_check("slot Rc", k->Rc.p, (size_t)k->ccap * k->ccap); nan_check("slot yt", k->yt.p, (size_t)k->ldr); }
            }
            const double t2k = now();
            if (!second_stage) {
                HIPCHK(hipStreamSynchronize(h->stream));
                if (timing)
                    fprintf(stderr, "[sgpr data factor] rows=%lld m=%d we=%d: K_mm factor %.2f ms, stage 1 %.2f ms (%s)\n", (long long)rows, h->m,
                            with_energies, t1 - t0, now() - t1, how);
                return SGPR_OK;
            }
            rc_ = solve_stage2(h, noise0, mu_out, choli_out, ridge_out, sigma_out, verify ? -1 : with_energies);
            if (timing)
                fprintf(stderr, "[sgpr data solve] rows=%lld m=%d: K_mm factor %.2f ms, stage 1 %.2f ms (%s), stage 2 %.2f ms\n",
                        (long long)rows, h->m, t1 - t0, t2k - t1, how, now() - t2k);
            if (!verify || rc_ || !mu_out) return rc_;
            mu_keep.assign(mu_out, mu_out + m);
            how_keep = how;
        }
    }
    // the first stage only depends on (matrix, targets, with_energies): look it up
    uint64_t key[2] = {1469598103934665603ull, 0x9e3779b97f4a7c15ull};
    auto mix = [&](uint64_t v) {
        key[0] = (key[0] ^ v) * 1099511628211ull;
        key[1] = (key[1] + v) * 0xff51afd7ed558ccdull;
        key[1] ^= key[1] >> 33;
    };
    mix((uint64_t)with_energies); mix((uint64_t)rows); mix((uint64_t)m);
    for (int64_t id : h->frame_ids) mix((uint64_t)id);
    mix(0xabcdefull);
    for (int64_t id : h->col_ids) mix((uint64_t)id);
    for (int64_t r = 0; r < rows; r++) { uint64_t b; memcpy(&b, Y + r, 8); mix(b); }
    const bool ids_ok = !verify && (int)h->col_ids.size() == m && h->frame_ids.size() == h->frames.size();
    sgpr_model::R1Entry *hit = nullptr, *victim = &h->r1_cache[0];
    for (auto &e : h->r1_cache) {
        if (ids_ok && e.m == m && e.r1.p && e.key[0] == key[0] && e.key[1] == key[1]) hit = &e;
        if (e.age < victim->age) victim = &e;
    }
    if (hit) {
        h->info_stage1 = "found in the cache";
        if (h->d_R1.alloc((size_t)m * m + m, false)) return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares)");
        HIPCHK(hipMemcpyAsync(h->d_R1.p, hit->r1.p, sizeof(double) * ((size_t)m * m + m), hipMemcpyDeviceToDevice, h->stream));
        hit->age = ++h->r1_clock;
        h->r1_valid = true;
        const double t2h = now();
        if (!second_stage) { HIPCHK(hipStreamSynchronize(h->stream)); return SGPR_OK; }
        rc_ = solve_stage2(h, noise0, mu_out, choli_out, ridge_out, sigma_out, verify ? -1 : with_energies);
        if (timing)
            fprintf(stderr, "[sgpr data solve] rows=%lld m=%d: K_mm factor %.2f ms, stage 1 found in the cache, stage 2 %.2f ms\n",
                    (long long)rows, h->m, t1 - t0, now() - t2h);
        return rc_;
    }
    DevBuf<double> &d_y = h->sc_y;
    DevBuf<unsigned char> &d_ise = h->sc_ise;
    if (d_y.alloc(std::max<int64_t>(rows, 1), false) || d_ise.alloc(std::max<int64_t>(rows, 1)))
        return fail(SGPR_E_NODEVICE, "hipMalloc failed (least squares)");
    rc_ = solve_stage1(h, (int)rows, [&](double *At, int ldr, hipStream_t st) -> int {
        HIPCHK(hipMemcpyAsync(d_y.p, Y, sizeof(double) * rows, hipMemcpyHostToDevice, st));
        if (!with_energies) {
            std::vector<unsigned char> ise((size_t)rows, 0);
            for (const auto &fr : h->frames) ise[(size_t)fr.row0] = 1;
            HIPCHK(hipMemcpy(d_ise.p, ise.data(), (size_t)rows, hipMemcpyHostToDevice));
        }
        const int gx = (int)std::min<int64_t>((rows + 255) / 256, 8192);
        hipLaunchKernelGGL(design_to_qr_kernel, dim3(gx, m + 1), dim3(256), 0, st, rows, m, h->d_design.p, (size_t)h->design_rcap,
                           d_y.p, d_ise.p, with_energies, At, ldr);
        return 0;
    });
    if (rc_) return rc_;
    if (ids_ok && !victim->r1.alloc((size_t)m * m + m, false)) {
        HIPCHK(hipMemcpyAsync(victim->r1.p, h->d_R1.p, sizeof(double) * ((size_t)m * m + m), hipMemcpyDeviceToDevice, h->stream));
        victim->key[0] = key[0]; victim->key[1] = key[1];
        victim->m = m;
        victim->age = ++h->r1_clock;
    }
    const double t2 = now();
    if (!second_stage) return SGPR_OK;
    rc_ = solve_stage2(h, noise0, mu_out, choli_out, ridge_out, sigma_out, verify ? -1 : with_energies);
    if (!mu_keep.empty() && !rc_) {
        double dmax = 0.0, nmax = 0.0;
        for (int q = 0; q < m; q++) { dmax = std::max(dmax, fabs(mu_keep[q] - mu_out[q])); nmax = std::max(nmax, fabs(mu_out[q])); }
        fprintf(stderr, "[sgpr verify] rows=%lld m=%d we=%d (%s): max|mu_keep - mu_full| / max|mu| = %.3e\n", (long long)rows, m,
                with_energies, how_keep, dmax / (nmax > 0 ? nmax : 1.0));
    }
    if (timing)
        fprintf(stderr, "[sgpr data solve] rows=%lld m=%d: K_mm factor %.2f ms, stage 1 (QR of the resident [K|Y]) %.2f ms, stage 2 %.2f ms\n",
                (long long)rows, h->m, t1 - t0, t2 - t1, now() - t2);
    return rc_;
}

extern "C" int sgpr_data_solve(sgpr_model *h, const double *Y, int with_energies, double noise0, double *mu_out,
                               double *choli_out, double *ridge_out, double *sigma_out)
{
    return data_solve_impl(h, Y, with_energies, noise0, mu_out, choli_out, ridge_out, sigma_out, true);
}

// The first stage alone (K_mm factor + [R1, z] of the resident [K | Y]): what the noise search needs before its
// sgpr_resolve / sgpr_resolve_batch evaluations; the weights installed for prediction are not touched.
extern "C" int sgpr_data_factor(sgpr_model *h, const double *Y, int with_energies)
{
    return data_solve_impl(h, Y, with_energies, 0.0, nullptr, nullptr, nullptr, nullptr, false);
}

extern "C" int sgpr_solve_info(sgpr_model *h, char *buf, int cap)
{
    if (!h || !buf || cap < 1) return fail(SGPR_E_INVALID, "sgpr_solve_info: bad arguments");
    // ("rows=" stays the last field: callers read everything behind it as the route)
    snprintf(buf, (size_t)cap, "stage1=%s; stage2=%s; kmm_blocks=%d/%d; step=knm%d wcov%d chain%d cov=%s; rows=%s", h->info_stage1.c_str(),
             h->info_stage2, h->info_blocks_done, h->info_blocks, h->info_step_bm_k, h->info_step_bm_w, h->info_step_chain,
             h->info_step_cov, h->info_rows);
    return SGPR_OK;
}
