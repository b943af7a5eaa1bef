// spmm.hip — fp64 CSR times a dense block of k vectors for gfx950:  Y = alpha·A·X + beta·Y, X: cols × k, Y: rows × k (include/g4s.h, g4s_spmm).
//
// k SpMVs read the matrix k times; this reads it once per column tile (up to 32 vectors) and, on a row-major X, gathers k contiguous doubles per entry
// instead of one. One kernel family serves every handle, whichever of the four SpMV paths it took: it runs on the handle's CSR arrays and on the
// row-streaming plan of spmv.hip (spmv_stream.hpp: row-aligned blocks of <= 2048 entries, 2048-entry chunks of longer rows), which a blocked-path handle builds on demand.
//
//   * spmm_csr_kernel<KT, MODE> — one workgroup per (plan block, tile of KT columns). The block's column ids and values are staged in LDS with
//     coalesced loads; then a group of KT/2 lanes (1 lane for KT = 1) owns one row and the tile, each lane two columns, and walks the row's entries
//     in stored order: every (row, column) of an unchunked row is summed left to right — the oracle's order, so it is bit-identical to the oracle's
//     SpMV of that column. Four entries' gathers are issued before their products are added. A long-row chunk is split among the groups in
//     contiguous pieces; the pieces' sums are added in group order into the chunk's slot of the workspace.
//   * spmm_long_fixup_kernel — per (long row, column), the chunk partials in chunk order. No atomics anywhere: results are bit-equal run to run.
//
// MODE: 0 = row-major with 16-byte loads / stores of column pairs (X, Y 16-byte aligned, even ld), 1 = row-major with 8-byte accesses (any
// alignment, odd ld), 2 = column-major (element (i, j) at [i + j·ld]; strided, correct but slower). Columns past k in the last tile are masked:
// those lanes load and store nothing, so padding of Y is never touched.
#include "common.hpp"
#include "csr_handle.hpp"
#include <algorithm>
#include <new>
#include <vector>

namespace {

constexpr int WG = 256;
using g4s::TILE_NNZ;
using g4s::TILE_ROWS;
using g4s::LongChunk;
using g4s::LongRow;
static_assert(g4s::LONG_CHUNK <= TILE_NNZ, "a long-row chunk is staged in the LDS tile of a block");
constexpr int kMaxTile = 32;     // vectors per column tile

typedef double spmm_double2 __attribute__((ext_vector_type(2)));

template <int MODE>
__device__ __forceinline__ long long at(int i, int j, long long ld) { return MODE == 2 ? (long long)i + (long long)j * ld : (long long)i * ld + j; }

// The lane's (up to) two columns j, j+1 of row i; only live columns are read.
template <int MODE>
__device__ __forceinline__ void load2(const double *__restrict__ M, int i, int j, long long ld, bool live0, bool live1, double &a, double &b)
{
    if (MODE == 0 && live1) {
        const spmm_double2 v = *reinterpret_cast<const spmm_double2 *>(M + at<MODE>(i, j, ld));
        a = v[0]; b = v[1];
    } else {
        a = live0 ? M[at<MODE>(i, j, ld)] : 0.0;
        b = live1 ? M[at<MODE>(i, j + 1, ld)] : 0.0;
    }
}

__device__ __forceinline__ double combine(double s, double alpha, double beta, double old) { return beta == 0.0 ? alpha * s : alpha * s + beta * old; }

template <int MODE>
__device__ __forceinline__ void store2(double *__restrict__ Y, int i, int j, long long ld, bool live0, bool live1, double s0, double s1, double alpha, double beta)
{
    if (MODE == 0 && live1) {
        spmm_double2 *p = reinterpret_cast<spmm_double2 *>(Y + at<MODE>(i, j, ld));
        spmm_double2 o = {0.0, 0.0};
        if (beta != 0.0) o = *p;                                         // beta == 0 never reads Y
        spmm_double2 v;
        v[0] = combine(s0, alpha, beta, o[0]);
        v[1] = combine(s1, alpha, beta, o[1]);
        *p = v;
    } else {
        if (live0) { double *p = Y + at<MODE>(i, j, ld); *p = combine(s0, alpha, beta, beta != 0.0 ? *p : 0.0); }
        if (live1) { double *p = Y + at<MODE>(i, j + 1, ld); *p = combine(s1, alpha, beta, beta != 0.0 ? *p : 0.0); }
    }
}

// Sequential sum over staged entries [a, b) for the lane's columns, in stored order; four entries' gathers in flight before their products are added.
// (Measured against two other forms at full size, DESIGN §4.1 (e): masked batches of eight without a serial tail, and a kernel without LDS — one
// group per row, ids and values read from global memory, 6-8 waves per SIMD instead of 4 — were both slower, the second by 7 % on the 431³ stencil
// and 1.7x on the banded matrix at k = 8: the staged, coalesced matrix stream is worth more than the occupancy it costs.)
// (A masked batch of eight with no serial tail measured slower at full size: 431³ stencil k = 8 7.12 -> 7.49 ms, banded 1.16 -> 1.42 ms.)
template <int MODE, int CPL>
__device__ __forceinline__ void row_sum(const int32_t *s_col, const double *s_val, int a, int b, const double *__restrict__ X, long long ldx, int j,
                                        bool live0, bool live1, double &s0, double &s1)
{
    int p = a;
    for (; p + 4 <= b; p += 4) {
        double x0[4], x1[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = s_val[p + u];
            load2<MODE>(X, s_col[p + u], j, ldx, live0, CPL == 2 && live1, x0[u], x1[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s0 += v[u] * x0[u];
            if (CPL == 2) s1 += v[u] * x1[u];
        }
    }
    for (; p < b; ++p) {
        double x0, x1;
        const double v = s_val[p];
        load2<MODE>(X, s_col[p], j, ldx, live0, CPL == 2 && live1, x0, x1);
        s0 += v * x0;
        if (CPL == 2) s1 += v * x1;
    }
}

template <int KT, int MODE>
__global__ __launch_bounds__(WG) void spmm_csr_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colids, const double *__restrict__ values,
    const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int k,
    const int4 *__restrict__ blocks, const LongChunk *__restrict__ chunks, int n_chunks, double *__restrict__ partials, int kmax,
    double alpha, double beta)
{
    constexpr int CPL = KT >= 2 ? 2 : 1;   // columns per lane
    constexpr int G = KT / CPL;            // lanes per row
    constexpr int NG = WG / G;             // row groups per workgroup
    __shared__ int32_t s_col[TILE_NNZ];
    __shared__ double s_val[TILE_NNZ];
    __shared__ int32_t s_rp[TILE_ROWS + 1];
    __shared__ double s_part[NG * KT];

    const int tid = (int)threadIdx.x, g = tid / G, l = tid % G;
    const int j = (int)blockIdx.y * KT + l * CPL;                   // the lane's first column
    const bool live0 = j < k, live1 = CPL == 2 && j + 1 < k;

    if ((int)blockIdx.x < n_chunks) {
        // ---- one chunk of a long row: contiguous pieces per group, the pieces' sums added in group order
        const LongChunk c = chunks[blockIdx.x];
        const int n = c.k1 - c.k0;
        for (int i = tid; i < n; i += WG) {
            s_col[i] = __builtin_nontemporal_load(colids + c.k0 + i);
            s_val[i] = __builtin_nontemporal_load(values + c.k0 + i);
        }
        __syncthreads();
        const int per = (n + NG - 1) / NG, a = min(n, g * per), b = min(n, a + per);
        double s0 = 0.0, s1 = 0.0;
        row_sum<MODE, CPL>(s_col, s_val, a, b, X, ldx, j, live0, live1, s0, s1);
        s_part[g * KT + l * CPL] = s0;
        if (CPL == 2) s_part[g * KT + l * CPL + 1] = s1;
        __syncthreads();
        if (tid < KT) {
            const int jj = (int)blockIdx.y * KT + tid;
            if (jj < k) {
                double s = 0.0;
                for (int q = 0; q < NG; ++q) s += s_part[q * KT + tid];
                partials[(long long)c.slot * kmax + jj] = s;
            }
        }
        return;
    }

    // ---- a row-aligned block of the streaming plan
    const int4 blk = blocks[(int)blockIdx.x - n_chunks];              // {row0, nrows, k0, nnz}
    const int r0 = blk.x, nrows = blk.y, k0 = blk.z, nnzb = blk.w;
    for (int r = tid; r <= nrows; r += WG) s_rp[r] = __builtin_nontemporal_load(rowptr + r0 + r) - k0;
    for (int i = tid; i < nnzb; i += WG) {
        s_col[i] = __builtin_nontemporal_load(colids + k0 + i);
        s_val[i] = __builtin_nontemporal_load(values + k0 + i);
    }
    __syncthreads();
    for (int r = g; r < nrows; r += NG) {
        double s0 = 0.0, s1 = 0.0;
        row_sum<MODE, CPL>(s_col, s_val, s_rp[r], s_rp[r + 1], X, ldx, j, live0, live1, s0, s1);
        store2<MODE>(Y, r0 + r, j, ldy, live0, live1, s0, s1, alpha, beta);
    }
}

// Rows longer than a block: per (long row, column) the chunk partials in chunk order, then alpha / beta.
template <int MODE>
__global__ void spmm_long_fixup_kernel(const LongRow *__restrict__ long_rows, int n_long, int k, const double *__restrict__ partials, int kmax,
                                       double *__restrict__ Y, long long ldy, double alpha, double beta)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_long * k) return;
    const int i = (int)(t / k), jj = (int)(t % k);
    const LongRow lr = long_rows[i];
    double s = 0.0;
    for (int q = 0; q < lr.nslots; ++q) s += partials[(long long)(lr.slot0 + q) * kmax + jj];
    double *p = Y + at<MODE == 2 ? 2 : 1>(lr.row, jj, ldy);
    *p = combine(s, alpha, beta, beta != 0.0 ? *p : 0.0);
}

template <int KT, int MODE>
void launch_tiles(const g4s_csr_s &A, const double *X, long long ldx, double *Y, long long ldy, int k, double *partials, int kmax,
                  double alpha, double beta, hipStream_t s)
{
    const g4s::StreamPlan &P = A.stream;
    const dim3 grid((unsigned)(P.n_chunks + P.n_stream), (unsigned)((k + KT - 1) / KT)), block(WG);
    hipLaunchKernelGGL((spmm_csr_kernel<KT, MODE>), grid, block, 0, s, A.d_rowptr, A.d_colids, A.d_values, X, ldx, Y, ldy, k, P.blocks.as<int4>(),
                       P.chunks.as<LongChunk>(), P.n_chunks, partials, kmax, alpha, beta);
}

template <int MODE>
void launch_mode(const g4s_csr_s &A, const double *X, long long ldx, double *Y, long long ldy, int k, double *partials, int kmax,
                 double alpha, double beta, hipStream_t s)
{
    // the smallest tile that holds k (at most 32); larger k is covered by tiles along the grid's y dimension, the last one masked
    if (k <= 1) launch_tiles<1, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    else if (k <= 2) launch_tiles<2, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    else if (k <= 4) launch_tiles<4, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    else if (k <= 8) launch_tiles<8, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    else if (k <= 16) launch_tiles<16, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    else launch_tiles<kMaxTile, MODE>(A, X, ldx, Y, ldy, k, partials, kmax, alpha, beta, s);
    if (A.stream.n_long > 0) {
        const long long n = (long long)A.stream.n_long * k;
        hipLaunchKernelGGL((spmm_long_fixup_kernel<MODE>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A.stream.long_rows.as<LongRow>(), A.stream.n_long, k,
                           partials, kmax, Y, ldy, alpha, beta);
    }
}

// Argument rules of g4s_spmm / g4s_spmm_csr_i32_f64, checked before any HIP call.
int check_args(const char *fn, int32_t rows, int32_t cols, int32_t k, const double *X, int64_t ldx, const double *Y, int64_t ldy, bool cm)
{
    if (k < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: k is negative", fn);
    if (cm) {
        if (ldx < cols) return g4s::set_error(G4S_ERR_INVALID, "%s: column-major X needs ldx >= cols (%lld < %d)", fn, (long long)ldx, cols);
        if (ldy < rows) return g4s::set_error(G4S_ERR_INVALID, "%s: column-major Y needs ldy >= rows (%lld < %d)", fn, (long long)ldy, rows);
    } else {
        if (ldx < k) return g4s::set_error(G4S_ERR_INVALID, "%s: row-major X needs ldx >= k (%lld < %d)", fn, (long long)ldx, k);
        if (ldy < k) return g4s::set_error(G4S_ERR_INVALID, "%s: row-major Y needs ldy >= k (%lld < %d)", fn, (long long)ldy, k);
    }
    if (k == 0 || rows == 0) return G4S_OK;
    if (!Y) return g4s::set_error(G4S_ERR_INVALID, "%s: Y is NULL", fn);
    if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 7u) return g4s::set_error(G4S_ERR_INVALID, "%s: X and Y must be 8-byte aligned", fn);
    // the blocks' extents (in elements) must fit the address space before their end addresses are formed
    const int64_t lim = INT64_MAX / 16;
    auto extent_ok = [&](int64_t n_outer, int64_t ld, int64_t n_inner) { return n_outer <= 1 || ld <= (lim - n_inner) / (n_outer - 1); };
    if (!(cm ? extent_ok(k, ldx, cols) && extent_ok(k, ldy, rows) : extent_ok(cols, ldx, k) && extent_ok(rows, ldy, k)))
        return g4s::set_error(G4S_ERR_INVALID, "%s: a leading dimension is so large that the block does not fit the address space", fn);
    if (cols > 0) {
        if (!X) return g4s::set_error(G4S_ERR_INVALID, "%s: X is NULL", fn);
        // [first, last] element of each block; overlapping address ranges are refused
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), y0 = reinterpret_cast<uintptr_t>(Y);
        const uintptr_t x1 = x0 + 8u * (uintptr_t)(cm ? (int64_t)(k - 1) * ldx + (cols - 1) : (int64_t)(cols - 1) * ldx + (k - 1));
        const uintptr_t y1 = y0 + 8u * (uintptr_t)(cm ? (int64_t)(k - 1) * ldy + (rows - 1) : (int64_t)(rows - 1) * ldy + (k - 1));
        if (x0 <= y1 && y0 <= x1) return g4s::set_error(G4S_ERR_INVALID, "%s: the address ranges of X and Y overlap", fn);
    }
    return G4S_OK;
}

} // namespace

namespace g4s {
struct SpmmWork {
    int kmax = 0;
    DevBuf partials;   // n_chunks × kmax doubles
};
void spmm_work_destroy(SpmmWork *w) { delete w; }
long long spmm_work_bytes(const SpmmWork *w) { return w ? (long long)w->partials.bytes : 0; }
} // namespace g4s

namespace {
// Workspace for up to k_max vectors: the row-streaming plan (blocked-path handles) and the chunk partials. NULL stream, synchronous.
int reserve(g4s_csr_t A, int32_t k_max)
{
    G4S_TRY(g4s_csr_build_stream_plan(A));
    if (!A->spmm) {
        A->spmm = new (std::nothrow) g4s::SpmmWork();
        if (!A->spmm) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
    }
    g4s::SpmmWork *w = A->spmm;
    if (k_max <= w->kmax) return G4S_OK;
    if (A->stream.n_chunks > 0) {
        g4s::DevBuf grown;
        G4S_TRY(grown.alloc(sizeof(double) * (size_t)A->stream.n_chunks * (size_t)k_max));
        G4S_HIP_TRY(hipDeviceSynchronize());                           // the old workspace may still be in use by an earlier product
        std::swap(w->partials.p, grown.p);
        std::swap(w->partials.bytes, grown.bytes);
    }
    w->kmax = k_max;
    return G4S_OK;
}
} // namespace

G4S_API g4s_status g4s_csr_spmm_reserve(g4s_csr_t A, int32_t k_max)
{
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(k_max >= 0, "k_max is negative");
    return reserve(A, std::max(k_max, 1));
}

G4S_API g4s_status g4s_spmm(g4s_csr_t A, int32_t k, const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy, double alpha, double beta,
                            unsigned flags, void *stream)
{
    G4S_REQUIRE(A, "NULL handle");
    const bool cm = (flags & G4S_SPMM_COL_MAJOR) != 0;
    G4S_TRY(check_args("g4s_spmm", A->rows, A->cols, k, X_dev, ldx, Y_dev, ldy, cm));
    if (k == 0 || A->rows == 0) return G4S_OK;
    if (A->nnz == 0 || A->cols == 0) X_dev = nullptr;                     // nothing is gathered
    hipStream_t s = g4s::as_stream(stream);
    // one vector with unit stride: the handle's own SpMV, except on the blocked path (its LDS atomics are not reproducible run to run)
    if (k == 1 && !A->pb && (cm || (ldx == 1 && ldy == 1))) return g4s_spmv(A, X_dev, Y_dev, alpha, beta, stream);

    if (!A->spmm || k > A->spmm->kmax) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        G4S_HIP_TRY(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return g4s::set_error(G4S_ERR_INVALID, "g4s_spmm: the handle has no workspace for k = %d and the stream is capturing; call g4s_csr_spmm_reserve before the capture", k);
        G4S_TRY(reserve(A, k));
    }
    if (A->stream.n_stream + A->stream.n_chunks == 0) return G4S_OK;
    double *partials = A->spmm->partials.as<double>();
    const int kmax = A->spmm->kmax;
    const bool pairs = !cm && k >= 2 && ((reinterpret_cast<uintptr_t>(X_dev) | reinterpret_cast<uintptr_t>(Y_dev)) & 15u) == 0 && (ldx % 2) == 0 && (ldy % 2) == 0;
    if (cm) launch_mode<2>(*A, X_dev, ldx, Y_dev, ldy, k, partials, kmax, alpha, beta, s);
    else if (pairs) launch_mode<0>(*A, X_dev, ldx, Y_dev, ldy, k, partials, kmax, alpha, beta, s);
    else launch_mode<1>(*A, X_dev, ldx, Y_dev, ldy, k, partials, kmax, alpha, beta, s);
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

G4S_API g4s_status g4s_spmm_csr_i32_f64(int32_t rows, int32_t cols, int32_t k, const int32_t *rowptr, const int32_t *colids, const double *values,
                                        const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta, unsigned flags)
{
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    const bool cm = (flags & G4S_SPMM_COL_MAJOR) != 0, dev = (flags & G4S_DEVICE_POINTERS) != 0;
    G4S_TRY(check_args("g4s_spmm_csr_i32_f64", rows, cols, k, X, ldx, Y, ldy, cm));
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    if (k == 0 || rows == 0) return G4S_OK;
    const unsigned cflags = flags & (G4S_DEVICE_POINTERS | G4S_SPMV_BLOCKED | G4S_SPMV_NO_NT);
    if (dev)
        return g4s::csr_one_shot(rows, cols, rowptr, colids, values, cflags, X, 0, Y, 0, false, [&](g4s_csr_t A, const double *dx, double *dy) {
            return g4s_spmm(A, k, dx, ldx, dy, ldy, alpha, beta, flags & G4S_SPMM_COL_MAJOR, nullptr);
        });
    // host blocks are packed into compact device blocks (ld = k row-major, rows / cols column-major) and only the rows × k block of Y comes back
    const size_t nx = (size_t)cols * (size_t)k, ny = (size_t)rows * (size_t)k;
    std::vector<double> hx(nx), hy(ny);
    auto pack = [&](const double *M, int64_t ld, int32_t n, double *out) {
        for (int32_t i = 0; i < n; ++i)
            for (int32_t j = 0; j < k; ++j) out[cm ? (size_t)i + (size_t)j * n : (size_t)i * k + j] = M[cm ? i + (int64_t)j * ld : (int64_t)i * ld + j];
    };
    if (cols > 0) pack(X, ldx, cols, hx.data());
    if (beta != 0.0) pack(Y, ldy, rows, hy.data());
    G4S_TRY(g4s::csr_one_shot(rows, cols, rowptr, colids, values, cflags, hx.data(), nx, hy.data(), ny, beta != 0.0, [&](g4s_csr_t A, const double *dx, double *dy) {
        return g4s_spmm(A, k, dx, cm ? std::max(cols, 1) : k, dy, cm ? rows : k, alpha, beta, flags & G4S_SPMM_COL_MAJOR, nullptr);
    }));
    for (int32_t i = 0; i < rows; ++i)
        for (int32_t j = 0; j < k; ++j) Y[cm ? i + (int64_t)j * ldy : (int64_t)i * ldy + j] = hy[cm ? (size_t)i + (size_t)j * rows : (size_t)i * k + j];
    return G4S_OK;
}
