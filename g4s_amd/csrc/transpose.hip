// transpose.hip — Aᵀ of a CSR matrix on the device (include/g4s.h, g4s_csr_transpose) and the transposed products of a handle
// (g4s_csr_transpose_reserve, g4s_spmv_transpose, g4s_spmv_semiring_transpose).
//
// The reference converts between the two layouts on the host (mm/inc/CSR.h:171-230, CSR(const CSC&) and CSR(const CSC&, bool transpose);
// mm/inc/convert.h). Here every step runs on the device, on the call's stream:
//   1. tr_check_rowptr_kernel / tr_key_kernel — rowptr zero-based, non-decreasing and ending at nnz, every column in [0, cols); per entry the sort key
//      cols − 1 − col and the payload k; per column its count (integer atomics: the same counts whatever the order). One read-back of the failure flag
//      before anything is written by row or by column.
//   2. prims::exclusive_scan over the cols + 1 counts (the last one 0) → trowptr.
//   3. tr_rows_kernel — the row of every entry. One workgroup per 256 rows, their row pointers in LDS, a strided pass over the rows' entries: a hub row of
//      1e5 entries is a loop of a workgroup, not of one lane. A lane finds its row by a binary search in LDS that starts at the row of its previous entry.
//   4. prims::sort_pairs_descending on (key, k): ascending column, and stable, so the entries of one column keep their entry order → perm.
//   5. tr_gather_kernel — tcolids[k] = row[perm[k]], tvalues[k] = values[perm[k]].
// Nothing depends on timing: the outputs are the same bits on every run.
// g4s_csr_row_indices is steps 1 (the row pointers only) and 3 alone: the row of every entry, the array a CSR lacks to be a COO (coo.hip is the way back).
//
// A handle's transpose (TransposeWork) holds the arrays of Aᵀ, perm and an inner handle of Aᵀ created from them with A's path flags. The transposed
// products are the inner handle's g4s_spmv / g4s_spmv_semiring, and g4s_csr_update_values of A refreshes it with one gather through perm.
#include "common.hpp"
#include "prims.hpp"
#include "csr_handle.hpp"
#include "readback.hpp"
#include "call_util.hpp"
#include <algorithm>
#include <new>

namespace {

constexpr int WG = 256;
constexpr long long kMaxGrid = 16384;   // grid-stride kernels: at most 64 workgroups per CU of the 256


// fail bit 1: rowptr[0] != 0, rowptr[rows] != nnz or a decrease
__global__ __launch_bounds__(WG) void tr_check_rowptr_kernel(int rows, long long nnz, const int32_t *__restrict__ rowptr, int *__restrict__ fail)
{
    for (long long r = (long long)blockIdx.x * WG + threadIdx.x; r <= rows; r += (long long)gridDim.x * WG) {
        const int v = rowptr[r];
        if ((r == 0 && v != 0) || (r == rows && (long long)v != nnz) || (r < rows && rowptr[r + 1] < v)) atomicOr(fail, 1);
    }
}

// fail bit 2: a column outside [0, cols) (it is neither counted nor given a key that the sort could misplace)
__global__ __launch_bounds__(WG) void tr_key_kernel(long long nnz, int cols, const int32_t *__restrict__ colids, int *__restrict__ keys, int *__restrict__ idx,
                                                    int *__restrict__ counts, int *__restrict__ fail)
{
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) {
        const int c = colids[k];
        if ((unsigned)c < (unsigned)cols) {
            keys[k] = cols - 1 - c;
            atomicAdd(counts + c, 1);
        } else {
            keys[k] = 0;
            atomicOr(fail, 2);
        }
        idx[k] = (int)k;
    }
}

__global__ __launch_bounds__(WG) void tr_rows_kernel(int rows, const int32_t *__restrict__ rowptr, int *__restrict__ row_of)
{
    __shared__ int rp[WG + 1];
    const int r0 = (int)blockIdx.x * WG, nr = min(WG, rows - r0);
    for (int i = threadIdx.x; i <= nr; i += WG) rp[i] = rowptr[r0 + i];
    __syncthreads();
    const long long k1 = rp[nr];
    int lo = 0;                                                     // the last row i with rp[i] <= k: never decreases as k grows
    for (long long k = rp[0] + (long long)threadIdx.x; k < k1; k += WG) {
        int hi = nr - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rp[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        row_of[k] = r0 + lo;
    }
}

template <bool VALUES>
__global__ __launch_bounds__(WG) void tr_gather_kernel(long long nnz, const int *__restrict__ perm, const int *__restrict__ row_of, const double *__restrict__ values,
                                                       int32_t *__restrict__ tcolids, double *__restrict__ tvalues)
{
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) {
        const int p = perm[k];
        tcolids[k] = row_of[p];
        if constexpr (VALUES) tvalues[k] = values[p];
    }
}

__global__ __launch_bounds__(WG) void tr_refill_kernel(long long nnz, const int *__restrict__ perm, const double *__restrict__ values, double *__restrict__ tvalues)
{
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) tvalues[k] = values[perm[k]];
}

// Device arrays in and out, on `s`, synchronous. perm (nnz ints) is required here: it is the sort's payload output. Scratch: one allocation of
// cols + 1 + 4 + 6·nnz ints (counts, flags, keys, payload, sorted keys, the sort's two ping-pong partners, the row of each entry), freed before return.
int transpose_device(int32_t rows, int32_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colids, const double *values,
                     int32_t *trowptr, int32_t *tcolids, double *tvalues, int32_t *perm, hipStream_t s)
{
    const size_t n = (size_t)nnz;
    int *scr = nullptr;
    if (g4s::device_malloc((void **)&scr, sizeof(int) * ((size_t)cols + 5 + 6 * n)) != hipSuccess)
        return g4s::set_error(G4S_ERR_NOMEM, "g4s_csr_transpose: %zu bytes of scratch", sizeof(int) * ((size_t)cols + 5 + 6 * n));
    int *counts = scr, *fail = counts + cols + 1, *keys = fail + 4, *idx = keys + n, *keys_out = idx + n, *tmp_k = keys_out + n, *tmp_v = tmp_k + n,
        *row_of = tmp_v + n;
    auto done = [&](int st) {
        const hipError_t e = hipStreamSynchronize(s);
        (void)hipFree(scr);
        if (st == G4S_OK && e != hipSuccess) st = g4s::set_error(G4S_ERR_HIP, "g4s_csr_transpose: %s", hipGetErrorString(e));
        return st;
    };
#define TR_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return done(g4s::set_error(G4S_ERR_HIP, "g4s_csr_transpose: %s: %s", #expr, hipGetErrorString(e_))); } while (0)
    TR_TRY(hipMemsetAsync(counts, 0, sizeof(int) * ((size_t)cols + 5), s));   // the counts, their trailing 0 and the flags
    hipLaunchKernelGGL(tr_check_rowptr_kernel, dim3(grid_for<WG>((long long)rows + 1, kMaxGrid)), dim3(WG), 0, s, rows, (long long)nnz, rowptr, fail);
    if (nnz > 0) hipLaunchKernelGGL(tr_key_kernel, dim3(grid_for<WG>(nnz, kMaxGrid)), dim3(WG), 0, s, (long long)nnz, cols, colids, keys, idx, counts, fail);
    TR_TRY(hipGetLastError());
    int h_fail = 0;
    TR_TRY(hipMemcpyAsync(&h_fail, fail, sizeof(int), hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));
    if (h_fail & 1) return done(g4s::set_error(G4S_ERR_INVALID, "g4s_csr_transpose: rowptr is not zero-based, non-decreasing and ending at nnz = %lld", (long long)nnz));
    if (h_fail & 2) return done(g4s::set_error(G4S_ERR_INVALID, "g4s_csr_transpose: a column index is outside [0, %d)", cols));
    int st = g4s::prims::exclusive_scan(counts, trowptr, (long long)cols + 1, s);
    if (st != G4S_OK || nnz == 0) return done(st);
    hipLaunchKernelGGL(tr_rows_kernel, dim3((unsigned)((rows + WG - 1) / WG)), dim3(WG), 0, s, rows, rowptr, row_of);
    TR_TRY(hipGetLastError());
    const int key_bits = cols > 1 ? 32 - __builtin_clz((unsigned)(cols - 1)) : 1;
    st = g4s::prims::sort_pairs_descending(keys, idx, keys_out, perm, tmp_k, tmp_v, (int)nnz, key_bits, s);
    if (st != G4S_OK) return done(st);
    if (tvalues) hipLaunchKernelGGL(tr_gather_kernel<true>, dim3(grid_for<WG>(nnz, kMaxGrid)), dim3(WG), 0, s, (long long)nnz, perm, row_of, values, tcolids, tvalues);
    else hipLaunchKernelGGL(tr_gather_kernel<false>, dim3(grid_for<WG>(nnz, kMaxGrid)), dim3(WG), 0, s, (long long)nnz, perm, row_of, values, tcolids, tvalues);
    TR_TRY(hipGetLastError());
#undef TR_TRY
    return done(G4S_OK);
}

// Device arrays, synchronous on `s`: the row-pointer check read back before tr_rows_kernel indexes by them. Two waits.
int row_indices_device(int32_t rows, int64_t nnz, const int32_t *rowptr, int32_t *row_out, hipStream_t s)
{
    BigBuf flag;
    G4S_TRY(flag.alloc(256));
    int fail = 0;
    G4S_HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(tr_check_rowptr_kernel, dim3(grid_for<WG>((long long)rows + 1, kMaxGrid)), dim3(WG), 0, s, rows, (long long)nnz, rowptr, flag.as<int>());
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(g4s::ReadScope(s).fetch(fail, flag.p));
    flag.idle = true;
    if (fail) return g4s::set_error(G4S_ERR_INVALID, "g4s_csr_row_indices: rowptr is not zero-based, non-decreasing and ending at nnz = %lld", (long long)nnz);
    if (rows > 0 && nnz > 0) {
        hipLaunchKernelGGL(tr_rows_kernel, dim3((unsigned)(((long long)rows + WG - 1) / WG)), dim3(WG), 0, s, rows, rowptr, row_out);
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(hipStreamSynchronize(s));
    }
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_row_indices(int32_t rows, int64_t nnz, const int32_t *rowptr, int32_t *row_out, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(rows >= 0 && nnz >= 0, "negative dimension or entry count");
    if (nnz > INT32_MAX) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: %lld entries exceed the int32 row pointers", __func__, (long long)nnz);
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    G4S_REQUIRE(row_out || nnz == 0, "row_out is NULL with nnz > 0");
    const size_t rp = sizeof(int32_t) * ((size_t)rows + 1), nb = sizeof(int32_t) * (size_t)nnz;
    const bool dev = flags & G4S_DEVICE_POINTERS;
    if (!dev && overlap(row_out, nb, rowptr, rp)) return g4s::set_error(G4S_ERR_INVALID, "%s: row_out overlaps rowptr", __func__);
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s));
    if (dev) return row_indices_device(rows, nnz, rowptr, row_out, s);
    Staged stage(s);
    const int32_t *d_rp = stage.in(rowptr, rp);
    int32_t *d_out = stage.out<int32_t>(nb);
    int status = stage.error();
    if (status == G4S_OK) status = row_indices_device(rows, nnz, d_rp, d_out, s);
    if (status == G4S_OK) status = stage.to_host(row_out, d_out, nb);
    if (status == G4S_OK) status = stage.wait();
    return stage.finish(status);
}

namespace {

// device_malloc of `count` elements (at least one), NULL-initialised by the caller
template <class T>
int dev_array(T **p, size_t count)
{
    if (g4s::device_malloc((void **)p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) return g4s::set_error(G4S_ERR_NOMEM, "hipMalloc of %zu bytes", sizeof(T) * count);
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_transpose(int32_t rows, int32_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colids, const double *values,
                                     int32_t *trowptr, int32_t *tcolids, double *tvalues, int32_t *perm, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(rows >= 0 && cols >= 0 && nnz >= 0, "negative dimension");
    G4S_REQUIRE(nnz <= INT32_MAX, "nnz exceeds INT32_MAX");
    G4S_REQUIRE(rowptr && trowptr, "rowptr or trowptr is NULL");
    G4S_REQUIRE(nnz == 0 || (colids && tcolids), "colids or tcolids is NULL with nnz > 0");
    G4S_REQUIRE(values || !tvalues, "tvalues without values");
    G4S_REQUIRE(tvalues || !values, "values without tvalues");
    const hipStream_t s = g4s::as_stream(stream);
    const size_t n = (size_t)nnz;
    if (flags & G4S_DEVICE_POINTERS) {
        int32_t *p = perm;
        if (!p && n) G4S_TRY(dev_array(&p, n));
        const int st = transpose_device(rows, cols, nnz, rowptr, colids, values, trowptr, tcolids, tvalues, p, s);
        if (p != perm) (void)hipFree(p);
        return st;
    }
    // host arrays: device copies of the inputs and outputs, the same steps, the outputs copied back
    int32_t *d_rp = nullptr, *d_ci = nullptr, *d_trp = nullptr, *d_tci = nullptr, *d_perm = nullptr;
    double *d_va = nullptr, *d_tva = nullptr;
    auto done = [&](int st) {
        (void)hipStreamSynchronize(s);
        for (void *q : {(void *)d_rp, (void *)d_ci, (void *)d_trp, (void *)d_tci, (void *)d_perm, (void *)d_va, (void *)d_tva}) (void)hipFree(q);
        return st;
    };
#define TRH_TRY(expr) do { const int st_ = (expr); if (st_ != G4S_OK) return done(st_); } while (0)
#define TRH_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return done(g4s::set_error(G4S_ERR_HIP, "g4s_csr_transpose: %s: %s", #expr, hipGetErrorString(e_))); } while (0)
    TRH_TRY(dev_array(&d_rp, (size_t)rows + 1));
    TRH_TRY(dev_array(&d_trp, (size_t)cols + 1));
    if (n) {
        TRH_TRY(dev_array(&d_ci, n));
        TRH_TRY(dev_array(&d_tci, n));
        TRH_TRY(dev_array(&d_perm, n));
        if (values) {
            TRH_TRY(dev_array(&d_va, n));
            TRH_TRY(dev_array(&d_tva, n));
        }
    }
    TRH_HIP(hipMemcpyAsync(d_rp, rowptr, sizeof(int32_t) * ((size_t)rows + 1), hipMemcpyHostToDevice, s));
    if (n) TRH_HIP(hipMemcpyAsync(d_ci, colids, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    if (n && values) TRH_HIP(hipMemcpyAsync(d_va, values, sizeof(double) * n, hipMemcpyHostToDevice, s));
    TRH_TRY(transpose_device(rows, cols, nnz, d_rp, d_ci, d_va, d_trp, d_tci, d_tva, d_perm, s));
    TRH_HIP(hipMemcpyAsync(trowptr, d_trp, sizeof(int32_t) * ((size_t)cols + 1), hipMemcpyDeviceToHost, s));
    if (n) TRH_HIP(hipMemcpyAsync(tcolids, d_tci, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    if (n && tvalues) TRH_HIP(hipMemcpyAsync(tvalues, d_tva, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (n && perm) TRH_HIP(hipMemcpyAsync(perm, d_perm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    TRH_HIP(hipStreamSynchronize(s));
#undef TRH_TRY
#undef TRH_HIP
    return done(G4S_OK);
}

// ------------------------------------------------------------------------------------------------ the transpose of a handle
namespace g4s {

struct TransposeWork {
    int32_t *rowptr = nullptr, *colids = nullptr, *perm = nullptr;   // Aᵀ (cols + 1, nnz) and the entry of A behind each of its slots (nnz)
    double *values = nullptr;
    g4s_csr_t inner = nullptr;                                       // the handle of Aᵀ: borrows the arrays above, which live as long as it
    int64_t nnz = 0;
    int64_t bytes = 0;                                               // the four arrays
};

void transpose_work_destroy(TransposeWork *w)
{
    if (!w) return;
    (void)g4s_csr_destroy(w->inner);
    (void)hipFree(w->rowptr);
    (void)hipFree(w->colids);
    (void)hipFree(w->perm);
    (void)hipFree(w->values);
    delete w;
}

void transpose_work_view(const TransposeWork *w, const int32_t **rowptr, const int32_t **colids, const double **values, g4s_csr_t *inner)
{
    *rowptr = w->rowptr; *colids = w->colids; *values = w->values; *inner = w->inner;
}

int transpose_update_values(TransposeWork *w, const double *values, hipStream_t s)
{
    if (w->nnz > 0) {
        hipLaunchKernelGGL(tr_refill_kernel, dim3(grid_for<WG>(w->nnz, kMaxGrid)), dim3(WG), 0, s, (long long)w->nnz, w->perm, values, w->values);
        G4S_HIP_TRY(hipGetLastError());
    }
    return g4s_csr_update_values(w->inner, w->values, G4S_DEVICE_POINTERS, s);   // the same array: only the inner plan's own copy is refreshed
}

} // namespace g4s

namespace {

constexpr unsigned kInnerFlags = G4S_SPMV_NO_NT | G4S_SPMV_BLOCKED | G4S_SPMV_STREAM | G4S_SPMV_UPDATABLE;

// §1 on the handle's device arrays, then the inner handle; NULL stream, synchronous. Nothing is kept on failure.
int reserve(g4s_csr_t A)
{
    if (A->tr) return G4S_OK;
    G4S_HIP_TRY(hipDeviceSynchronize());                           // value updates and products on other streams are complete
    g4s::TransposeWork *w = new (std::nothrow) g4s::TransposeWork();
    if (!w) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
    const size_t n = (size_t)A->nnz;
    int st = dev_array(&w->rowptr, (size_t)A->cols + 1);
    if (st == G4S_OK) st = dev_array(&w->colids, n);
    if (st == G4S_OK) st = dev_array(&w->values, n);
    if (st == G4S_OK) st = dev_array(&w->perm, n);
    if (st == G4S_OK) st = transpose_device(A->rows, A->cols, A->nnz, A->d_rowptr, A->d_colids, A->d_values, w->rowptr, w->colids, w->values, w->perm, nullptr);
    if (st == G4S_OK)
        st = g4s_csr_create(&w->inner, A->cols, A->rows, A->nnz, w->rowptr, w->colids, w->values, (A->flags & kInnerFlags) | G4S_DEVICE_POINTERS);
    if (st != G4S_OK) {
        g4s::transpose_work_destroy(w);
        return st;
    }
    w->nnz = A->nnz;
    w->bytes = 4 * ((int64_t)A->cols + 1) + 16 * A->nnz + 4 * A->nnz;
    A->tr = w;
    return G4S_OK;
}

// The checks of g4s_spmv with the two lengths swapped (the aliasing check comes before the handle is read), then the handle's transpose for a product on `s`:
// reserved now (synchronously) if it does not exist yet, refused on a capturing stream. *inner stays NULL for an empty product.
int ready(const char *fn, g4s_csr_t A, const double *x_dev, const double *y_dev, hipStream_t s, g4s_csr_t *inner)
{
    *inner = nullptr;
    if (!A) return g4s::set_error(G4S_ERR_INVALID, "%s: NULL handle", fn);
    if (x_dev && (const void *)x_dev == (const void *)y_dev) return g4s::set_error(G4S_ERR_INVALID, "%s: x and y must not alias", fn);
    G4S_TRY(g4s::check_spmv_args(fn, A, A->cols, x_dev, y_dev));
    if (A->cols == 0) return G4S_OK;
    if (!A->tr) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        G4S_HIP_TRY(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return g4s::set_error(G4S_ERR_INVALID, "%s: the handle has no transpose yet and the stream is capturing; call g4s_csr_transpose_reserve before the capture", fn);
        G4S_TRY(reserve(A));
    }
    *inner = A->tr->inner;
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_transpose_reserve(g4s_csr_t A)
{
    G4S_REQUIRE(A, "NULL handle");
    return reserve(A);
}

G4S_API g4s_status g4s_csr_transpose_info(g4s_csr_t A, g4s_csr_info *info)
{
    G4S_REQUIRE(A && info, "NULL argument");
    G4S_REQUIRE(A->tr, "the handle has no transpose: call g4s_csr_transpose_reserve first");
    G4S_TRY(g4s_csr_get_info(A->tr->inner, info));
    info->plan_bytes += A->tr->bytes;
    return G4S_OK;
}

// y(cols) = alpha·Aᵀ·x(rows) + beta·y
G4S_API g4s_status g4s_spmv_transpose(g4s_csr_t A, const double *x_dev, double *y_dev, double alpha, double beta, void *stream)
{
    g4s_csr_t inner = nullptr;
    G4S_TRY(ready(__func__, A, x_dev, y_dev, g4s::as_stream(stream), &inner));
    return inner ? g4s_spmv(inner, x_dev, y_dev, alpha, beta, stream) : G4S_OK;
}

G4S_API g4s_status g4s_spmv_semiring_transpose(g4s_csr_t A, const double *x_dev, double *y_dev, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_SEMIRING_MASK | G4S_SPMV_ACCUMULATE)) == 0u, "g4s_spmv_semiring_transpose: flags other than G4S_SEMIRING_* | G4S_SPMV_ACCUMULATE");
    g4s_csr_t inner = nullptr;
    G4S_TRY(ready(__func__, A, x_dev, y_dev, g4s::as_stream(stream), &inner));
    return inner ? g4s_spmv_semiring(inner, x_dev, y_dev, flags, stream) : G4S_OK;
}
