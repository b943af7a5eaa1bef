// csr.hip — the CSR handle of include/g4s.h (g4s_csr_t): its life cycle, the choice of its SpMV path and the dispatch of a product to that path.
//
// A handle holds the matrix on the device and the plan of one of four SpMV paths, each a module of its own with the same interface (build, update_values,
// destroy, bytes, spmv): row-streaming (spmv.hip, spmv_stream.hpp), propagation-blocked (spmv_pb.hip), diagonal (spmv_dia.hip), block-row (spmv_bcsr.hip).
// g4s_spmm (spmm.hip), the transposed products (transpose.hip), the traversals (traverse.hip), PageRank (pagerank.hip) and betweenness centrality (betweenness.hip) work on the same handle through csr_handle.hpp. Nothing device-side lives here but the
// column range check of g4s_csr_create.
#include "csr_handle.hpp"
#include <new>
#include <vector>

namespace {

// flag |= 1 if any column index is outside [0, cols): an out-of-range gather would fault the GPU.
__global__ void check_colids_kernel(const int32_t *__restrict__ colids, int64_t nnz, int32_t cols, int *flag)
{
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = colids[k];
        bad |= (c < 0) | (c >= cols);
    }
    if (bad) atomicOr(flag, 1);
}

void release(g4s_csr_s *A)
{
    if (!A) return;
    if (A->owns) {
        (void)hipFree((void *)A->d_rowptr);
        (void)hipFree((void *)A->d_colids);
        (void)hipFree((void *)A->d_values);
    }
    g4s::pb_destroy(A->pb);
    g4s::dia_destroy(A->dia);
    g4s::bcsr_destroy(A->bcsr);
    g4s::spmm_work_destroy(A->spmm);
    g4s::transpose_work_destroy(A->tr);
    g4s::traverse_work_destroy(A->trv);
    g4s::pagerank_work_destroy(A->prk);
    g4s::betweenness_work_destroy(A->bc);
    delete A;                                                       // the row-streaming plan frees its own buffers
}

int check_rowptr_device(g4s_csr_s *A)
{
    if (!A->rowptr_checked) G4S_TRY(g4s::stream_check_rowptr_device(A->rows, A->nnz, A->d_rowptr));
    A->rowptr_checked = true;
    return G4S_OK;
}

} // namespace

int g4s::csr_spmv_path(const g4s_csr_s *A) { return A->pb ? 1 : (A->dia ? 3 : (A->bcsr ? 4 : 0)); }

int g4s_csr_build_stream_plan(g4s_csr_t A)
{
    G4S_REQUIRE(A, "NULL handle");
    if (A->stream.built) return G4S_OK;
    G4S_TRY(check_rowptr_device(A));
    return g4s::stream_build_device(&A->stream, A->rows, A->nnz, A->d_rowptr);
}

G4S_API g4s_status g4s_csr_create(g4s_csr_t *out, int32_t rows, int32_t cols, int64_t nnz,
                                  const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags)
{
    G4S_REQUIRE(out, "out is NULL");
    *out = nullptr;
    G4S_REQUIRE(rows >= 0 && cols >= 0 && nnz >= 0, "negative dimension");
    G4S_REQUIRE(nnz <= INT32_MAX, "nnz exceeds the int32 index type of the reference (mm/inc/define.h:14)");
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    G4S_REQUIRE(nnz == 0 || (colids && values), "colids/values NULL with nnz > 0");
    int ndev = 0;
    G4S_HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return g4s::set_error(G4S_ERR_HIP, "no HIP device");

    // the create's scratch requests (scans, flags) come from a per-call arena, not from the stream-ordered pool: the pool's first use in a process creates it — 3 ms
    // in the middle of the first create (round 5); everything the plan KEEPS is allocated on its own
    struct CreateArena { CreateArena() { g4s::arena_enter(); } ~CreateArena() { g4s::arena_leave(nullptr, false); } } create_arena;
    g4s_csr_s *A = new (std::nothrow) g4s_csr_s();
    if (!A) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
    A->rows = rows; A->cols = cols; A->nnz = nnz;
    A->flags = flags;
    A->use_nt = !(flags & G4S_SPMV_NO_NT);

    std::vector<int32_t> h_rowptr_copy;
    const int32_t *h_rowptr = nullptr;
    int st = G4S_OK;
    auto fail = [&](int code) { release(A); return code; };

    // Row pointers that live on the device are planned there once the matrix is large (G4S_PLAN_HOST forces the host builder, G4S_PLAN_DEVICE
    // the device one at any size: the tests compare the two).
    const bool plan_on_device = (flags & G4S_DEVICE_POINTERS) && !getenv("G4S_PLAN_HOST") && (rows >= (1 << 18) || getenv("G4S_PLAN_DEVICE")) && rows > 0;
    if (flags & G4S_DEVICE_POINTERS) {
        A->d_rowptr = rowptr; A->d_colids = colids; A->d_values = values; A->owns = false;
        if (!plan_on_device) {
            h_rowptr_copy.resize((size_t)rows + 1);
            if (hipMemcpy(h_rowptr_copy.data(), rowptr, sizeof(int32_t) * ((size_t)rows + 1), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(g4s::set_error(G4S_ERR_HIP, "g4s_csr_create: D2H copy of rowptr failed"));
            h_rowptr = h_rowptr_copy.data();
        }
    } else {
        A->owns = true;
        void *p = nullptr;
        if (g4s::device_malloc(&p, sizeof(int32_t) * ((size_t)rows + 1)) != hipSuccess) return fail(g4s::set_error(G4S_ERR_NOMEM, "hipMalloc rowptr"));
        A->d_rowptr = (const int32_t *)p;
        if (g4s::device_malloc(&p, sizeof(int32_t) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(g4s::set_error(G4S_ERR_NOMEM, "hipMalloc colids"));
        A->d_colids = (const int32_t *)p;
        if (g4s::device_malloc(&p, sizeof(double) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(g4s::set_error(G4S_ERR_NOMEM, "hipMalloc values"));
        A->d_values = (const double *)p;
        if (hipMemcpy((void *)A->d_rowptr, rowptr, sizeof(int32_t) * ((size_t)rows + 1), hipMemcpyHostToDevice) != hipSuccess ||
            (nnz && hipMemcpy((void *)A->d_colids, colids, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice) != hipSuccess) ||
            (nnz && hipMemcpy((void *)A->d_values, values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice) != hipSuccess))
            return fail(g4s::set_error(G4S_ERR_HIP, "g4s_csr_create: H2D upload failed"));
        h_rowptr = rowptr;
    }

    // The row-streaming plan of a LARGE device-resident matrix waits for the path choice below (round 5): a matrix that takes the blocked path never runs it,
    // and its two plan_walk launches were 3 ms of every create on configs[1]. Only the row-pointer checks every builder relies on run here.
    st = plan_on_device ? check_rowptr_device(A) : g4s::stream_build(&A->stream, rows, nnz, h_rowptr);
    if (st != G4S_OK) return fail(st);

    // Column range check on the device copy (an out-of-range gather is a GPU fault, not an error code).
    if (nnz > 0) {
        g4s::DevBuf flag;
        int h_flag = 0;
        if (flag.alloc(sizeof(int)) != G4S_OK) return fail(G4S_ERR_NOMEM);
        (void)hipMemset(flag.p, 0, sizeof(int));
        int grid = (int)((nnz + 255) / 256 < 4096 ? (nnz + 255) / 256 : 4096);
        hipLaunchKernelGGL(check_colids_kernel, dim3(grid), dim3(256), 0, 0, A->d_colids, nnz, cols, flag.as<int>());
        hipError_t e = hipMemcpy(&h_flag, flag.p, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(g4s::set_error(G4S_ERR_HIP, "g4s_csr_create: column check failed: %s", hipGetErrorString(e)));
        if (h_flag) return fail(g4s::set_error(G4S_ERR_INVALID, "g4s_csr_create: a column index is outside [0, cols)"));
    }
    // Path choice: the row-streaming kernel unless the x gathers have no locality (or the caller forces one).
    const bool want_pb = (flags & G4S_SPMV_BLOCKED) || (!(flags & G4S_SPMV_STREAM) && g4s::pb_should_use(rows, cols, nnz, A->d_colids));
    if (want_pb && nnz > 0) {
        st = g4s::pb_build(&A->pb, rows, cols, nnz, A->d_rowptr, A->d_colids, A->d_values, (flags & G4S_SPMV_UPDATABLE) != 0);
        if (st != G4S_OK && (flags & G4S_SPMV_BLOCKED)) return fail(st);   // auto mode falls back to the streaming path
    }
    if (!A->pb && !A->stream.built) {
        st = g4s_csr_build_stream_plan(A);
        if (st != G4S_OK) return fail(st);
    }
    // stencil / banded matrices: the index-free diagonal form (not when the caller forces the CSR kernels)
    if (!A->pb && !(flags & G4S_SPMV_STREAM) && nnz > 0) {
        st = g4s::dia_try_build(&A->dia, rows, cols, nnz, A->d_rowptr, A->d_colids, A->d_values, A->use_nt);
        if (st != G4S_OK) return fail(st);
    }
    // assembled FE matrices (aligned b×b blocks, b rows with one column list): one block-column id per block instead of b² column ids
    if (!A->pb && !A->dia && !(flags & G4S_SPMV_STREAM) && nnz > 0) {
        st = g4s::bcsr_try_build(&A->bcsr, rows, cols, nnz, A->d_rowptr, A->d_colids, A->d_values, A->use_nt);
        if (st != G4S_OK) return fail(st);
    }
    *out = A;
    return G4S_OK;
}

// New values, same pattern (citcoms/lib/Drive_solvers.c:88,134 → construct_stiffness_B_matrix, Construct_arrays.c:740: the stiffness matrix is rebuilt
// before every Stokes solve and inside the viscosity iteration). The CSR array is replaced (owned copy: copied into; borrowed: the handle borrows the new
// array), then whatever the plan keeps of the values in another order is refreshed on `stream`: the regrouped producer stream of the blocked path (one
// gather pass through its value map), the diagonals, the block-major copy; the row-streaming kernel reads the CSR array itself.
namespace {
int update_values(g4s_csr_s *A, const double *values, unsigned flags, void *stream)
{
    if (A->nnz == 0) return G4S_OK;
    hipStream_t s = g4s::as_stream(stream);
    const bool dev = (flags & G4S_DEVICE_POINTERS) != 0;
    if (values && values != A->d_values) {
        if (A->owns) {
            G4S_HIP_TRY(hipMemcpyAsync(const_cast<double *>(A->d_values), values, sizeof(double) * (size_t)A->nnz, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        } else {
            G4S_REQUIRE(dev, "the handle borrows device arrays: new values must be a device array too (it is borrowed from here on)");
            A->d_values = values;
        }
    }
    if (A->pb) {
        if (g4s::pb_has_value_map(A->pb)) return g4s::pb_update_values(A->pb, A->d_values, s);
        // created without G4S_SPMV_UPDATABLE: the regrouping is done again (the cost of a create, on the NULL stream like a create)
        G4S_HIP_TRY(hipStreamSynchronize(s));
        g4s::pb_destroy(A->pb);
        A->pb = nullptr;
        const int st = g4s::pb_build(&A->pb, A->rows, A->cols, A->nnz, A->d_rowptr, A->d_colids, A->d_values, false);
        if (st != G4S_OK) {                                         // no blocked plan any more: the handle must still multiply — the row-streaming plan, built now if it never was
            G4S_TRY(g4s_csr_build_stream_plan(A));
        }
        return st;
    }
    if (A->dia) return g4s::dia_update_values(A->dia, A->d_values, s);
    if (A->bcsr) return g4s::bcsr_update_values(A->bcsr, A->d_colids, A->d_values, s);
    return G4S_OK;
}
} // namespace

// A transpose, where one exists, follows on the same stream (one gather through its entry map from the handle's current array, then its own
// handle's update), also after a failed regrouping above: the CSR array has been replaced by then.
G4S_API g4s_status g4s_csr_update_values(g4s_csr_t A, const double *values, unsigned flags, void *stream)
{
    G4S_REQUIRE(A, "NULL handle");
    int st = update_values(A, values, flags, stream);
    g4s::traverse_values_changed(A->trv);
    g4s::pagerank_values_changed(A->prk);
    g4s::betweenness_values_changed(A->bc);
    if (A->tr) {
        const int st2 = g4s::transpose_update_values(A->tr, A->d_values, g4s::as_stream(stream));
        if (st == G4S_OK) st = st2;
    }
    return st;
}

G4S_API g4s_status g4s_csr_destroy(g4s_csr_t A)
{
    release(A);
    return G4S_OK;
}

G4S_API g4s_status g4s_csr_get_info(g4s_csr_t A, g4s_csr_info *info)
{
    G4S_REQUIRE(A && info, "NULL argument");
    info->rows = A->rows; info->cols = A->cols; info->nnz = A->nnz;
    info->stream_blocks = A->stream.n_stream; info->long_rows = A->stream.n_long; info->long_chunks = A->stream.n_chunks;
    info->tile_nnz = g4s::TILE_NNZ; info->tile_rows = g4s::TILE_ROWS; info->long_chunk_nnz = g4s::LONG_CHUNK;
    info->algorithmic_bytes = 12 * A->nnz + 4 * ((int64_t)A->rows + 1) + 8 * (int64_t)A->rows + 8 * (int64_t)A->cols;
    // every part knows its own size; a transpose's bytes are added by g4s_csr_transpose_info
    info->plan_bytes = A->stream.bytes() + g4s::pb_bytes(A->pb) + g4s::dia_bytes(A->dia) + g4s::bcsr_bytes(A->bcsr) + g4s::spmm_work_bytes(A->spmm) +
                       g4s::traverse_work_bytes(A->trv) + g4s::pagerank_work_bytes(A->prk) + g4s::betweenness_work_bytes(A->bc);
    info->spmv_path = g4s::csr_spmv_path(A);
    return G4S_OK;
}

G4S_API g4s_status g4s_csr_device_arrays(g4s_csr_t A, const int32_t **rowptr, const int32_t **colids, const double **values)
{
    G4S_REQUIRE(A, "NULL handle");
    if (rowptr) *rowptr = A->d_rowptr;
    if (colids) *colids = A->d_colids;
    if (values) *values = A->d_values;
    return G4S_OK;
}

namespace {
// One product on the handle's path. semiring: a G4S_SEMIRING_* value (plus-times: alpha, beta as in g4s_spmv; the others: alpha = 1, beta = 0 or 1).
int spmv_on_path(g4s_csr_s *A, const double *x, double *y, unsigned semiring, double alpha, double beta, hipStream_t s)
{
    if (A->pb) return g4s::pb_spmv(A->pb, x, y, semiring, alpha, beta, s);
    if (A->bcsr) return g4s::bcsr_spmv(A->bcsr, x, y, semiring, alpha, beta, s);
    if (A->dia) return g4s::dia_spmv(A->dia, x, y, semiring, alpha, beta, s);
    return g4s::stream_spmv(A->stream, A->d_rowptr, A->d_colids, A->d_values, A->use_nt, x, y, semiring, alpha, beta, s);
}
} // namespace

int g4s::check_spmv_args(const char *fn, const g4s_csr_s *A, int32_t n_out, const double *x, const double *y)
{
    if (n_out == 0) return G4S_OK;
    const char *what = !y ? "y is NULL" : (!x && A->nnz != 0) ? "x is NULL" : (const void *)x == (const void *)y ? "x and y must not alias" : nullptr;
    return what ? set_error(G4S_ERR_INVALID, "%s: %s", fn, what) : (int)G4S_OK;
}

G4S_API g4s_status g4s_spmv(g4s_csr_t A, const double *x_dev, double *y_dev, double alpha, double beta, void *stream)
{
    G4S_REQUIRE(A, "NULL handle");
    G4S_TRY(g4s::check_spmv_args(__func__, A, A->rows, x_dev, y_dev));
    if (A->rows == 0) return G4S_OK;
    return spmv_on_path(A, x_dev, y_dev, G4S_SEMIRING_PLUS_TIMES, alpha, beta, g4s::as_stream(stream));
}

// y := A ⊗ x or y ⊕ (A ⊗ x) over a semiring (include/g4s.h): the kernels of g4s_spmv, instantiated for the policy the flags select; plus-times IS g4s_spmv.
G4S_API g4s_status g4s_spmv_semiring(g4s_csr_t A, const double *x_dev, double *y_dev, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_SEMIRING_MASK | G4S_SPMV_ACCUMULATE)) == 0u, "g4s_spmv_semiring: flags other than G4S_SEMIRING_* | G4S_SPMV_ACCUMULATE");
    G4S_REQUIRE(A, "NULL handle");
    G4S_TRY(g4s::check_spmv_args(__func__, A, A->rows, x_dev, y_dev));
    if (A->rows == 0) return G4S_OK;
    return spmv_on_path(A, x_dev, y_dev, flags & G4S_SEMIRING_MASK, 1.0, (flags & G4S_SPMV_ACCUMULATE) ? 1.0 : 0.0, g4s::as_stream(stream));
}

int g4s::csr_one_shot(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags,
                      const double *x, size_t nx, double *y, size_t ny, bool read_y, const std::function<int(g4s_csr_t, const double *, double *)> &product)
{
    const bool dev = (flags & G4S_DEVICE_POINTERS) != 0;
    int32_t nnz32 = 0;
    if (dev) G4S_HIP_TRY(hipMemcpy(&nnz32, rowptr + rows, sizeof(int32_t), hipMemcpyDeviceToHost));
    else nnz32 = rowptr[rows];
    G4S_REQUIRE(nnz32 >= 0, "rowptr[rows] is negative");
    g4s_csr_t A = nullptr;
    // one call, one product: the blocked path's regrouping (tens of ms) cannot pay off — stay on the streaming path unless asked
    if (!(flags & G4S_SPMV_BLOCKED)) flags |= G4S_SPMV_STREAM;
    G4S_TRY(g4s_csr_create(&A, rows, cols, nnz32, rowptr, colids, values, flags));
    int st = G4S_OK;
    if (dev) {
        st = product(A, x, y);
        if (st == G4S_OK && hipStreamSynchronize(nullptr) != hipSuccess) st = set_error(G4S_ERR_HIP, "synchronize failed");
    } else {
        DevBuf dx, dy;
        if (dx.alloc(sizeof(double) * nx) != G4S_OK || dy.alloc(sizeof(double) * ny) != G4S_OK) {
            st = G4S_ERR_NOMEM;
        } else if ((nx && hipMemcpy(dx.p, x, sizeof(double) * nx, hipMemcpyHostToDevice) != hipSuccess) ||
                   (read_y && hipMemcpy(dy.p, y, sizeof(double) * ny, hipMemcpyHostToDevice) != hipSuccess)) {
            st = set_error(G4S_ERR_HIP, "H2D copy of x/y failed");
        } else {
            st = product(A, dx.as<double>(), dy.as<double>());
            if (st == G4S_OK && hipMemcpy(y, dy.p, sizeof(double) * ny, hipMemcpyDeviceToHost) != hipSuccess)
                st = set_error(G4S_ERR_HIP, "D2H copy of y failed");
        }
    }
    g4s_csr_destroy(A);
    return st;
}

G4S_API g4s_status g4s_spmv_semiring_csr_i32_f64(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids, const double *values,
                                                 const double *x, double *y, unsigned flags)
{
    constexpr unsigned kPathFlags = G4S_DEVICE_POINTERS | G4S_SPMV_BLOCKED | G4S_SPMV_STREAM;
    G4S_REQUIRE((flags & ~(kPathFlags | G4S_SEMIRING_MASK | G4S_SPMV_ACCUMULATE)) == 0u,
                "g4s_spmv_semiring_csr_i32_f64: flags other than G4S_SEMIRING_* | G4S_SPMV_ACCUMULATE | pointer kind | G4S_SPMV_BLOCKED / G4S_SPMV_STREAM");
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    if (rows == 0) return G4S_OK;
    G4S_REQUIRE(y, "y is NULL");
    G4S_REQUIRE(x || cols == 0, "x is NULL");
    G4S_REQUIRE((const void *)x != (const void *)y, "x and y must not alias");
    const unsigned op = flags & (G4S_SEMIRING_MASK | G4S_SPMV_ACCUMULATE);
    return g4s::csr_one_shot(rows, cols, rowptr, colids, values, flags & kPathFlags, x, (size_t)cols, y, (size_t)rows, (flags & G4S_SPMV_ACCUMULATE) != 0,
                             [op](g4s_csr_t A, const double *dx, double *dy) { return g4s_spmv_semiring(A, dx, dy, op, nullptr); });
}

G4S_API g4s_status g4s_spmv_csr_i32_f64(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids,
                                        const double *values, const double *x, double *y,
                                        double alpha, double beta, unsigned flags)
{
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    if (rows == 0) return G4S_OK;
    G4S_REQUIRE(y, "y is NULL");
    return g4s::csr_one_shot(rows, cols, rowptr, colids, values, flags, x, (size_t)cols, y, (size_t)rows, beta != 0.0,
                             [alpha, beta](g4s_csr_t A, const double *dx, double *dy) { return g4s_spmv(A, dx, dy, alpha, beta, nullptr); });
}
