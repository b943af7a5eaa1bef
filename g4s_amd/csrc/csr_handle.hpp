// csr_handle.hpp — the CSR handle behind g4s_csr_t, for the files of the library that work on one: csr.hip (life cycle, SpMV), spmm.hip, transpose.hip,
// traverse.hip, pagerank.hip, betweenness.hip. The device arrays of the last three's workspaces have one owner, DevicePieces below. What
// traverse.hip and betweenness.hip share with the calls on raw CSR arrays, which have no handle (components.hip, kcore.hip, color.hip, ktruss.hip,
// scc.hip), is frontier.hpp (device) and step_batch.hpp (host).
#pragma once
#include "common.hpp"
#include "spmv_stream.hpp"
#include "spmv_pb.hpp"
#include "spmv_dia.hpp"
#include "spmv_bcsr.hpp"
#include <functional>
#include <memory>

namespace g4s {

// spmm.hip: the handle's SpMM workspace (reserved k_max, the partial sums of long-row chunks for k_max vectors)
struct SpmmWork;
void spmm_work_destroy(SpmmWork *w);
long long spmm_work_bytes(const SpmmWork *w);

// transpose.hip: the arrays of Aᵀ, the entry map perm and the inner handle of Aᵀ
struct TransposeWork;
void transpose_work_destroy(TransposeWork *w);
// tvalues[k] = values[perm[k]] on `stream`, then the inner handle's own g4s_csr_update_values (after the forward handle's update)
int transpose_update_values(TransposeWork *w, const double *values, hipStream_t stream);
// the kept arrays of Aᵀ and its inner handle (traverse.hip: the pull steps)
void transpose_work_view(const TransposeWork *w, const int32_t **rowptr, const int32_t **colids, const double **values, g4s_csr_t *inner);

// traverse.hip: the workspace of g4s_sssp / g4s_bfs (frontier queues, marks, the pull step's vector, the state block)
struct TraverseWork;
void traverse_work_destroy(TraverseWork *w);
long long traverse_work_bytes(const TraverseWork *w);
void traverse_values_changed(TraverseWork *w);   // g4s_csr_update_values: whether a stored value is zero has to be found out again

// pagerank.hip: the workspace of g4s_pagerank (1 / out-strength, x, y, the normalised teleport vector, per-workgroup partials, the state block)
struct PagerankWork;
void pagerank_work_destroy(PagerankWork *w);
long long pagerank_work_bytes(const PagerankWork *w);
void pagerank_values_changed(PagerankWork *w);   // g4s_csr_update_values: the strength pass has to run again

// betweenness.hip: the workspace of g4s_betweenness (levels, the concatenated frontiers and their starts, hub lists, σ, δ, the sum over sources, the state block)
struct BcWork;
void betweenness_work_destroy(BcWork *w);
long long betweenness_work_bytes(const BcWork *w);
void betweenness_values_changed(BcWork *w);   // g4s_csr_update_values: whether a stored value is zero has to be found out again

} // namespace g4s

struct g4s_csr_s {
    int32_t rows = 0, cols = 0;
    int64_t nnz = 0;
    const int32_t *d_rowptr = nullptr;
    const int32_t *d_colids = nullptr;
    const double *d_values = nullptr;   // current values (g4s_csr_update_values swaps a borrowed array)
    bool owns = false;
    bool use_nt = true;
    unsigned flags = 0;                 // of g4s_csr_create
    bool rowptr_checked = false;        // stream_check_rowptr_device has passed
    // At most one of pb / dia / bcsr exists: the handle's SpMV path. Without one it is the row-streaming plan, which SpMM runs on whatever the path.
    g4s::StreamPlan stream;             // row-streaming path (spmv.hip)
    g4s::PbPlan *pb = nullptr;          // propagation-blocked path (spmv_pb.hip) for matrices without gather locality
    g4s::DiaPlan *dia = nullptr;        // diagonal form of a stencil or band (spmv_dia.hip)
    g4s::BcsrPlan *bcsr = nullptr;      // block-row form of an assembled FE matrix (spmv_bcsr.hip)
    g4s::SpmmWork *spmm = nullptr;      // g4s_spmm's workspace (spmm.hip), built by g4s_csr_spmm_reserve or a first g4s_spmm
    g4s::TransposeWork *tr = nullptr;   // Aᵀ and its handle (transpose.hip), built by g4s_csr_transpose_reserve or a first transposed product
    g4s::TraverseWork *trv = nullptr;   // g4s_sssp / g4s_bfs workspace (traverse.hip), built by g4s_csr_traverse_reserve or a first traversal
    g4s::PagerankWork *prk = nullptr;   // g4s_pagerank workspace (pagerank.hip), built by g4s_csr_pagerank_reserve or a first g4s_pagerank
    g4s::BcWork *bc = nullptr;          // g4s_betweenness workspace (betweenness.hip), built by g4s_csr_betweenness_reserve or a first g4s_betweenness
};

namespace g4s {

// What TraverseWork, PagerankWork and BcWork hold: one device_malloc per take(), all freed with the owner. The first failure is kept — the CU
// count's, a take's or a noted call's — and every take() behind it does nothing; `bytes` sums what was allocated (g4s_csr_info.plan_bytes).
class DevicePieces {
    static constexpr int kMost = 8;   // TraverseWork takes five; a take() past kMost is a mistake in this library, reported as hipErrorInvalidValue
    void *p_[kMost];
    int n_ = 0;
    hipError_t err_;
public:
    int cus = 1;          // compute units of the device
    int64_t bytes = 0;    // allocated by take()
    DevicePieces() { err_ = device_cus(&cus); }
    DevicePieces(const DevicePieces &) = delete;
    ~DevicePieces() { for (int i = 0; i < n_; ++i) (void)hipFree(p_[i]); }
    template <typename T> void take(T **ptr, size_t n_bytes)
    {
        if (err_ == hipSuccess) err_ = n_ < kMost ? device_malloc(&p_[n_], n_bytes) : hipErrorInvalidValue;
        if (err_ != hipSuccess) return;
        *ptr = static_cast<T *>(p_[n_++]);
        bytes += (int64_t)n_bytes;
    }
    void note(hipError_t e) { if (err_ == hipSuccess) err_ = e; }   // a call that belongs to building the workspace
    bool ok() const { return err_ == hipSuccess; }
    int report(const char *fn) const { return set_error(err_ == hipErrorOutOfMemory ? G4S_ERR_NOMEM : G4S_ERR_HIP, "%s: %s", fn, hipGetErrorString(err_)); }
};

int csr_spmv_path(const g4s_csr_s *A);   // g4s_csr_info.spmv_path: 0 row-streaming, 1 blocked, 3 diagonal, 4 block-row

// The argument rules of a product y(n_out) = A·x or Aᵀ·x on a handle, in g4s_spmv's order; an empty product (n_out == 0) passes whatever x and y are.
int check_spmv_args(const char *fn, const g4s_csr_s *A, int32_t n_out, const double *x, const double *y);

// The one-shot forms: a handle on host or device CSR arrays (create_flags: G4S_DEVICE_POINTERS and the path flags; the streaming path unless
// G4S_SPMV_BLOCKED), one `product(handle, device x, device y)`, synchronous, the handle destroyed. Host pointers: x (nx doubles) is staged on the
// device, y (ny doubles) too when read_y, and y is read back after the product.
int csr_one_shot(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids, const double *values, unsigned create_flags,
                 const double *x, size_t nx, double *y, size_t ny, bool read_y, const std::function<int(g4s_csr_t, const double *, double *)> &product);

} // namespace g4s

// The row-streaming plan of a handle that took the blocked path without one (SpMM runs on it; g4s_csr_update_values falls back to it); NULL stream, synchronous.
int g4s_csr_build_stream_plan(g4s_csr_t A);
