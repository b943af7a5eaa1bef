// cg_async.hpp — a conjugate-gradient solve whose first batch of iterations is only ENQUEUED (cg.hip: CgRun, DistCgAsync), for callers that go on
// enqueuing dependent work speculatively and read the solve's state with their own scalars in one host synchronisation (stokes.hip).
#pragma once
#include "common.hpp"

namespace g4s {
struct CgRun;        // one device: the product is the element operator or g4s_spmv
struct DistCgAsync;  // a row-partitioned operator: the product and the all-reduces of the dot products go through the transport

// The velocity solves of one call, on either operator: what they share is given once, each solve is start → read → (the caller synchronises) → settle. The
// object owns what the solves reuse — the work vectors and the boundary-equation mask, built by the first start and held (zero_resid must keep its contents
// for the object's life) — and frees it when it goes.
template <typename Run>
class CgSolve {
public:
    CgSolve(const CgSolve &) = delete;
    CgSolve &operator=(const CgSolve &) = delete;
    ~CgSolve();
    // Enqueues: set-up, the first batch of iterations (one more than this thread's previous solve needed), the loop test, the strip of d0's boundary rows.
    int start(const double *rhs, double *d0);
    int read();   // enqueues the copy of the solve's state into the object (the caller synchronises)
    // After that synchronisation. *speculation_held = the first batch met the loop test, so everything enqueued behind it used the final d0. If it did
    // not, the solve is run to its end here (synchronising) and d0 stripped again; the caller must redo what it had enqueued behind the solve.
    int settle(bool *speculation_held, int32_t *cycles, double *residual);

protected:
    explicit CgSolve(Run *run) : run_(run) {}
    Run *run_;
};

struct LocalCgSolve : CgSolve<CgRun> {      // exactly one of op / A
    LocalCgSolve(g4s_elem_op_t op, g4s_csr_t A, int32_t neq, const double *BI, const int32_t *zero_resid, int32_t n_zero, double acc, int32_t steps, void *stream);
};
struct DistCgSolve : CgSolve<DistCgAsync> { // every rank reads the same all-reduced sums and takes the same turn
    DistCgSolve(g4s_spmv_dist_t A, const g4s_transport *tr, int32_t n_local, const double *BI, const int32_t *zero_resid, int32_t n_zero, double acc, int32_t steps,
                void *stream);
};
} // namespace g4s
