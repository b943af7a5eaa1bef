// spmv_bcsr.hpp — interface of the block-row SpMV path (spmv_bcsr.hip) used by the CSR handle (csr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace g4s {
struct BcsrPlan;
// *out stays NULL (status OK) when the matrix is not made of aligned b×b blocks (b = 3, then 2; aligned 4×4 blocks run as 2×2)
int bcsr_try_build(BcsrPlan **out, int rows, int cols, long long nnz, const int32_t *d_rowptr, const int32_t *d_colids, const double *d_values, bool use_nt);
int bcsr_update_values(BcsrPlan *plan, const int32_t *d_colids, const double *d_values, hipStream_t stream);
void bcsr_destroy(BcsrPlan *plan);
long long bcsr_bytes(const BcsrPlan *plan);
int bcsr_block(const BcsrPlan *plan);
// `semiring`: a G4S_SEMIRING_* value; other than plus-times: y := A ⊗ x (beta != 0: y ⊕ (A ⊗ x)), alpha unused
int bcsr_spmv(BcsrPlan *plan, const double *x, double *y, unsigned semiring, double alpha, double beta, hipStream_t stream);
} // namespace g4s
