// spmv_dia.hpp — interface of the diagonal-form SpMV path (spmv_dia.hip) used by the CSR handle (csr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace g4s {
struct DiaPlan;
// *out stays NULL (status OK) when the entries do not lie on at most 32 well-filled diagonals, or when there is no room for the diagonal form
int dia_try_build(DiaPlan **out, int rows, int cols, long long nnz, const int32_t *d_rowptr, const int32_t *d_colids, const double *d_values, bool use_nt);
int dia_update_values(DiaPlan *plan, const double *d_values, hipStream_t stream);
void dia_destroy(DiaPlan *plan);
long long dia_bytes(const DiaPlan *plan);
// `semiring`: a G4S_SEMIRING_* value; other than plus-times: y := A ⊗ x (beta != 0: y ⊕ (A ⊗ x)), alpha unused
int dia_spmv(DiaPlan *plan, const double *x, double *y, unsigned semiring, double alpha, double beta, hipStream_t stream);
} // namespace g4s
