// transpose.hpp — what a CSR handle (spmv.hip) keeps of its transpose: transpose.hip builds, refreshes and frees it.
#pragma once
#include "common.hpp"

namespace g4s {

struct TransposeWork;   // transpose.hip: the arrays of Aᵀ, the entry map perm and the inner handle of Aᵀ

void transpose_work_destroy(TransposeWork *w);
// tvalues[k] = values[perm[k]] on `stream`, then the inner handle's own g4s_csr_update_values (after the forward handle's update)
int transpose_update_values(TransposeWork *w, const double *values, hipStream_t stream);

} // namespace g4s

// spmv.hip: the handle's transpose slot and its create flags (transpose.hip fills the slot on reserve; g4s_csr_destroy frees it)
int g4s_csr_transpose_slot(g4s_csr_t A, g4s::TransposeWork ***slot, unsigned *create_flags);
