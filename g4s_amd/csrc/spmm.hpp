// spmm.hpp — what the SpMM entry points (spmm.hip) read of a CSR handle (spmv.hip owns the handle and its row-streaming plan).
#pragma once
#include "common.hpp"

namespace g4s {

struct SpmmWork;   // spmm.hip: the handle's SpMM workspace (reserved k_max, the partial sums of long-row chunks for k_max vectors)

struct CsrSpmmView {
    int32_t rows, cols;
    int64_t nnz;
    const int32_t *rowptr, *colids;
    const double *values;                 // the CSR arrays, current values (g4s_csr_update_values swaps a borrowed array)
    int spmv_path;                        // g4s_csr_info.spmv_path
    bool stream_plan;                     // the row-streaming plan below exists (a large blocked-path handle builds it only on demand)
    int tile_nnz, tile_rows, long_chunk;  // the plan's block limits
    const int4 *blocks;                   // row-aligned blocks {row0, nrows, k0, nnz}
    int n_blocks;
    const int4 *chunks;                   // long-row chunks {row, k0, k1, slot}
    int n_chunks;
    const int4 *long_rows;                // {row, slot0, nslots, unused}
    int n_long;
    SpmmWork **work;                      // the handle's workspace slot; spmm_work_destroy frees it with the handle
    int64_t *plan_bytes;                  // g4s_csr_info.plan_bytes: the SpMM workspace is counted in it
};

void spmm_work_destroy(SpmmWork *w);      // spmm.hip

} // namespace g4s

int g4s_csr_spmm_view(g4s_csr_t A, g4s::CsrSpmmView *out);   // spmv.hip
int g4s_csr_build_stream_plan(g4s_csr_t A);                  // spmv.hip: the row-streaming plan on the NULL stream, synchronous (added to plan_bytes)
