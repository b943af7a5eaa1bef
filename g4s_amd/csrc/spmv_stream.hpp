// spmv_stream.hpp — interface of the row-streaming SpMV path (spmv.hip) and the format of its plan, which the SpMM kernels (spmm.hip) run on too.
#pragma once
#include "common.hpp"

namespace g4s {

constexpr int TILE_NNZ = 2048;            // fp64 products staged in LDS per workgroup (16 KiB)
#ifndef G4S_TILE_ROWS
#define G4S_TILE_ROWS 1024
#endif
constexpr int TILE_ROWS = G4S_TILE_ROWS;  // row cap per stream block (4 KiB of staged row pointers)
constexpr int LONG_CHUNK = 2048;          // nonzeros per long-row chunk (8192 until round 5: a chunk is one workgroup's serial loop of eight rounds)

// A stream block is an int4 {row0, nrows, k0, nnz}: consecutive rows of at most TILE_NNZ entries and TILE_ROWS rows.
struct LongChunk { int32_t row, k0, k1, slot; };     // entries [k0, k1) of a row longer than TILE_NNZ; its partial sum goes to partials[slot]
struct LongRow { int32_t row, slot0, nslots, pad; }; // the row's chunks are slots [slot0, slot0 + nslots)

struct StreamPlan {
    bool built = false;             // a large matrix that took the blocked path builds it only if it ever needs it
    DevBuf blocks;                  // n_stream int4
    int n_stream = 0, stream_per_xcd = 0;
    bool xcd_runs = true;
    DevBuf chunks;                  // n_chunks LongChunk
    int n_chunks = 0, chunks_pad = 0;
    DevBuf long_rows;               // n_long LongRow
    int n_long = 0;
    DevBuf partials;                // n_chunks doubles
    long long bytes() const { return (long long)(blocks.bytes + chunks.bytes + long_rows.bytes + partials.bytes); }
};

// The plan from row pointers on the host (checked on the way: zero-based, ending at nnz, never decreasing) ...
int stream_build(StreamPlan *plan, int32_t rows, int64_t nnz, const int32_t *h_rowptr);
// ... and from row pointers on the device that stream_check_rowptr_device has passed. NULL stream, synchronous.
int stream_build_device(StreamPlan *plan, int32_t rows, int64_t nnz, const int32_t *d_rowptr);
int stream_check_rowptr_device(int32_t rows, int64_t nnz, const int32_t *d_rowptr);
// `semiring`: a G4S_SEMIRING_* value; other than plus-times: y := A ⊗ x (beta != 0: y ⊕ (A ⊗ x)), alpha unused
int stream_spmv(const StreamPlan &plan, const int32_t *d_rowptr, const int32_t *d_colids, const double *d_values, bool use_nt, const double *x, double *y,
                unsigned semiring, double alpha, double beta, hipStream_t stream);

} // namespace g4s
