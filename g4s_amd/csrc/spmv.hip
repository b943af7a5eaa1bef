// spmv.hip — fp64 CSR SpMV for gfx950 (B2 of include/g4s.h):  y = alpha·A·x + beta·y.
//
// The reference has no CSR mat-vec (mv/mv.c:6-27 times dense BLAS-2 on a dense copy of the graph matrix); the
// operation is defined in DESIGN.md §SpMV and restated on the CPU in oracle/g4s_oracle.c:oracle_spmv_csr.
//
// Execution plan (built once per matrix in g4s_csr_create, the role BIN plays for SpGEMM in mm/inc/BIN.h:
// classify rows by work, then give each worker an equal share):
//   * stream blocks — consecutive rows whose nonzeros fit one LDS tile (<= TILE_NNZ products, <= TILE_ROWS rows).
//     A 256-thread workgroup streams colids/values with fully coalesced loads, gathers x, writes the products to
//     LDS, then reduces each row out of LDS. With >128 rows in the block one lane sums one row left to right —
//     the oracle's order, so those rows are bit-identical to it; with fewer rows 2..64 lanes share a row and
//     finish with a wavefront shuffle reduction (segmented by row).
//   * long rows (> TILE_NNZ nonzeros; the hubs of a power-law graph) — split into LONG_CHUNK pieces, one workgroup
//     each, partial sums to a workspace; a second tiny kernel adds a row's partials in chunk order. No atomics, so
//     results are reproducible run to run.
// Stream blocks are dealt to the 8 XCDs in contiguous runs (blockIdx%8 selects the run) so that neighbouring row
// blocks, which touch neighbouring parts of x on banded/stencil matrices, share one L2.
//
// This file is the row-streaming path alone: its plan (spmv_stream.hpp holds the format), the two plan builders and the kernels. The handle that owns a
// plan, and the choice between this path and the blocked, diagonal and block-row ones, are in csr.hip.
#include "common.hpp"
#include "prims.hpp"
#include "spmv_stream.hpp"
#include "spmv_device.hpp"
#include "semiring.hpp"
#include <algorithm>
#include <vector>

namespace {

using g4s::TILE_NNZ;
using g4s::TILE_ROWS;
using g4s::LONG_CHUNK;
using g4s::LongChunk;
using g4s::LongRow;
using g4s::StreamPlan;
using g4s::store_y;

constexpr int WG = 256;
constexpr int UNROLL = TILE_NNZ / WG;     // independent loads in flight per lane
constexpr int kLaneRowMax = 64;           // a longer row inside a many-row block is summed by a wavefront, not by one lane

template <bool NT, typename T>
__device__ __forceinline__ T stream_load(const T *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// Every kernel of this file is a template on a value policy (semiring.hpp): PlusTimes for g4s_spmv, MinPlus / MaxPlus / OrAnd for g4s_spmv_semiring.
// The sums below go through S::identity / S::mul / S::combine, which PlusTimes spells as 0.0, a * b and a + b: its kernels compile to the code they had
// before the policy existed. The semiring kernels read alpha / beta as "beta != 0: combine with the old y" (ACCUMULATE) and ignore alpha.

template <class S>
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = S::combine(v, __shfl_down(v, off, 64));
    return v;
}

template <bool NT, class S>
__global__ __launch_bounds__(WG) void spmv_csr_adaptive_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colids, const double *__restrict__ values,
    const double *__restrict__ x, double *__restrict__ y,
    const int4 *__restrict__ blocks, int n_stream, int stream_per_xcd,
    const LongChunk *__restrict__ chunks, int n_chunks, int chunks_pad, double *__restrict__ partials,
    double alpha, double beta)
{
    __shared__ double prod[TILE_NNZ];
    __shared__ int32_t rp[TILE_ROWS + 1];
    const int tid = threadIdx.x;

    if ((int)blockIdx.x < chunks_pad) {
        // ---- long-row chunk: strided private sums, then workgroup reduction
        if ((int)blockIdx.x >= n_chunks) return;
        const LongChunk c = chunks[blockIdx.x];
        double acc = S::identity();
        int k = c.k0 + tid;
        for (; k + 3 * WG < c.k1; k += 4 * WG) {
            const int c0 = stream_load<NT>(colids + k), c1 = stream_load<NT>(colids + k + WG);
            const int c2 = stream_load<NT>(colids + k + 2 * WG), c3 = stream_load<NT>(colids + k + 3 * WG);
            const double v0 = stream_load<NT>(values + k), v1 = stream_load<NT>(values + k + WG);
            const double v2 = stream_load<NT>(values + k + 2 * WG), v3 = stream_load<NT>(values + k + 3 * WG);
            const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
            acc = S::combine(acc, S::mul(v0, x0)); acc = S::combine(acc, S::mul(v1, x1)); acc = S::combine(acc, S::mul(v2, x2)); acc = S::combine(acc, S::mul(v3, x3));
        }
        for (; k < c.k1; k += WG) acc = S::combine(acc, S::mul(stream_load<NT>(values + k), x[stream_load<NT>(colids + k)]));
        acc = wave_sum<S>(acc);
        if ((tid & 63) == 0) prod[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) partials[c.slot] = S::combine(S::combine(prod[0], prod[1]), S::combine(prod[2], prod[3]));
        return;
    }

    // ---- stream block (XCD-contiguous remap of the block index)
    const int bid = (int)blockIdx.x - chunks_pad;
    // stream_per_xcd > 0: XCD-contiguous runs (block b and b+8 share an XCD); 0: blocks in launch order
    const int lb = stream_per_xcd > 0 ? (bid % g4s::kXcds) * stream_per_xcd + bid / g4s::kXcds : bid;
    if (lb >= n_stream) return;
    const int4 blk = blocks[lb];
    const int r0 = blk.x, nrows = blk.y, k0 = blk.z, nnzb = blk.w;

    for (int r = tid; r <= nrows; r += WG) rp[r] = stream_load<NT>(rowptr + r0 + r);

    if (nnzb > 0) {
        // Branch-free: lanes past the block's last nonzero re-read it (a broadcast, never used) so that all UNROLL
        // index/value loads, then all UNROLL gathers, are in flight together instead of one wait per predicated load.
        const int last = nnzb - 1;
        int cidx[UNROLL];
        double val[UNROLL];
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) {
            const int j = min(i * WG + tid, last);
            cidx[i] = stream_load<NT>(colids + k0 + j);
            val[i] = stream_load<NT>(values + k0 + j);
        }
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) val[i] = S::mul(val[i], x[cidx[i]]);
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) prod[i * WG + tid] = val[i];   // slots >= nnzb are written but never read
    }
    __syncthreads();

    if (nrows * 2 > WG || nnzb <= 16 * nrows) {
        // one lane per row, left-to-right (the oracle's summation order): blocks of many rows, and blocks of short rows however few
        // (a stencil's last block, the forced cuts of the device-side plan builder) — rows of a stencil or band are exact everywhere
        // (Round 5: a row of more than kLaneRowMax entries in such a block — a block of a power-law matrix: hundreds of short rows and one of a thousand
        // entries — is left to a whole wavefront below. As one lane's loop it was a thousand dependent LDS reads: 20 of the 24 µs of a product on a 5e5-entry
        // R-MAT, profiles/r05_small_sizes.txt. Stencil and band rows are far shorter, so their exact order stays.)
        __shared__ int heavy[TILE_NNZ / kLaneRowMax], n_heavy;
        if (tid == 0) n_heavy = 0;
        __syncthreads();
        for (int r = tid; r < nrows; r += WG) {
            const int a = rp[r] - k0, b = rp[r + 1] - k0;
            if (b - a > kLaneRowMax) { const int h = atomicAdd(&n_heavy, 1); if (h < TILE_NNZ / kLaneRowMax) heavy[h] = r; else { double s = S::identity(); for (int j = a; j < b; ++j) s = S::combine(s, prod[j]); store_y<S>(y, r0 + r, s, alpha, beta); } continue; }
            double s = S::identity();
            for (int j = a; j < b; ++j) s = S::combine(s, prod[j]);
            store_y<S>(y, r0 + r, s, alpha, beta);
        }
        __syncthreads();
        const int nh = min(n_heavy, TILE_NNZ / kLaneRowMax);        // (no more such rows fit a block; the guard above is for safety)
        for (int h = tid >> 6; h < nh; h += WG / 64) {              // one wavefront per heavy row: strided partial sums, then a shuffle reduction
            const int r = heavy[h], a = rp[r] - k0, b = rp[r + 1] - k0;
            double s = S::identity();
            for (int j = a + (tid & 63); j < b; j += 64) s = S::combine(s, prod[j]);
            s = wave_sum<S>(s);
            if ((tid & 63) == 0) store_y<S>(y, r0 + r, s, alpha, beta);
        }
    } else {
        // tpr lanes per row (power of two, <= 64, tpr·nrows <= WG), strided partials + shuffle reduction
        int tpr = 64;
        while (tpr * nrows > WG) tpr >>= 1;
        const int g = tid / tpr, sub = tid & (tpr - 1);
        double s = S::identity();                                 // (groups with g >= nrows hold the identity)
        if (g < nrows) {
            const int a = rp[g] - k0, b = rp[g + 1] - k0;
            for (int j = a + sub; j < b; j += tpr) s = S::combine(s, prod[j]);
        }
        for (int off = tpr >> 1; off > 0; off >>= 1) s = S::combine(s, __shfl_down(s, off, 64));
        if (g < nrows && sub == 0) store_y<S>(y, r0 + g, s, alpha, beta);
    }
}

template <class S>
__global__ void spmv_long_fixup_kernel(const LongRow *__restrict__ lrows, int n_long,
                                       const double *__restrict__ partials, double *__restrict__ y,
                                       double alpha, double beta)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_long) return;
    const LongRow lr = lrows[i];
    double s = S::identity();
    for (int j = 0; j < lr.nslots; ++j) s = S::combine(s, partials[lr.slot0 + j]);
    store_y<S>(y, lr.row, s, alpha, beta);
}

// The same plan built on the device, for matrices whose row pointer is already there: reading 80 M row pointers back and walking them
// on the host cost 100 ms of a 140 ms create (431³ stencil). Rows are cut into runs of kPlanRun; one thread walks each run with the
// greedy rule of build_plan (a binary search per block instead of a row-by-row loop), first counting, then — after a scan — writing. The
// forced cut at the end of a run leaves one short block per run (the kernel reduces short-row blocks with one lane per row, see above).
// Long rows are collected through a counter (few: the hubs) and laid out on the host as before.
constexpr int kPlanRun = 4096;
struct PlanLong { int32_t row, k0, k1; };
template <bool WRITE>
__global__ void plan_walk_kernel(int rows, int nruns, const int32_t *__restrict__ rowptr, const int *__restrict__ blk_off, int *__restrict__ blk_count,
                                 int4 *__restrict__ blocks, PlanLong *__restrict__ longs, int long_cap, int *__restrict__ n_long, int *__restrict__ fail)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nruns) return;
    int r = c * kPlanRun, cnt = 0;
    const int end = min(rows, r + kPlanRun);
    int4 *out = WRITE ? blocks + blk_off[c] : nullptr;
    while (r < end) {
        const int k0 = rowptr[r], len = rowptr[r + 1] - k0;
        if (len < 0) { if (!WRITE) atomicExch(fail, r + 1); return; }
        if (len > TILE_NNZ) {
            if (!WRITE) { const int slot = atomicAdd(n_long, 1); if (slot < long_cap) longs[slot] = PlanLong{r, k0, k0 + len}; }
            ++r;
            continue;
        }
        int lo = r + 1, hi = min(end, r + TILE_ROWS);               // the last row boundary e in [lo, hi] with rowptr[e] − k0 <= TILE_NNZ
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] - k0 <= TILE_NNZ && rowptr[mid] >= k0) lo = mid; else hi = mid - 1;
        }
        if (WRITE) out[cnt] = make_int4(r, lo - r, k0, rowptr[lo] - k0);
        ++cnt;
        r = lo;
    }
    if (!WRITE) blk_count[c] = cnt;
}
__global__ void plan_monotone_kernel(int rows, const int32_t *__restrict__ rowptr, int *__restrict__ fail)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows && rowptr[r + 1] < rowptr[r]) atomicExch(fail, r + 1);
}

// A row of more than TILE_NNZ entries [k0, k1): its chunks of LONG_CHUNK entries, one partial-sum slot each, in entry order.
void push_long_row(int32_t row, int64_t k0, int64_t k1, std::vector<LongChunk> &chunks, std::vector<LongRow> &lrows)
{
    LongRow lr{row, (int32_t)chunks.size(), 0, 0};
    for (int64_t k = k0; k < k1; k += LONG_CHUNK) {
        chunks.push_back(LongChunk{row, (int32_t)k, (int32_t)std::min<int64_t>(k + LONG_CHUNK, k1), (int32_t)chunks.size()});
        lr.nslots++;
    }
    lrows.push_back(lr);
}

// The blocks are in place: the launch geometry and the long-row tables.
int finish_plan(StreamPlan *P, int64_t nnz, size_t n_blocks, const std::vector<LongChunk> &chunks, const std::vector<LongRow> &lrows)
{
    P->n_stream = (int)n_blocks;
    // Contiguous runs of blocks per XCD pay off while the matrix stays cache-resident across launches (+12 % on the 80 MB 5-point
    // Laplacian); on matrices far beyond the 256 MiB Infinity Cache plain launch order measured 2 % faster (banded 10M, 7-point 431³).
    P->xcd_runs = 12 * nnz <= (256ll << 20);
    P->stream_per_xcd = (P->n_stream + g4s::kXcds - 1) / g4s::kXcds;
    P->n_chunks = (int)chunks.size();
    P->chunks_pad = (P->n_chunks + g4s::kXcds - 1) / g4s::kXcds * g4s::kXcds;
    P->n_long = (int)lrows.size();
    if (P->n_chunks) {
        G4S_TRY(P->chunks.alloc(sizeof(LongChunk) * chunks.size()));
        G4S_HIP_TRY(hipMemcpy(P->chunks.p, chunks.data(), sizeof(LongChunk) * chunks.size(), hipMemcpyHostToDevice));
        G4S_TRY(P->long_rows.alloc(sizeof(LongRow) * lrows.size()));
        G4S_HIP_TRY(hipMemcpy(P->long_rows.p, lrows.data(), sizeof(LongRow) * lrows.size(), hipMemcpyHostToDevice));
        G4S_TRY(P->partials.alloc(sizeof(double) * chunks.size()));
    }
    P->built = true;
    return G4S_OK;
}

} // namespace

namespace g4s {

// Row classification + equal-share blocking on the host (one pass over rowptr).
int stream_build(StreamPlan *P, int32_t rows, int64_t nnz, const int32_t *rowptr)
{
    if (rows > 0) {
        if (rowptr[0] != 0) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr[0] != 0 (zero-based CSR expected)");
        if ((int64_t)rowptr[rows] != nnz) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr[rows] != nnz");
    }
    std::vector<int4> blocks;
    std::vector<LongChunk> chunks;
    std::vector<LongRow> lrows;
    blocks.reserve((size_t)(nnz / TILE_NNZ + rows / TILE_ROWS + 16));
    int32_t r = 0;
    while (r < rows) {
        int64_t len = (int64_t)rowptr[r + 1] - rowptr[r];
        if (len < 0) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr decreases at row %d", r);
        if (len > TILE_NNZ) {
            push_long_row(r, rowptr[r], rowptr[r + 1], chunks, lrows);
            ++r;
            continue;
        }
        const int32_t rb = r;
        int64_t nz = 0;
        while (r < rows && r - rb < TILE_ROWS) {
            len = (int64_t)rowptr[r + 1] - rowptr[r];
            if (len < 0) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr decreases at row %d", r);
            if (len > TILE_NNZ || nz + len > TILE_NNZ) break;
            nz += len;
            ++r;
        }
        blocks.push_back(make_int4(rb, r - rb, rowptr[rb], (int)nz));
    }
    if (!blocks.empty()) {
        G4S_TRY(P->blocks.alloc(sizeof(int4) * blocks.size()));
        G4S_HIP_TRY(hipMemcpy(P->blocks.p, blocks.data(), sizeof(int4) * blocks.size(), hipMemcpyHostToDevice));
    }
    return finish_plan(P, nnz, blocks.size(), chunks, lrows);
}

// The row pointers of a device-resident matrix: zero-based, ending at nnz, never decreasing. Every plan builder relies on it (binary searches over rowptr).
// (The flag is a piece of the create's arena, not a DevBuf: a hipMalloc / hipFree pair here is a device-wide wait in every create of a large matrix.)
int stream_check_rowptr_device(int32_t rows, int64_t nnz, const int32_t *d_rowptr)
{
    int32_t ends[2] = {0, 0};
    G4S_HIP_TRY(hipMemcpy(&ends[0], d_rowptr, sizeof(int32_t), hipMemcpyDeviceToHost));
    G4S_HIP_TRY(hipMemcpy(&ends[1], d_rowptr + rows, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ends[0] != 0) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr[0] != 0 (zero-based CSR expected)");
    if ((int64_t)ends[1] != nnz) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr[rows] != nnz");
    int *d_fail = nullptr, h_fail = 0;
    if (scratch_alloc((void **)&d_fail, sizeof(int), nullptr) != G4S_OK) return G4S_ERR_NOMEM;
    hipError_t e = hipMemsetAsync(d_fail, 0, sizeof(int), nullptr);
    hipLaunchKernelGGL(plan_monotone_kernel, dim3((rows + 255) / 256), dim3(256), 0, nullptr, rows, d_rowptr, d_fail);
    if (e == hipSuccess) e = hipMemcpy(&h_fail, d_fail, sizeof(int), hipMemcpyDeviceToHost);
    scratch_free(d_fail, nullptr);
    if (e != hipSuccess) return set_error(G4S_ERR_HIP, "g4s_csr_create: rowptr check failed: %s", hipGetErrorString(e));
    if (h_fail) return set_error(G4S_ERR_INVALID, "g4s_csr_create: rowptr decreases at row %d", h_fail - 1);
    return G4S_OK;
}

int stream_build_device(StreamPlan *P, int32_t rows, int64_t nnz, const int32_t *d_rowptr)
{
    const int nruns = (rows + kPlanRun - 1) / kPlanRun;
    const int long_cap = (int)std::min<int64_t>(nnz / TILE_NNZ + 1, rows);
    DevBuf cnt, off, scalars, d_longs;                              // scalars: [0] n_long, [1] fail (row + 1)
    G4S_TRY(cnt.alloc(sizeof(int) * ((size_t)nruns + 1)));
    G4S_TRY(off.alloc(sizeof(int) * ((size_t)nruns + 1)));
    G4S_TRY(scalars.alloc(sizeof(int) * 2));
    G4S_TRY(d_longs.alloc(sizeof(PlanLong) * (size_t)long_cap));
    G4S_HIP_TRY(hipMemset(scalars.p, 0, sizeof(int) * 2));
    G4S_HIP_TRY(hipMemset(cnt.p, 0, sizeof(int) * ((size_t)nruns + 1)));
    int *d_scalars = scalars.as<int>(), h_scalars[2] = {0, 0};
    hipLaunchKernelGGL(plan_walk_kernel<false>, dim3((nruns + 63) / 64), dim3(64), 0, nullptr, rows, nruns, d_rowptr, (const int *)nullptr, cnt.as<int>(), (int4 *)nullptr,
                       d_longs.as<PlanLong>(), long_cap, d_scalars, d_scalars + 1);
    G4S_HIP_TRY(hipGetLastError());                                // the two plan kernels' launches were never checked
    G4S_TRY(prims::exclusive_scan(cnt.as<int>(), off.as<int>(), (long long)nruns + 1, nullptr));
    int n_blocks = 0;
    G4S_HIP_TRY(hipMemcpy(&n_blocks, off.as<int>() + nruns, sizeof(int), hipMemcpyDeviceToHost));
    G4S_HIP_TRY(hipMemcpy(h_scalars, d_scalars, sizeof(int) * 2, hipMemcpyDeviceToHost));
    if (n_blocks) {
        G4S_TRY(P->blocks.alloc(sizeof(int4) * (size_t)n_blocks));
        hipLaunchKernelGGL(plan_walk_kernel<true>, dim3((nruns + 63) / 64), dim3(64), 0, nullptr, rows, nruns, d_rowptr, off.as<int>(), cnt.as<int>(), P->blocks.as<int4>(),
                           d_longs.as<PlanLong>(), long_cap, d_scalars, d_scalars + 1);
        G4S_HIP_TRY(hipGetLastError());
    }
    std::vector<PlanLong> longs((size_t)std::min(h_scalars[0], long_cap));
    if (!longs.empty()) G4S_HIP_TRY(hipMemcpy(longs.data(), d_longs.p, sizeof(PlanLong) * longs.size(), hipMemcpyDeviceToHost));
    G4S_HIP_TRY(hipDeviceSynchronize());
    std::sort(longs.begin(), longs.end(), [](const PlanLong &a, const PlanLong &b) { return a.row < b.row; });
    std::vector<LongChunk> chunks;
    std::vector<LongRow> lrows;
    for (const PlanLong &l : longs) push_long_row(l.row, l.k0, l.k1, chunks, lrows);
    return finish_plan(P, nnz, (size_t)n_blocks, chunks, lrows);
}

int stream_spmv(const StreamPlan &P, const int32_t *d_rowptr, const int32_t *d_colids, const double *d_values, bool use_nt, const double *x, double *y,
                unsigned sr_flag, double alpha, double beta, hipStream_t s)
{
    return semiring::dispatch(sr_flag, [&](auto policy) {
        using S = decltype(policy);
        const int grid = P.chunks_pad + P.stream_per_xcd * kXcds;
        if (grid > 0) {
            if (use_nt)
                hipLaunchKernelGGL((spmv_csr_adaptive_kernel<true, S>), dim3(grid), dim3(WG), 0, s, d_rowptr, d_colids, d_values,
                                   x, y, P.blocks.as<int4>(), P.n_stream, P.xcd_runs ? P.stream_per_xcd : 0, P.chunks.as<LongChunk>(), P.n_chunks,
                                   P.chunks_pad, P.partials.as<double>(), alpha, beta);
            else
                hipLaunchKernelGGL((spmv_csr_adaptive_kernel<false, S>), dim3(grid), dim3(WG), 0, s, d_rowptr, d_colids, d_values,
                                   x, y, P.blocks.as<int4>(), P.n_stream, P.xcd_runs ? P.stream_per_xcd : 0, P.chunks.as<LongChunk>(), P.n_chunks,
                                   P.chunks_pad, P.partials.as<double>(), alpha, beta);
            G4S_HIP_TRY(hipGetLastError());
        }
        if (P.n_long > 0) {
            hipLaunchKernelGGL(spmv_long_fixup_kernel<S>, dim3((P.n_long + 255) / 256), dim3(256), 0, s, P.long_rows.as<LongRow>(), P.n_long,
                               P.partials.as<double>(), y, alpha, beta);
            G4S_HIP_TRY(hipGetLastError());
        }
        return (int)G4S_OK;
    });
}

} // namespace g4s
