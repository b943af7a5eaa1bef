/*
 * g4s.h — C-ABI of libg4s_hip.so: the MI355X (gfx950) drop-in for G4S's graph-as-sparse-matrix hot path.
 *
 * Plain C types only, no exceptions cross this boundary, every entry point returns a g4s_status
 * (0 = success, negative = error; g4s_last_error() gives the message of the calling thread's last failure).
 *
 * Each entry point names the reference interface (file:line under the G4S tree) it replaces:
 *
 *   B1  raw-pointer CSR SpGEMM     mm/inc/mkl_mult.h:40-43      void mkl(arpt,acol,aval, brpt,bcol,bval, &crpt,&ccol,&cval, M,K,N,&cnnz, Timings&)
 *                                   mm/inc/hash_mult.h:1028-1057 HashSpGEMM<vectorProbing,sortOutput>(a,b,c,multop,addop)
 *   B2  CSR SpMV                   mv/mv.c:6-27                 void matrix_multiply_*(double*A,double*B,double*C,int dim)  (y = A·x; the
 *                                                                reference ships only dense BLAS-2 forms, the CSR form is defined in DESIGN.md)
 *   B3  graph gather/apply         citcoms/lib/global_defs.h:48-49,854-857  spmm_dense(numNodes,degree,edgeWeight,vertexStates,temp,result,gather,apply,time,threadNum)
 *                                   deepmd/source/op/graph.h:5-32            struct Graph, GraphProcess(graph,result,gather,apply)
 *                                   cantera/src/thermo/RedlichKwongMFTP.cpp:917-983  GraphProcess1/2
 *
 * Index type is int32 and value type fp64, as in the reference (mm/inc/define.h:14-15).
 * The library fails loudly (G4S_ERR_HIP) when no HIP device is usable; there is no CPU fallback in it.
 */
#ifndef G4S_H
#define G4S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
typedef int g4s_status;
#define G4S_OK               0
#define G4S_ERR_INVALID     -1 /* bad argument (null pointer, negative size, unsorted rowptr …)           */
#define G4S_ERR_NOMEM       -2 /* host or device allocation failed                                        */
#define G4S_ERR_HIP         -3 /* a HIP runtime call failed / no device                                   */
#define G4S_ERR_OVERFLOW    -4 /* a result does not fit the reference's int32 index type (define.h:14)    */
#define G4S_ERR_UNSUPPORTED -5 /* e.g. an unregistered gather/apply pair handed to the device dispatcher  */

/* ------------------------------------------------------------------ flags */
#define G4S_HOST_POINTERS    0u /* array arguments are host memory (default; H2D/D2H happen inside)       */
#define G4S_DEVICE_POINTERS  1u /* array arguments are device memory, borrowed for the handle's lifetime  */
#define G4S_SORT_OUTPUT      2u /* SpGEMM: rows of C sorted by column (HashSpGEMM sortOutput, hash_mult.h:526-553) */
#define G4S_SPMV_NO_NT       4u /* SpMV: plain (cache-allocating) loads for the matrix stream instead of nontemporal */
#define G4S_SPMV_BLOCKED     8u /* SpMV: force the propagation-blocked path (x band / y band in LDS; for matrices without gather locality) */
#define G4S_SPMV_STREAM     16u /* SpMV: force the row-streaming CSR kernel (default: chosen per matrix — blocked for matrices without gather locality,
                                 * the index-free diagonal form for stencil / banded matrices, the CSR kernel otherwise) */

#define G4S_SPMV_UPDATABLE 128u /* SpMV: the values of this matrix will be replaced (g4s_csr_update_values): a plan that keeps them in another order also keeps the
                                 * map back to the CSR order (blocked path: 4 bytes per entry), so that an update is one pass instead of a new plan */

/* ------------------------------------------------------------------ runtime */
const char *g4s_version(void);
/* "spmv_kernel_sources_sha256=<hex>;variant=<name>": the SpMV kernel sources this library was built from (tools/kernel_hash.py) and the name of an A/B
 * variant build (empty for the regular one) — for tools that pair a stored measurement with the LOADED build (bench.py's roofline.traffic). */
const char *g4s_build_info(void);
/* Loads the device code of the plan builders, the SpMV kernels and the SpGEMM row classes now instead of inside the first g4s_csr_create / g4s_spmv /
 * g4s_spgemm_* of the process (HIP loads a translation
 * unit's code object at its first launch: 12–25 ms of a first create of configs[1] that takes 18.6 ms afterwards). Builds, runs and destroys one small matrix on
 * the path g4s_csr_create picks for it, on the blocked and on the streaming path, and squares it. Optional; synchronous; may be called again (≈ 25 ms then, 0.2 s in a
 * process that has not touched the device yet).
 * No reference counterpart (a CPU library has no such step). */
g4s_status g4s_warm_up(void);
const char *g4s_last_error(void);                 /* thread-local, never NULL                              */
g4s_status  g4s_device_count(int *count);
g4s_status  g4s_set_device(int device);           /* also honours HIP_VISIBLE_DEVICES                      */
g4s_status  g4s_device_synchronize(void);
g4s_status  g4s_shutdown(void);                   /* releases cached workspaces                            */
g4s_status  g4s_trim(void);                       /* returns the library's cached device blocks (freed SpGEMM outputs, column scratch) to the
                                                    * driver; for host frameworks whose own allocator is about to need the memory            */

/* Allocator that matches every callee-allocated output of this library (the reference pairs
 * my_malloc/my_free, mm/inc/utility.h:126-153; CSR::make_empty frees what mkl()/HashSpGEMM allocated,
 * mm/inc/CSR.h:50-62). */
void       *g4s_malloc(size_t bytes);
void        g4s_free(void *p);

/* Device buffers for callers without their own HIP code (the bench and the tests use torch tensors instead). */
/* Device blocks of the library's caching allocator (a freed block is kept and handed out again for a request it fits within 25 %:
 * fresh multi-GB allocations cost up to seconds on this stack; g4s_shutdown releases what is cached). g4s_dev_free synchronises the
 * device like hipFree, and also accepts a plain hipMalloc pointer. */
g4s_status  g4s_dev_alloc(void **dptr, size_t bytes);
g4s_status  g4s_dev_free(void *dptr);
g4s_status  g4s_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
g4s_status  g4s_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);

/* ------------------------------------------------------------------ B2: CSR SpMV  y = alpha·A·x + beta·y */

/* Opaque device-resident CSR matrix + its SpMV execution plan (row blocks, long-row chunks). */
typedef struct g4s_csr_s *g4s_csr_t;

typedef struct g4s_csr_info {
    int32_t rows, cols;
    int64_t nnz;
    int32_t stream_blocks;    /* row-aligned blocks of <= tile_nnz nonzeros handled by the LDS-staged path */
    int32_t long_rows;        /* rows longer than tile_nnz, split into chunks                             */
    int32_t long_chunks;
    int32_t tile_nnz, tile_rows, long_chunk_nnz;
    int64_t algorithmic_bytes;/* 12·nnz + 4·(rows+1) + 8·rows + 8·cols                      */
    int64_t plan_bytes;       /* extra device bytes the plan itself occupies                               */
    int32_t spmv_path;        /* 0 = row-streaming CSR kernel, 1 = propagation-blocked (regrouped copy of the matrix), 2 = unused (was round 2's tile-blocked experiment, removed),
                               * 3 = diagonal-structured, index-free (stencil / banded matrices: values by diagonal + a presence mask per row),
                               * 4 = block-row (assembled FE matrices: aligned b×b blocks, one block-column id per block, one lane per row) */
    int32_t reserved;
} g4s_csr_info;

/* Create a handle. rowptr has rows+1 entries, zero-based, non-decreasing, rowptr[rows] == nnz; colids in [0,cols).
 * With G4S_HOST_POINTERS the three arrays are copied to the device (the handle owns the copies);
 * with G4S_DEVICE_POINTERS they are borrowed and must outlive the handle. Replaces the container role of
 * CSR<int,double> (mm/inc/CSR.h:22-113) for device residency.
 * The handle is a SNAPSHOT of the matrix: the execution plan (and, on three of the four paths, a copy of the values in the plan's own order) is
 * built here; the PATTERN is fixed for the handle's life, new VALUES go in through g4s_csr_update_values.
 * Concurrency: a handle supports ONE product in flight at a time — g4s_spmv uses per-handle workspaces (the partial sums of split long
 * rows on the streaming path, the product buffer and the gathered hot columns on the blocked path), so two g4s_spmv calls on the same
 * handle must be ordered (same stream, or an event between them); different handles are independent.
 * Threads and streams (what tests/test_concurrency_gpu.py pins — for g4s_csr_extract_* tests/test_extract_threads_gpu.py, for g4s_kcore tests/test_kcore_threads_gpu.py, for g4s_color tests/test_color_threads_gpu.py, for g4s_ktruss tests/test_ktruss_threads_gpu.py, for g4s_strongly_connected_components tests/test_scc_threads_gpu.py, for g4s_minimum_spanning_forest tests/test_msf_threads_gpu.py —, every result compared bit for bit):
 *   Different host threads may call at the same time: the one-call and the two-call SpGEMM, g4s_spgemm_masked, g4s_triangle_count,
 *     g4s_minimum_spanning_forest, g4s_connected_components, g4s_strongly_connected_components, g4s_kcore, g4s_color, g4s_ktruss, g4s_csr_transpose, the four g4s_csr_ewise_* / g4s_csr_select_* calls, g4s_csr_from_coo_symbolic / _numeric, g4s_csr_row_indices, g4s_csr_extract_symbolic / _numeric, the one-shot g4s_spmv_csr_i32_f64, g4s_csr_create / g4s_csr_destroy of their own handles,
 *     g4s_sssp / g4s_bfs and the products on a handle the thread owns, g4s_free / g4s_dev_free of their outputs and g4s_trim. Each thread
 *     passes a stream of its own (or the NULL stream); inputs that are only read may be shared. The library's scratch is per thread and per call; the
 *     freed blocks it caches per process are handed to another thread only after the stream that used them has been synchronised.
 *   Different streams from one thread: g4s_spmv, g4s_spmm, g4s_spmv_semiring and g4s_spmv_transpose (after the reserves) on DIFFERENT handles may be
 *     enqueued on different streams with nothing between them; each result is that of the call made alone. One handle stays one product at a time.
 *   g4s_last_error() belongs to the calling thread: a refusal in one thread never shows in another, and leaves nothing behind in its own — the
 *     next valid call there is exact.
 *   The state g4s_spgemm_symbolic keeps for g4s_spgemm_numeric is ONE per process, whichever thread made it. Any thread's next g4s_spgemm_symbolic
 *     or one-call product, g4s_trim and g4s_shutdown drop it; a numeric call that is using it at that moment finishes with it, the next one works
 *     everything out again — the result is the same either way. The column scratch is one per process too: a product that starts while another
 *     call or the kept state holds it runs without (G4S_SPGEMM_NO_COLSCRATCH=1 takes that path on purpose), with the same result.
 *   g4s_shutdown must not run beside other calls: it destroys the scratch pools they allocate from.
 * Stream order of create: g4s_csr_create reads the arrays and builds the plan on the NULL (legacy default) stream and returns after it
 * has synchronised; with G4S_DEVICE_POINTERS the arrays must be complete with respect to that stream — a caller that filled them on a
 * non-blocking stream synchronises it first. */
g4s_status g4s_csr_create(g4s_csr_t *out, int32_t rows, int32_t cols, int64_t nnz,
                          const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags);
/* New values for the same pattern — what a time-stepping caller does to its operator (CitcomS rebuilds the stiffness matrix before every Stokes solve and
 * inside the viscosity iteration: citcoms/lib/Drive_solvers.c:88,134 → construct_stiffness_B_matrix, Construct_arrays.c:740). values: nnz entries in the
 * order of the arrays the handle was created from (flags: G4S_HOST_POINTERS or G4S_DEVICE_POINTERS), or NULL when a BORROWED device array has been rewritten
 * in place. A handle that owns its arrays copies them in; a handle that borrows device arrays borrows the new array from here on (device pointer required).
 * The plan's own copy is refreshed on `stream` (asynchronous like g4s_spmv, ordered with the products on that stream): one gather pass on the blocked path
 * (created with G4S_SPMV_UPDATABLE; without the flag the regrouping is repeated — the cost of a create), a refill of the diagonals / the block-major copy,
 * nothing on the row-streaming path. Results afterwards are those of a handle freshly created from the new values, bit for bit. A matrix built from
 * an edge list gets such values from a repeat of g4s_csr_from_coo_numeric with the new val on the perm and crpt it was built with. */
g4s_status g4s_csr_update_values(g4s_csr_t A, const double *values, unsigned flags, void *stream);
g4s_status g4s_csr_destroy(g4s_csr_t A);
g4s_status g4s_csr_get_info(g4s_csr_t A, g4s_csr_info *info);
/* Device pointers of the handle's arrays (borrowed). */
g4s_status g4s_csr_device_arrays(g4s_csr_t A, const int32_t **rowptr, const int32_t **colids, const double **values);

/* Asynchronous SpMV on `stream` (a hipStream_t; NULL = the default stream). x_dev (cols doubles) and
 * y_dev (rows doubles) are device pointers and must not alias. beta == 0 never reads y (BLAS convention).
 * The call only enqueues kernels on `stream` — no allocation, no synchronisation, no host read — so a sequence of products may be recorded
 * in a hipGraph (stream capture) and replayed (tests/test_graph_capture_gpu.py, all three paths). */
g4s_status g4s_spmv(g4s_csr_t A, const double *x_dev, double *y_dev, double alpha, double beta, void *stream);

/* One-shot form with the call shape of mv/mv.c:6-27 (caller-owned in/out arrays, synchronous).
 * flags: G4S_HOST_POINTERS or G4S_DEVICE_POINTERS applies to all five arrays. */
g4s_status g4s_spmv_csr_i32_f64(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids,
                                const double *values, const double *x, double *y,
                                double alpha, double beta, unsigned flags);

/* ------------------------------------------------------------------ B2 with k vectors: CSR SpMM  Y = alpha·A·X + beta·Y */
/* The sparse form of the reference's dense comparison driver (mm/src/cblas_dxxmm.c: a .mtx matrix times a dense dim × dim column-major B
 * with cblas_dgemm), and what several right-hand sides, block Krylov solvers or multi-source walks do instead of k g4s_spmv calls: the
 * matrix is read once per call (per tile of 32 vectors), not once per vector. X is cols × k, Y is rows × k.
 *   When it pays: one SpMM beats k g4s_spmv calls only where the SpMV path of the handle is not much faster per vector than a CSR walk — it
 *     is a CSR kernel on every handle. On the blocked path (power-law graphs) the k-call loop is faster at every k measured, and at small k the
 *     loop can be faster on the other paths too; DESIGN.md §4.1 (e) has the measured ratios per path and k.
 *   Layout: row-major by default, element (i, j) at [i·ld + j], needs ldx >= k and ldy >= k; with G4S_SPMM_COL_MAJOR element (i, j) is at
 *     [i + j·ld] and ldx >= cols, ldy >= rows are needed.
 *   Padding is never touched: entries of Y outside the rows × k block are neither read nor written.
 *   Any alignment: any 8-byte-aligned base pointer and any ld (odd ld, offset sub-views); 16-byte aligned X and Y with even ld are the fast case.
 *   beta == 0 never reads Y (BLAS convention: NaN in Y does not leak). k == 0 and rows == 0 are no-ops; nnz == 0 gives Y = beta·Y.
 *   X and Y must not overlap: overlapping address ranges return G4S_ERR_INVALID. Argument checks run before any HIP call.
 *   Summation is deterministic on every handle (no atomics): each (row, column) of a row of at most tile_nnz entries is summed in stored order,
 *     bit-identical to a column-by-column oracle SpMV; longer rows are split into chunks whose partial sums are added in a fixed order.
 *   One product in flight per handle: g4s_spmm and g4s_spmv share the concurrency rule of g4s_csr_create.
 *   New values (g4s_csr_update_values) are used by the next g4s_spmm, owned and borrowed handles alike.
 *   k == 1 with unit-stride X and Y (column-major, or ld = 1) is g4s_spmv on the streaming, diagonal and block-row paths; on the blocked path it
 *     stays on the SpMM kernels, which are reproducible where the blocked SpMV is not. Such a call sums as g4s_spmv does: on the streaming path
 *     only the rows that one lane sums are bit-identical to the oracle; any other ld keeps the rule above. */
#define G4S_SPMM_COL_MAJOR 256u /* X and Y column-major: element (i, j) at [i + j·ld]; default row-major: [i·ld + j] */

/* Asynchronous on `stream` like g4s_spmv; X_dev and Y_dev are device pointers. Workspace: the SpMM kernels run on the handle's row-streaming
 * plan (which a large blocked-path handle builds on demand) and need n_long_chunks × k_max doubles of their own. Once g4s_csr_spmm_reserve(A, k_max)
 * has run, a call with k <= k_max only enqueues kernels — no allocation, no synchronisation, no host read — and may be recorded in a hipGraph.
 * A call with k above the reserved k_max (every handle starts at 0) first reserves k: on the NULL stream, synchronously, as a create does; if `stream`
 * is capturing at that moment (hipStreamIsCapturing) the call returns G4S_ERR_INVALID and enqueues nothing — reserve before the capture. */
g4s_status g4s_spmm(g4s_csr_t A, int32_t k, const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy,
                    double alpha, double beta, unsigned flags, void *stream);
/* Builds now what g4s_spmm needs for up to k_max vectors (synchronous, NULL stream), so that later calls with k <= k_max — and stream capture — never allocate. */
g4s_status g4s_csr_spmm_reserve(g4s_csr_t A, int32_t k_max);
/* One-shot form, like g4s_spmv_csr_i32_f64 (synchronous): G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays, | G4S_SPMM_COL_MAJOR.
 * With host pointers only the rows × k block of Y is read (beta != 0) and written back. */
g4s_status g4s_spmm_csr_i32_f64(int32_t rows, int32_t cols, int32_t k, const int32_t *rowptr, const int32_t *colids,
                                const double *values, const double *X, int64_t ldx, double *Y, int64_t ldy,
                                double alpha, double beta, unsigned flags);

/* ---- B2 on several GPUs: the 1-D row-partitioned product (SURVEY.md §8b "g4s_spmv_dist_*", §8e). One process per GPU. Rank r owns rows
 * [row_offsets[r], row_offsets[r+1]) of a square operator and the same slab of x and y; the local rows are given as CSR with GLOBAL column
 * ids. The reference has no multi-device code on this path; the pattern replaced is CitcomS's per-mat-vec neighbour exchange
 * (citcoms/lib/Regional_parallel_related.c:744-789) with the equal-work row split of mm/inc/BIN.h:101-122. Per product only the x entries
 * a rank's rows actually reference travel (halo planes for stencils), each peer pair over its own xGMI link (ncclSend/ncclRecv in one
 * group), while the own-column part of the product runs. */
#define G4S_DIST_LOOPBACK 32u   /* single-rank rehearsal: half of the own slab is treated as remote and travels rank 0 → rank 0 through RCCL, cut into
                                 * G4S_DIST_LOOPBACK_PEERS (default 7) segments with their own ncclSend / ncclRecv pair each — the message pattern
                                 * one rank of an 8-GPU node has, on one GPU */
#define G4S_DIST_ALLGATHER 64u  /* exchange = ONE in-place ncclAllGather of the whole vector (every slab padded to the longest; north_star's
                                 * "RCCL all-gather of the dense vector") instead of packed point-to-point messages: more bytes, no index
                                 * lists, nothing to wire. Also selected by G4S_DIST_EXCHANGE=allgather in the environment. */

/* Equal-work contiguous row partition — BIN::set_rows_offset, mm/inc/BIN.h:101-122: prefix-sum the per-row work, average share
 * avg = ceil(total / parts), boundary t = lower_bound(prefix, avg·t), last boundary = rows. The reference splits rows over threads (work =
 * flop per row); the same rule gives g4s_spmv_dist_create its row_offsets. work_i = row_work[i] when row_work is given (host array, rows
 * entries — any cost model the caller has), else (rowptr[i+1] − rowptr[i]) + row_weight (bench.py: row_weight = 1). row_offsets: parts+1
 * entries, host memory. flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for rowptr. Host-side set-up logic: runs without a GPU. */
g4s_status g4s_row_partition(int32_t rows, const int32_t *rowptr, const int64_t *row_work, int64_t row_weight, int32_t parts,
                             int64_t *row_offsets, unsigned flags);

/* One rank's rows cut into the own-column part (columns renumbered to the own slab) and the remote-column part (columns renumbered into
 * the remote x: packed mode — the referenced columns only, ascending, segment [recv_cut[k], recv_cut[k+1]) from owner k, `want` = their
 * indices local to the owner's slab; all-gather mode — k·pad + (c − row_offsets[k])). What g4s_spmv_dist_create does before it uploads;
 * exported for hosts that bring their own transport or device set-up. Host arrays in, g4s_malloc'ed host arrays out (g4s_dist_split_free);
 * needs no GPU. flags: G4S_DIST_ALLGATHER, G4S_DIST_LOOPBACK. merged = 1: fewer than a quarter of the entries sit in own columns and ALL
 * columns went to the remote part (one product per step). */
typedef struct g4s_dist_split {
    int32_t local_rows, n_ref, merged, allgather;
    int64_t nnz_own, nnz_rem, pad;
    int32_t *own_rowptr, *own_colids; double *own_values;
    int32_t *rem_rowptr, *rem_colids; double *rem_values;
    int32_t *want;            /* packed mode: n_ref entries */
    int64_t *recv_cut;        /* segments + 1 entries (segments = world; in loopback mode the rehearsed peer count) */
} g4s_dist_split;
g4s_status g4s_dist_split_rows(int32_t rank, int32_t world, const int64_t *row_offsets, int64_t n_cols,
                               const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags, g4s_dist_split *out);
void g4s_dist_split_free(g4s_dist_split *s);

typedef struct g4s_spmv_dist_s *g4s_spmv_dist_t;
typedef struct g4s_spmv_dist_info {
    int32_t rank, world, local_rows, n_ref;     /* n_ref: distinct remote columns this rank's rows reference (length of the compact remote x) */
    int64_t nnz_own, nnz_rem;                   /* nonzeros in own / remote columns */
    int64_t send_bytes, recv_bytes;             /* per product */
    int32_t own_path, rem_path;                 /* g4s_csr_info.spmv_path of the two parts */
    int32_t connected, reserved;                /* connected: every peer's give list is known; reserved: bit 0 = merged form (own columns are few and live in
                                                 * the remote x with the remote ones: one product per step instead of two), bit 1 = all-gather exchange,
                                                 * bit 2 = poisoned by a failed set-up exchange (see g4s_spmv_dist_apply) */
} g4s_spmv_dist_info;
/* flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for the three matrix arrays, the G4S_SPMV_* path flags, G4S_DIST_LOOPBACK, G4S_DIST_ALLGATHER.
 * row_offsets: world+1 entries, host memory; row_offsets[world] == n_cols. Collective only in the sense that every rank creates its own. */
g4s_status g4s_spmv_dist_create(g4s_spmv_dist_t *out, int32_t rank, int32_t world, const int64_t *row_offsets, int64_t n_cols,
                                const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags);
/* Rectangular operator: rows partitioned by row_offsets (y), columns by col_offsets (x) — the discrete divergence / gradient of the Stokes
 * iteration (elements × equations and back, citcoms/lib/Element_calculations.c:701-779) next to the square stiffness operator. */
g4s_status g4s_spmv_dist_create_rect(g4s_spmv_dist_t *out, int32_t rank, int32_t world, const int64_t *row_offsets, const int64_t *col_offsets,
                                     const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags);
g4s_status g4s_spmv_dist_destroy(g4s_spmv_dist_t h);
g4s_status g4s_spmv_dist_get_info(g4s_spmv_dist_t h, g4s_spmv_dist_info *info);
/* Wiring, RCCL: comm is an ncclComm_t over the same ranks (the caller's own, or g4s_comm_create below); the want / give index lists
 * are exchanged once with ncclSend / ncclRecv. Collective over the communicator. */
g4s_status g4s_spmv_dist_connect_rccl(g4s_spmv_dist_t h, void *comm);
/* Wiring, any other transport (MPI, gloo): idx_dev[0..count) are the entries this rank wants from `peer` (indices local to the peer's
 * slab, device memory); the caller carries every list to its owner and hands it over with _set_give (flags: host or device pointer). */
g4s_status g4s_spmv_dist_want(g4s_spmv_dist_t h, int32_t peer, int64_t *count, const int32_t **idx_dev);
g4s_status g4s_spmv_dist_set_give(g4s_spmv_dist_t h, int32_t peer, int64_t count, const int32_t *idx, unsigned flags);
/* y_local = (A·x)[own rows]. x_local_dev / y_local_dev: this rank's slabs, device memory (y may be NULL on a rank that owns no rows, x on a
 * rank that owns no x entries — a rectangular operator; such a rank still posts its part of the exchange). Asynchronous on `stream`; RCCL
 * traffic runs on a stream of the handle. Needs g4s_spmv_dist_connect_rccl when world > 1.
 * Failure of the set-up exchange: g4s_spmv_dist_connect_rccl waits with a deadline (G4S_DIST_TIMEOUT_S, default 120 s) and watches RCCL's
 * asynchronous error state. When either fires — a peer never entered the exchange — the communicator is ABORTED (ncclCommAbort) and the handle
 * is poisoned: later calls on it fail, g4s_spmv_dist_destroy drops only its host side (the device memory of the stuck operation is left to the
 * process's exit, nothing is synchronised). The caller reports the error and exits non-zero; a supervisor starts a fresh process. */
g4s_status g4s_spmv_dist_apply(g4s_spmv_dist_t h, const double *x_local_dev, double *y_local_dev, void *stream);
/* The same in two halves for callers with their own transport: _begin packs the send buffer and starts y = A_own·x_local; the caller moves
 * send_dev[send_cut[k]..send_cut[k+1]) to peer k and receives peer k's entries into recv_dev[recv_cut[k]..recv_cut[k+1]) (both ordered after
 * _begin on `stream`); _finish adds the remote-column part. */
g4s_status g4s_spmv_dist_begin(g4s_spmv_dist_t h, const double *x_local_dev, double *y_local_dev, void *stream);
/* All-gather mode: send_dev = this rank's slot (pad entries) and goes to EVERY peer (send_cut = {0, …, 0, pad}); recv_dev = the gathered vector,
 * slot k = [k·pad, (k+1)·pad) comes from rank k. */
g4s_status g4s_spmv_dist_buffers(g4s_spmv_dist_t h, double **send_dev, const int64_t **send_cut, double **recv_dev, const int64_t **recv_cut);
g4s_status g4s_spmv_dist_finish(g4s_spmv_dist_t h, double *y_local_dev, void *stream);
/* Column-partition variant — a CORRECTNESS variant (north_star's "all-reduce of partial products"): rank g holds the columns
 * [col_offsets[g], col_offsets[g+1]) of A (all n_rows rows, global column ids inside the slab) and that slab of x; _begin forms the partial y of ALL rows
 * (y_local_dev: n_rows entries), _finish / _apply sum it over the ranks with ncclAllReduce on the communicator of g4s_spmv_dist_connect_rccl — every rank ends
 * with the whole y. With another transport the caller all-reduces y itself between _begin and _finish (_buffers has nothing to hand out). Twice the traffic of
 * the all-gather exchange and every rank reduces all of y: the row partition is the product's form. get_info.reserved bit 3. */
g4s_status g4s_spmv_dist_create_columns(g4s_spmv_dist_t *out, int32_t rank, int32_t world, const int64_t *col_offsets, int32_t n_rows,
                                        const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags);
/* New values for this rank's rows, same pattern (see g4s_csr_update_values): values_local_dev in the order of the arrays given to _create, device memory;
 * the handle must have been created with G4S_SPMV_UPDATABLE. Asynchronous on `stream`; no communication. */
g4s_status g4s_spmv_dist_update_values(g4s_spmv_dist_t h, const double *values_local_dev, unsigned flags, void *stream);
/* RCCL communicator for hosts that have none (rank 0 makes the 128-byte id, every rank gets it by its own means and calls _create), and
 * the sum all-reduce the dot products of a Krylov solver need (citcoms/lib/Global_operations.c:534-562). RCCL is dlopen'ed at first use. */
g4s_status g4s_comm_unique_id(void *id128);
g4s_status g4s_comm_create(void **comm, int32_t world, int32_t rank, const void *id128);
g4s_status g4s_comm_destroy(void *comm);
g4s_status g4s_comm_allreduce_sum_f64(void *comm, double *buf_dev, int64_t count, void *stream);

/* ------------------------------------------------------------------ B1: CSR SpGEMM  C = A·B */

/* Stage timer with the reference's seven fields, milliseconds (mm/inc/Timings.h:4-23). */
typedef struct g4s_timings {
    double create, spmm, convert, order, export_csr, destroy, total;
} g4s_timings;

/* flop = Σ_i Σ_{j∈A(i,:)} nnz(B(acol_j,:))  (mm/inc/mkl_mult.h:8-38, hash_mult.h:46-62); device pointers
 * when flags has G4S_DEVICE_POINTERS. row_flop (may be NULL) receives the per-row count as int64. */
g4s_status g4s_spgemm_flop(int32_t M, const int32_t *arpt, const int32_t *acol, const int32_t *brpt,
                           int64_t *flop, int64_t *row_flop, unsigned flags);

/* Input contract of the three SpGEMM entry points: zero-based CSR; the rows of A and of B may be in any order, as for HashSpGEMM (its hash traversal never
 * looks at the order, mm/inc/hash_mult.h:579-600, and HashSpGEMM<..., false> emits unsorted rows itself, :530-551) and mkl_sparse_spmm (mm/inc/mkl_mult.h:58);
 * repeated columns inside a row are allowed and are added up. The kernels cut B's rows at column boundaries, so a B whose rows are NOT sorted by column (checked
 * on the opening pass of every call) is sorted into a private copy first — the caller's arrays are never modified; sorted input (what CSR::construct produces,
 * mm/inc/CSR.h:640-651) is the fast path. Column ids are range-checked (G4S_ERR_INVALID).
 * Raw-pointer SpGEMM with the call shape of mkl(...) (mm/inc/mkl_mult.h:40-43): inputs borrowed,
 * outputs allocated by the callee — with g4s_malloc for host pointers (free with g4s_free), with
 * g4s_dev_alloc for G4S_DEVICE_POINTERS (free with g4s_dev_free). A is M×K, B is K×N, C is M×N.
 * cnnz is int64; G4S_ERR_OVERFLOW is returned (and nothing allocated) if it exceeds INT32_MAX,
 * because crpt keeps the reference's int32 type. timings may be NULL.
 *
 * Semirings (HashSpGEMM's MultiplyOperation / AddOperation pair, mm/inc/hash_mult.h:583-593, as a closed set on the device): one of the values below,
 * or-ed into the flags of g4s_spgemm_csr_i32_f64 and g4s_spgemm_numeric (host or device pointers, with or without G4S_SORT_OUTPUT). g4s_spgemm_symbolic
 * takes no flags: the pattern does not depend on the semiring. g4s_spmv_semiring and g4s_spmv_semiring_csr_i32_f64 (below) read them too; no other
 * entry point does.
 *   Pattern: crpt and ccol are bit-identical to the plus-times product of the same inputs (structural entries, repeated columns inside a row, unsorted B
 *     and empty rows included) — an entry exists wherever a product exists, whatever its value.
 *   Values, per output entry, over the products a·b that make it up:
 *     PLUS_TIMES  Σ a·b (identity 0.0) — today's behaviour, within 1e-10 relative of the reference's order of summation;
 *     MIN_PLUS    min(a + b) (identity +inf) — distance products: shortest paths by repeated squaring, k-hop distances;
 *     MAX_PLUS    max(a + b) (identity −inf) — longest / critical paths in a DAG;
 *     OR_AND      1.0 if any product has a != 0 && b != 0, else 0.0 (what std::logical_and / std::logical_or store; NaN counts as nonzero). An entry whose
 *                 products are all false stays in C with the value 0.0 — reachability, transitive closure.
 *   min, max and or do not depend on the order in which products arrive, and each min/max-plus product is one IEEE add: the values of the three are exact and
 *   deterministic on every path. Outside the contract: the sign of a zero result of min/max-plus, and the value of an entry that has a NaN product or a
 *   (+inf) + (−inf) product (the other entries are unaffected).
 *   Two-call form: the state carried from g4s_spgemm_symbolic is structural only, so successive numeric calls on the same arrays may each use another semiring. */
#define G4S_SEMIRING_PLUS_TIMES    0u /* default: C = Σ a·b */
#define G4S_SEMIRING_MIN_PLUS    512u /* C = min(a + b) */
#define G4S_SEMIRING_MAX_PLUS   1024u /* C = max(a + b) */
#define G4S_SEMIRING_OR_AND     1536u /* C = OR(a != 0 && b != 0) as 1.0 / 0.0 */
#define G4S_SEMIRING_MASK       1536u

/* Semiring SpMV: y := A ⊗ x, or y := y ⊕ (A ⊗ x) with G4S_SPMV_ACCUMULATE, over one of the semirings above — the mat-vec that graph algorithms iterate
 * (Bellman-Ford relaxes d := d ⊕ (Aᵀ ⊗ d) over min-plus, BFS expands a frontier over or-and, longest paths in a DAG use max-plus).
 *   flags: one G4S_SEMIRING_* value, optionally | G4S_SPMV_ACCUMULATE. The one-shot form also takes G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and
 *     G4S_SPMV_BLOCKED / G4S_SPMV_STREAM, with the meaning they have in g4s_spmv_csr_i32_f64. Any other bit returns G4S_ERR_INVALID before any HIP call,
 *     and so do a NULL handle, a NULL x or y and an x that aliases y (the checks of g4s_spmv).
 *   Values, per row i, over the stored entries a_ij of the row (repeated columns included):
 *     MIN_PLUS    min(a_ij + x_j) (identity +inf);
 *     MAX_PLUS    max(a_ij + x_j) (identity −inf);
 *     OR_AND      1.0 if any a_ij != 0 && x_j != 0, else 0.0 (NaN counts as nonzero, as in SpGEMM).
 *     An empty row gets the identity. With G4S_SPMV_ACCUMULATE the row's result is combined with y by ⊕ (an empty row leaves y unchanged); for OR_AND the
 *     stored value is always 1.0 / 0.0, so a y of 5.0 becomes 1.0. Without it y is never read (the BLAS rule for beta = 0).
 *   PLUS_TIMES through this entry point is g4s_spmv(A, x, y, 1.0, ACCUMULATE ? 1.0 : 0.0): the same kernels and the same result.
 *   min, max and or do not depend on the order in which products arrive, and each min/max-plus product is one IEEE add: the values of the three are exact and
 *   deterministic on every SpMV path (the blocked one included). Outside the contract, as for SpGEMM: the sign of a zero result, and the value of a row that
 *   has a NaN product or a (+inf) + (−inf) product (the other rows are unaffected).
 *   Concurrency and stream order are those of g4s_spmv: one product in flight per handle; the call only enqueues kernels on `stream` — no allocation, no
 *   synchronisation, no host read — and may be recorded in a hipGraph. New values from g4s_csr_update_values are used by the next call. */
#define G4S_SPMV_ACCUMULATE 2048u /* semiring SpMV: y := y ⊕ (A ⊗ x) instead of y := A ⊗ x */
g4s_status g4s_spmv_semiring(g4s_csr_t A, const double *x_dev, double *y_dev, unsigned flags, void *stream);
/* One-shot form, like g4s_spmv_csr_i32_f64 (synchronous). With host pointers y is uploaded only under G4S_SPMV_ACCUMULATE. */
g4s_status g4s_spmv_semiring_csr_i32_f64(int32_t rows, int32_t cols, const int32_t *rowptr, const int32_t *colids, const double *values,
                                         const double *x, double *y, unsigned flags);

/* ---- Transpose: Aᵀ of a rows × cols CSR as a cols × rows CSR (equivalently, the CSC form of A), on the device — the role of the reference's
 * CSR(const CSC&) / CSR(const CSC&, bool transpose) (mm/inc/CSR.h:171-230) and mm/inc/convert.h. Caller-allocated outputs: trowptr (cols + 1),
 * tcolids, tvalues and perm (nnz each).
 *   Order is stable: row j of Aᵀ lists the entries of column j of A in increasing entry index, so rows ascend and repeated columns keep their stored
 *     order. perm[k] is the entry of A that went to slot k, and tvalues[k] == values[perm[k]] bit for bit. In numpy terms: perm =
 *     argsort(colids, kind="stable"), tcolids = row_of_entry[perm], tvalues = values[perm], trowptr = the scan of the column counts — which is also
 *     scipy.sparse.csr_matrix(A).T.tocsr() without sum_duplicates. The result is the same on every run.
 *   Inputs follow the rules of g4s_csr_create: zero-based, rowptr non-decreasing, rowptr[0] == 0, rowptr[rows] == nnz <= INT32_MAX, colids in
 *     [0, cols). Rows need not be sorted; duplicates are kept, not summed. A violation returns G4S_ERR_INVALID and leaves the outputs unspecified.
 *   Optional outputs: values and tvalues may both be NULL (the pattern only; one without the other is G4S_ERR_INVALID); perm may be NULL.
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays; any other bit returns G4S_ERR_INVALID. Argument checks (sizes, NULLs, flag bits)
 *     come before any HIP call.
 *   Synchronous: runs on `stream` and returns when the outputs are complete; device inputs must be complete with respect to that stream. Scratch
 *     (about 24·nnz + 4·cols bytes, plus device copies of the arrays with G4S_HOST_POINTERS) is freed before the call returns. rows, cols or nnz of 0
 *     are valid (nnz == 0: trowptr is all zeros). */
g4s_status g4s_csr_transpose(int32_t rows, int32_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colids, const double *values,
                             int32_t *trowptr, int32_t *tcolids, double *tvalues, int32_t *perm, unsigned flags, void *stream);

/* Transposed products on a handle: y(cols) = alpha·Aᵀ·x(rows) + beta·y, and y := Aᵀ ⊗ x or y ⊕ (Aᵀ ⊗ x) over a semiring — pull-style graph
 * relaxation on a graph stored by out-edges (Bellman-Ford's d := d ⊕ (Aᵀ ⊗ d) above, BFS), and the Dᵀ of a Uzawa iteration, without a second matrix.
 *   g4s_csr_transpose_reserve runs g4s_csr_transpose on the handle's device arrays (NULL stream, synchronous), keeps perm, and creates an inner handle of
 *     Aᵀ on arrays of its own, with A's path flags (G4S_SPMV_NO_NT, _BLOCKED, _STREAM, _UPDATABLE) — for owned and borrowed handles alike.
 *     g4s_csr_destroy releases all of it. Peak device memory of a reserve: the kept arrays (4·(cols + 1) + 20·nnz bytes) plus the larger of the
 *     transpose's scratch (about 24·nnz bytes) and the inner g4s_csr_create's own transients.
 *   g4s_csr_transpose_info: the g4s_csr_info of the inner handle (rows = A's cols, its spmv_path, …); plan_bytes also counts the four kept arrays.
 *     G4S_ERR_INVALID before a reserve. g4s_csr_get_info(A) does not change.
 *   The products run the SpMV kernels of the inner handle, at the speed of a forward product on Aᵀ. Semiring flags, G4S_SPMV_ACCUMULATE, the beta == 0
 *     rule and the argument checks are those of g4s_spmv / g4s_spmv_semiring, with x of length rows and y of length cols. The semiring form takes exactly
 *     the flags of g4s_spmv_semiring; transposition never goes through a flag bit.
 *   Result: bit-identical to g4s_spmv / g4s_spmv_semiring on a handle created (G4S_DEVICE_POINTERS) from g4s_csr_transpose's output with the same flags —
 *     on every path for the three semirings, on paths 0, 3 and 4 for plus-times; on the blocked path plus-times is within 1e-10·Σ|a·x| (its LDS atomic
 *     sums are not reproducible run to run).
 *   First call without a reserve: reserves synchronously, like g4s_spmm; on a capturing stream it returns G4S_ERR_INVALID and enqueues nothing. After a
 *     reserve a call only enqueues kernels on `stream` and may be recorded in a hipGraph.
 *   g4s_csr_update_values(A, …) refreshes Aᵀ on the same stream when it exists: one gather tvalues[k] = values[perm[k]], then the inner handle's own
 *     update under the same rules (one pass with G4S_SPMV_UPDATABLE). One product in flight per handle, forward or transposed. */
g4s_status g4s_csr_transpose_reserve(g4s_csr_t A);
g4s_status g4s_csr_transpose_info(g4s_csr_t A, g4s_csr_info *info);
g4s_status g4s_spmv_transpose(g4s_csr_t A, const double *x_dev, double *y_dev, double alpha, double beta, void *stream);
g4s_status g4s_spmv_semiring_transpose(g4s_csr_t A, const double *x_dev, double *y_dev, unsigned flags, void *stream);

/* ---- Graph traversal on a handle: single- / multi-source shortest paths (g4s_sssp) and BFS levels (g4s_bfs), device-resident, with a per-step choice
 * between a push from the frontier and the dense pull d := d ⊕ (Aᵀ ⊗ d) — the loops a caller would otherwise write around g4s_spmv_semiring_transpose.
 * A is square and stored by OUT-edges: row i lists the edges i → j with weight a_ij.
 *   sources: a HOST array of n_sources >= 1 vertex ids (repeats allowed); all start at distance 0 / level 0, so the result is the distance to the nearest
 *     source. dist_dev (rows doubles) / level_dev (rows int32) are device arrays that are only written: their old content is never read. Unreached
 *     vertices get +inf / −1. info may be NULL.
 *   g4s_sssp computes the min-plus fixed point of d := d ⊕ (Aᵀ ⊗ d) from d[sources] = 0; every stored entry of a row takes part (repeated columns
 *     included, as in g4s_spmv_semiring). max_iterations == 0 means rows. The result is exact and does not depend on the schedule: IEEE addition is
 *     monotone (a <= b ⇒ fl(a + w) <= fl(b + w)), so any order of relaxations — the synchronous pull, a push in whatever order its atomics land, any
 *     mixture — ends at d[v] = min over paths of the path sum rounded left to right. Push, pull and auto therefore agree bit for bit, with each other
 *     and from run to run. Outside the contract, as for the semiring SpMV: NaN weights, (+inf) + (−inf), the sign of a zero.
 *     Negative weights are allowed. With a negative cycle reachable from a source there is no fixed point: the call stops at the cap and reports
 *     converged = 0. Whenever converged == 0, every path of at most `iterations` edges has been relaxed: dist holds upper bounds with
 *     final <= dist[v] <= (the synchronous result after `iterations` rounds).
 *   g4s_bfs writes the hop count. A stored entry is an edge under the or-and rule: a_ij != 0 (NaN counts as nonzero), so the levels are those of the
 *     or-and loop over g4s_spmv_semiring. max_depth == 0 means no cap; with a cap, vertices beyond it stay −1 and converged = 0 if the last frontier
 *     was not empty. Levels are unique, hence the same in every direction. Whether any stored value is zero is found once (at the reserve, and again
 *     after g4s_csr_update_values); without one, BFS never reads the values.
 *   Direction: by default chosen per step — push while the frontier's out-edges are at most nnz / α, pull otherwise; α = 8 for g4s_sssp and 1 for
 *     g4s_bfs (the measured switch points, DESIGN §4.6 and profiles/traverse.txt; the environment variable G4S_TRAVERSE_ALPHA replaces both).
 *     G4S_TRAVERSE_PUSH / G4S_TRAVERSE_PULL force one.
 *   Where it loses: on a graph whose traversal is a handful of dense steps the host loop over g4s_spmv_semiring_transpose is faster — configs[1]
 *     (10 M R-MAT, 8 steps from the hub): 3.8 ms for the loop against 8.4 ms (SSSP) and 4.0 against 14.0 ms (BFS); every vertex a step changes is
 *     appended to the next frontier through one tail counter, which bounds a step at about 7 G edges/s. It wins where steps are many and frontiers
 *     small — the 1000 × 1000 grid, 2053 steps: 80.6 against 112.6 ms (SSSP), 34.8 against 128.7 ms (BFS).
 *   flags: G4S_TRAVERSE_PUSH, G4S_TRAVERSE_PULL (both together: G4S_ERR_INVALID), G4S_TRAVERSE_SYMMETRIC; any other bit, a NULL handle, sources or
 *     output, n_sources < 1 and a negative cap return G4S_ERR_INVALID before any HIP call. A non-square handle and a source outside [0, rows) return
 *     G4S_ERR_INVALID before anything is enqueued. No other entry point accepts these bits.
 *   Synchronous: the call runs on `stream` and returns when the output is complete. It reads its state back (once per batch of at least
 *     G4S_TRAVERSE_BATCH push steps, once per pull step: info.host_waits), so it cannot be captured: on a capturing stream it returns G4S_ERR_INVALID
 *     and enqueues nothing. One traversal or product in flight per handle.
 *   g4s_csr_traverse_reserve builds what the calls need (NULL stream, synchronous): two frontier queues and a mark per vertex (3·rows ints), the pull
 *     step's vector (rows doubles), an 80-byte state block, and the handle's transpose through g4s_csr_transpose_reserve — unless the flags hold
 *     G4S_TRAVERSE_SYMMETRIC or G4S_TRAVERSE_PUSH (which never pulls); a later auto or pull call then reserves the rest. A first call without a
 *     reserve reserves synchronously; after a reserve a call allocates nothing on the device. g4s_csr_destroy releases all of it,
 *     g4s_csr_get_info(A).plan_bytes counts the workspace (the transpose is counted by g4s_csr_transpose_info). g4s_csr_update_values needs nothing
 *     new: push reads the handle's current value array, pull the refreshed Aᵀ. */
#define G4S_TRAVERSE_PUSH       4096u  /* every step pushes from the frontier                                                          */
#define G4S_TRAVERSE_PULL       8192u  /* every step is the dense pull d := d ⊕ (Aᵀ ⊗ d)                                              */
#define G4S_TRAVERSE_SYMMETRIC 16384u  /* the caller declares A == Aᵀ (pattern and values): the pull runs on A itself, no transpose    */
#define G4S_TRAVERSE_BATCH 16          /* push steps enqueued behind one read of the state, at least (doubles up to 64 within a call)  */
typedef struct g4s_traverse_info {
    int32_t iterations;      /* steps run, push + pull                                                  */
    int32_t converged;       /* 1: fixed point / empty frontier; 0: stopped at the iteration cap        */
    int32_t push_steps, pull_steps;
    int32_t host_waits;      /* times the call waited for the device                                    */
    int32_t reserved;
    int64_t reached;         /* vertices with a finite distance / a level >= 0                          */
    int64_t edges_relaxed;   /* edges walked by push steps + nnz per pull step                          */
} g4s_traverse_info;
g4s_status g4s_csr_traverse_reserve(g4s_csr_t A, unsigned flags);
g4s_status g4s_sssp(g4s_csr_t A, const int32_t *sources, int32_t n_sources, double *dist_dev, int32_t max_iterations, unsigned flags,
                    g4s_traverse_info *info, void *stream);
g4s_status g4s_bfs(g4s_csr_t A, const int32_t *sources, int32_t n_sources, int32_t *level_dev, int32_t max_depth, unsigned flags,
                   g4s_traverse_info *info, void *stream);

/* ---- PageRank on a handle (g4s_pagerank): power iteration, device-resident — the loop a caller would otherwise write around g4s_spmv_transpose and
 * four or five vector operations, with a host read of the residual per iteration. The result is networkx's `pagerank` with dangling = personalization.
 * A is square and stored by OUT-edges: row u lists the edges u → v with weight a_uv; repeated columns add. An unweighted graph is a handle whose
 * values are all 1.
 *   Out-strength s_u = Σ_v a_uv; a vertex with s_u == 0 is dangling (an empty row, or a row whose weights are all zero). Weights must be finite and
 *     >= 0: the call checks this on the device in its strength pass; a violation returns G4S_ERR_INVALID and leaves rank_dev unspecified.
 *   Teleport vector p = personalization_dev / Σ personalization_dev: n doubles on the device, read only, finite and >= 0 with a sum > 0 (otherwise
 *     G4S_ERR_INVALID); NULL: p_v = 1.0 / n.
 *   One iteration, in this order of operations (the library is built with -ffp-contract=off):
 *       x_u = r_u · (1 / s_u), or 0 for a dangling u;   y = Aᵀ·x;   m = Σ_{u dangling} r_u;
 *       r'_v = damping · (y_v + m · p_v) + (1 − damping) · p_v;   residual = Σ_v |r'_v − r_v|.
 *   Stop: after the first iteration with residual < tol (strict: tol == 0 runs exactly max_iterations), or at the cap; max_iterations == 0 means 100.
 *   Start: r_0 = p; with G4S_PAGERANK_WARM_START r_0 = rank_dev / Σ rank_dev (the rules of p). rank_dev (n doubles, device) receives the ranks.
 *   Accuracy: every quantity is non-negative and the iteration contracts in L1 by `damping`, so after the same number of iterations the result is
 *     within γ / (1 − damping) in L1 of the exact iteration, γ = (max in-degree + max out-degree + ⌈log₂ n⌉ + 16) · 2⁻⁵³, whatever the order of the
 *     sums (tests/test_pagerank_gpu.py has the derivation). residual and the dangling mass are summed in a fixed order on a grid that depends on n
 *     only: the same bits on every run; the ranks too wherever the product is reproducible (every path but the blocked one).
 *   Checked before any HIP call (G4S_ERR_INVALID): a NULL handle or rank_dev, damping outside [0, 1) or NaN, tol < 0 or NaN, a negative cap, a flag
 *     bit other than the two below. A non-square handle returns G4S_ERR_INVALID before anything is enqueued. No other entry point accepts these bits.
 *   Synchronous: the call runs on `stream` and returns when rank_dev is complete. It reads its state back once per batch of at least
 *     G4S_PAGERANK_BATCH iterations (info.host_waits; later batches are sized from the geometric decay of the residual), so it cannot be captured: on
 *     a capturing stream it returns G4S_ERR_INVALID and enqueues nothing. Iterations enqueued behind the stop cost their product (info.products) and
 *     change nothing. One product, traversal or PageRank in flight per handle.
 *   g4s_csr_pagerank_reserve builds what the calls need (NULL stream, synchronous): 1 / s, x, y and the normalised p (4·n doubles), 16 KiB of
 *     per-workgroup partial sums, a 64-byte state block, the strength pass, and the handle's transpose through g4s_csr_transpose_reserve — unless
 *     the flags hold G4S_PAGERANK_SYMMETRIC. A first call without a reserve reserves synchronously; after a reserve a call allocates nothing on the
 *     device. g4s_csr_get_info(A).plan_bytes counts the workspace (the transpose is counted by g4s_csr_transpose_info); g4s_csr_destroy releases it.
 *     After g4s_csr_update_values the next call runs the strength pass again, on its stream.
 *   Out of scope: several teleport vectors at once through g4s_spmm, a pattern-only mode on a handle with arbitrary values, a capturable form, the
 *     distributed handle. */
#define G4S_PAGERANK_SYMMETRIC   65536u  /* the caller declares A == Aᵀ (pattern and values): products run on A itself, no transpose */
#define G4S_PAGERANK_WARM_START 131072u  /* rank_dev holds the starting vector (normalised inside); default start: the teleport vector */
#define G4S_PAGERANK_BATCH 8             /* iterations enqueued behind one read of the state, at least */
typedef struct g4s_pagerank_info {
    int32_t iterations;   /* iterations that changed rank */
    int32_t converged;    /* 1: residual < tol; 0: stopped at the cap */
    int32_t host_waits;   /* times the call waited for the device */
    int32_t products;     /* products enqueued, those behind the stop included */
    int64_t dangling;     /* vertices of zero out-strength */
    double  residual;     /* ‖r_k − r_{k−1}‖₁ of the last iteration */
} g4s_pagerank_info;
g4s_status g4s_csr_pagerank_reserve(g4s_csr_t A, unsigned flags);
g4s_status g4s_pagerank(g4s_csr_t A, double damping, double tol, int32_t max_iterations,
                        const double *personalization_dev, double *rank_dev, unsigned flags,
                        g4s_pagerank_info *info, void *stream);

/* ---- Betweenness centrality on a handle (g4s_betweenness): Brandes' algorithm, one BFS that counts shortest paths and one dependency sweep per
 * source, both device-resident — what neither g4s_bfs (it keeps no path counts and forgets its frontiers) nor a host loop over g4s_spmv_semiring
 * (no semiring expresses the σ_u / σ_v · (1 + δ_v) recurrence) can give. A is square and stored by OUT-edges: row u lists the edges u → v.
 *   Edges: a stored entry is an edge under g4s_bfs's or-and rule, a_uv != 0 (NaN counts as an edge); the weight itself is not used. Values are read
 *     only when a stored zero exists; that verdict is taken at the reserve and again after g4s_csr_update_values. Repeated columns are PARALLEL
 *     edges: each carries its own shortest paths.
 *   sources: a HOST array of n_sources >= 1 vertex ids, as for g4s_bfs. Each listed source is one traversal, in the order given; a repeated source
 *     counts twice.
 *   For a source s: level = BFS depth; σ[s] = 1, σ[v] = Σ σ[u] over the edges u → v with level[u] = level[v] − 1 (the number of shortest paths);
 *     from the deepest level upwards δ[u] = Σ over the edges u → v with level[v] = level[u] + 1 of (σ[u] / σ[v]) · (1 + δ[v]); δ[s] = 0, and an
 *     unreached vertex has δ = 0.
 *   Result: bc_dev[v] = scale · Σ_s δ_s(v) (rows doubles on the device, only written) — with G4S_BC_ACCUMULATE bc_dev[v] + scale · Σ_s δ_s(v), so a
 *     long source list may be split over calls. This is the sum over s of networkx's betweenness_centrality_subset(G, [s], all nodes,
 *     normalized=False) on a DiGraph without parallel edges; scale = 0.5 with every vertex as a source gives networkx's undirected value on a
 *     symmetric A, 1 / ((n − 1)(n − 2)) the normalised directed one.
 *   Exactness: σ is fp64. While every σ <= 2^53 the path counts are integers and their sums exact in whatever order the atomics of the forward step
 *     land; δ and the sum over sources are formed without atomics in an order that depends on the graph and the source list only (fixed lanes per
 *     row, fixed shuffle trees, sources one after the other). The result is then the same bits on every run, stream and launch grid, and
 *     info.sigma_exact = 1. Above 2^53 (sigma_exact = 0) σ carries rounding that depends on the order of arrival: the result stays within 1e-10
 *     relative of the exact one but need not repeat bit for bit. A σ that overflows to infinity returns G4S_ERR_OVERFLOW with bc_dev unspecified
 *     (a 1000 × 1000 grid from a corner reaches about 2^1994); it is detected on the device, one maximum per source read with the state, and the
 *     handle stays usable.
 *   Checked before any HIP call (G4S_ERR_INVALID, g4s_last_error names the argument): a NULL handle, sources or bc_dev, n_sources < 1, a scale
 *     that is not finite, a flag bit other than G4S_BC_ACCUMULATE (the reserve accepts no bit). Before anything is enqueued: a non-square handle, a
 *     source outside [0, rows), a capturing stream. No other entry point accepts the bit.
 *   Synchronous: the call runs on `stream` and returns when bc_dev is complete. The forward half is one kernel per level, enqueued blind in batches
 *     of at least G4S_BC_BATCH (doubling to 64 within a traversal) with one read of the 104-byte state per batch; the backward half is one kernel
 *     per level (two on a handle with a row above 4096 entries) without reads. info.host_waits <= ⌈levels / G4S_BC_BATCH⌉ + 2·sources. One product,
 *     traversal, PageRank or betweenness call in flight per handle.
 *   g4s_csr_betweenness_reserve builds what the calls need (NULL stream, synchronous): level, order — all frontiers of a traversal one behind the
 *     other — and level_start (3·rows + 2 ints), two hub lists of min(rows, nnz / 4097) + 1 ints, rows + 2 bytes of lanes-per-level, σ, δ and the
 *     sum over sources (3·rows doubles) and the state block: 4·(3·rows + 2 + 2·hub) + (rows + 2) + 24·rows + 104 bytes. No transpose: forward
 *     pushes along A, backward pulls along the out-edges of A. A first call without a reserve reserves synchronously; after a reserve a call
 *     allocates nothing on the device. g4s_csr_get_info(A).plan_bytes counts the workspace, g4s_csr_destroy releases it.
 *   Where it loses: one level is one launch in each direction, about 2·depth launches per source, so a deep graph (a grid, a road network) is
 *     launch-bound; the sources run one after the other, so a small graph never fills the device (profiles/betweenness.txt).
 *   Out of scope: several sources at once, direction switching (a bottom-up forward step), a weighted (Dijkstra) form, edge betweenness, a
 *     capturable form, the distributed handle. */
#define G4S_BC_ACCUMULATE 262144u   /* bc_dev holds earlier results: bc := bc + scale·Σ_s δ_s instead of bc := scale·Σ_s δ_s */
#define G4S_BC_BATCH 16             /* forward steps enqueued behind one read of the state, at least */
typedef struct g4s_bc_info {
    int32_t sources;       /* traversals run (= n_sources) */
    int32_t max_depth;     /* deepest BFS level over all sources */
    int32_t host_waits;    /* times the call waited for the device */
    int32_t sigma_exact;   /* 1: every path count stayed <= 2^53, so all σ are exact integers and the result is schedule-independent */
    int64_t levels;        /* forward steps, summed over sources (deepest level + 1 per source) */
    int64_t reached;       /* vertices reached, summed over sources */
    int64_t edges_walked;  /* forward + backward */
    double  sigma_max;     /* largest path count met */
} g4s_bc_info;             /* 48 bytes */
g4s_status g4s_csr_betweenness_reserve(g4s_csr_t A, unsigned flags);
g4s_status g4s_betweenness(g4s_csr_t A, const int32_t *sources, int32_t n_sources, double scale,
                           double *bc_dev, unsigned flags, g4s_bc_info *info, void *stream);
g4s_status g4s_spgemm_csr_i32_f64(const int32_t *arpt, const int32_t *acol, const double *aval,
                                  const int32_t *brpt, const int32_t *bcol, const double *bval,
                                  int32_t **crpt, int32_t **ccol, double **cval,
                                  int32_t M, int32_t K, int32_t N, int64_t *cnnz,
                                  g4s_timings *timings, unsigned flags);

/* Two-phase form (hash_symbolic / hash_numeric, mm/inc/hash_mult.h:496-508,559-608) on device pointers:
 * symbolic writes crpt_dev[M+1] (int32) and *cnnz; numeric fills ccol_dev/cval_dev (cnnz entries each).
 * The symbolic call keeps what it learned about the product (the sorted columns of the long rows, the column map of B, B's window splits) for the numeric
 * call that follows it with THE SAME arrays (same pointers, unchanged contents — crpt describes this product and no other): that call then does not traverse
 * the structure again (the pair costs what the one-call form costs), nor do further numeric calls on the same arrays (new VALUES of A or B, same pattern: the
 * time-stepping case). One product at a time per process: the next symbolic or one-call product, g4s_trim
 * and g4s_shutdown release whatever is still held. The state is keyed by the pointers AND by a hash of the five index arrays (arpt, acol, brpt, bcol, crpt)
 * taken at the end of the symbolic call and checked at the start of every numeric call that would use it: a numeric call with other arrays, with the same
 * buffers refilled by another pattern, with its own crpt, or without a symbolic call before it derives everything it needs itself (no carried state is used). */
g4s_status g4s_spgemm_symbolic(int32_t M, int32_t K, int32_t N,
                               const int32_t *arpt_dev, const int32_t *acol_dev,
                               const int32_t *brpt_dev, const int32_t *bcol_dev,
                               int32_t *crpt_dev, int64_t *cnnz, void *stream);
g4s_status g4s_spgemm_numeric(int32_t M, int32_t K, int32_t N,
                              const int32_t *arpt_dev, const int32_t *acol_dev, const double *aval_dev,
                              const int32_t *brpt_dev, const int32_t *bcol_dev, const double *bval_dev,
                              const int32_t *crpt_dev, int32_t *ccol_dev, double *cval_dev,
                              unsigned flags, void *stream);

/* ---- Masked SpGEMM: C⟨M⟩ = A ⊗ B, the product computed only at the positions of a given pattern M — what g4s_spgemm_csr_i32_f64 followed by a
 * selection of M's entries gives, without the full product: no symbolic phase, no output allocation, no crpt (the pattern of C is M), so it also works
 * where the full product exceeds the int32 crpt (G4S_ERR_OVERFLOW). Triangle counting, clustering coefficients, k-truss support, common-neighbour
 * scores of given pairs and sampled distance products are all of this shape.
 *   A is M×K, B is K×N, the mask an M×N pattern (mrpt, mcol; no values). cval is caller-allocated, mrpt[M] doubles, only written.
 *   Values: entry k = (i, j = mcol[k]) gets ⊕ over all products a_ip ⊗ b_pj with a stored a_ip and a stored b_pj (repeated columns in a row of A or B
 *     each take part, as in g4s_spgemm_*), and the semiring's identity (0.0, +inf, −inf, 0.0) where there is none: the value the full product of the
 *     same semiring has at (i, j), or the identity where it has no entry. Products whose column is not in the mask row are dropped.
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays (host: upload, run, copy cval back) and one G4S_SEMIRING_* value. Any other bit
 *     returns G4S_ERR_INVALID before any HIP call, and so do a NULL arpt, acol, brpt, bcol, mrpt or cval, a negative size, and a NULL mcol unless M == 0.
 *   Pattern-only: aval == NULL && bval == NULL makes every stored value of A and B count as 1.0, and no value array is read (4 instead of 12 bytes
 *     per product). Plus-times then counts the products of an entry (exact below 2^53), or-and gives 1.0 exactly where a product exists — the
 *     structural hit pattern that a plus-times value of 0.0 cannot give. One NULL without the other is G4S_ERR_INVALID.
 *   Inputs: A and B follow the SpGEMM input contract above (rows in any order, repeated columns, ids range-checked). The rows of the MASK must be
 *     strictly ascending (sorted, no repeats) with ids in [0, N) and mrpt non-decreasing from 0: checked on the device in the opening pass,
 *     G4S_ERR_INVALID, cval unspecified afterwards. The mask arrays may be the very arrays of A or B (C⟨A⟩ = A·A is the common call); cval must not
 *     overlap an input (G4S_ERR_INVALID).
 *   Exactness: min-plus, max-plus and or-and are exact and deterministic in every row class (min, max and or do not depend on the order of arrival;
 *     outside the contract, as for the SpGEMM semirings: NaN, (+inf) + (−inf), the sign of a zero). Plus-times is within 1e-10·Σ|a·b| of the entry's
 *     left-to-right sum and bit-exact whenever every partial sum is representable (integer values, pattern-only).
 *   Synchronous: runs on `stream` and returns when cval is complete. It classifies rows from counts it reads back, so on a capturing stream it
 *     returns G4S_ERR_INVALID and enqueues nothing (the rule of g4s_sssp). Scratch (16·M bytes, plus device copies of the arrays with host pointers)
 *     comes from the library's caching allocator and is released before the call returns. M, nnz(A), nnz(B) or nnz(M) of 0 are valid (cval all identity
 *     / nothing written). info may be NULL.
 *   Row classes (g4s_masked_info says which a row took): a mask row of at most 64 entries with at most 4096 products runs on one
 *     wavefront; up to 8192 entries the mask row is a table in LDS of one workgroup; a longer one is searched in HBM with global atomics; a row of more
 *     than 2^20 products is divided over up to 128 workgroups (an LDS table each when the mask row has at most 1024 entries, else the HBM search).
 *     Lookup is a binary search over the sorted mask row after a clip to [min, max] of the row.
 *   Where it loses: every product is walked even when the mask keeps a handful — a mask much sparser than the product wants the dot-product
 *     formulation on Bᵀ, which is not built. A split row is divided by entries of A, so a row whose products sit in a few very long rows of B stays
 *     on few workgroups. Against the full product alone it is level on a dense mask (R-MAT-18, edge factor 16, mask = A: 22.6 against 23.3 ms) and
 *     ahead where the output dominates (configs[2]: 17.7 against 26.8 ms; 65.3 ms with the selection); pattern-only gains only 4–6 %, the walk is
 *     bound by the lookups (profiles/spgemm_masked.txt). */
typedef struct g4s_masked_info {
    int64_t mask_nnz;        /* mrpt[M]                                                                                          */
    int64_t products;        /* Σ over rows i with a non-empty mask row of Σ_{p ∈ A(i,:)} nnz(B(p,:)): products looked up           */
    int32_t rows_wave;       /* rows handled by the wavefront-per-row class                                                       */
    int32_t rows_lds;        /* rows whose mask row was a table in LDS (split ones included)                                      */
    int32_t rows_global;     /* rows whose mask row was too long for LDS: searched in HBM, global atomics (split ones included)   */
    int32_t rows_split;      /* rows whose products were divided over several workgroups                                          */
} g4s_masked_info;
g4s_status g4s_spgemm_masked(int32_t M, int32_t K, int32_t N,
                             const int32_t *arpt, const int32_t *acol, const double *aval,
                             const int32_t *brpt, const int32_t *bcol, const double *bval,
                             const int32_t *mrpt, const int32_t *mcol,
                             double *cval, unsigned flags, g4s_masked_info *info, void *stream);

/* Triangle counting: *triangles (host) = the number of vertex triples i > j > k for which (i, j), (i, k) and (j, k) are all stored in the strictly
 * lower triangle L of the n×n pattern — for the symmetric pattern of a simple undirected graph, its number of triangles. Entries on and above the
 * diagonal are ignored, so a full symmetric matrix, its lower triangle alone, and either with self-loops give the same number.
 *   Rows must be strictly ascending with ids in [0, n) (checked on the device, G4S_ERR_INVALID): L(i) is then a prefix of row i; L is compacted into
 *     a CSR of its own (4·(n + 1) + 12·nnz(L) bytes of scratch with its values) and the count is Σ cval of the pattern-only plus-times product
 *     L·L⟨L⟩, summed on the device in int64 in a fixed order (the summands are integers).
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS only; any other bit, a NULL rowptr or triangles, a NULL colids with n > 0 and a negative n return
 *     G4S_ERR_INVALID before any HIP call. Synchronous, not capturable, info as for g4s_spgemm_masked (of the product L·L⟨L⟩).
 *   Per-vertex and per-edge counts are one g4s_spgemm_masked call on L away. Where it loses: vertices are taken in the order given — no degree
 *     reordering, so the hub rows of a skewed graph keep their full lower neighbourhoods as mask rows: configs[1] symmetrised (97.9 M edges) takes
 *     533 ms for 74.9 G products, of which 4 454 hub rows are split (profiles/spgemm_masked.txt). */
g4s_status g4s_triangle_count(int32_t n, const int32_t *rowptr, const int32_t *colids,
                              int64_t *triangles, unsigned flags, g4s_masked_info *info, void *stream);

/* Connected components: labels[v] (n int32, device or host like the other arrays, only written — its old content is never read) = the smallest vertex
 * id in v's component, for the WEAKLY connected components of the graph on vertices 0 … n−1 whose edges are the stored entries of the n×n pattern,
 * direction ignored. Raw arrays, no handle and no plan: the call reads the pattern only.
 *   Every stored entry is an edge, whatever its value (no value array is passed: g4s_triangle_count's rule, and what
 *     scipy.sparse.csgraph.connected_components does with an explicitly stored zero). Self-loops, repeated columns, unsorted rows and empty rows are
 *     valid and change nothing; an isolated vertex is a component of its own.
 *   Labels are canonical: labels[v] <= v, labels[labels[v]] == labels[v], a component's root is its vertex with labels[v] == v. The result is the
 *     same on every run, for every schedule and every tuning switch, and is compared with ==, never up to a relabelling.
 *   G4S_CC_SYMMETRIC: the caller declares the PATTERN symmetric ((i,j) stored ⇔ (j,i) stored). It allows the one optimisation that needs it: after the
 *     sampling rounds the rows of the most frequent sampled label are not walked again (info.skipped), which is only sound when every edge is also
 *     stored from its other end. Without the flag the pattern may be anything — a directed graph, an upper triangle alone — and the result is that of
 *     the symmetrised pattern. With the flag on a pattern that is NOT symmetric the call still terminates and writes ids in [0, n) with
 *     labels[v] <= v, but components may come out split: outside the contract.
 *   Algorithm: a union-find forest in `labels` itself, "smaller id wins", in the shape of Afforest — two sampling rounds (vertex v hooks
 *     to its r-th neighbour), pointer-jumping compress, the remaining entries balanced over edges (rows above 4096 entries in chunks of 1024 over all
 *     workgroups), compress. Hooks are one compare-and-swap on a root; a failed one continues from the value it returned towards strictly smaller
 *     ids, so every loop is bounded and nothing waits on another workgroup.
 *   Checks: any flag bit other than G4S_DEVICE_POINTERS and G4S_CC_SYMMETRIC, a NULL rowptr or labels, a NULL colids with n > 0 and a negative n
 *     return G4S_ERR_INVALID before any HIP call. On the device, before any id is dereferenced: rowptr[0] == 0, rowptr non-decreasing (so
 *     rowptr[n] <= INT32_MAX entries), ids in [0, n) — G4S_ERR_INVALID, labels unspecified afterwards. n == 0 (nothing written) and nnz == 0
 *     (labels[v] = v) are valid. labels must not overlap rowptr or colids. info may be NULL.
 *   Synchronous: runs on `stream` and returns when labels and info are complete; no decision is taken on the host between kernels, so the call
 *     waits for the device once (info.host_waits). On a capturing stream it returns G4S_ERR_INVALID and enqueues nothing. Scratch — a 512-byte
 *     state block, 4·n bytes for the component sizes, 4·min(n, 2^19) bytes for the list of long rows, plus device copies of rowptr, colids and labels
 *     with host pointers — comes from the library's caching allocator and is released before the call returns.
 *   Environment: G4S_CC_SAMPLE_ROUNDS = 0 … 4 (default 2), G4S_CC_NO_SKIP=1 (never skip, flag or not). Labels do not depend on them.
 *   Where it loses: not known yet — the comparison with the min-plus label-propagation loop over g4s_spmv_semiring / g4s_spmv_semiring_transpose
 *     and with scipy on the host (tools/bench_components.py) has not been recorded; profiles/components.txt holds the protocol and DESIGN §4.8 the
 *     expectation (the loop needs diameter-many rounds, so it should lose on a grid; on a graph of small diameter such as configs[1] it may not). */
#define G4S_CC_SYMMETRIC 32768u   /* the caller declares the PATTERN symmetric: (i,j) stored ⇔ (j,i) stored */
typedef struct g4s_cc_info {
    int64_t components;      /* number of distinct labels (isolated vertices and empty rows count)              */
    int64_t largest;         /* vertices in the largest component                                                */
    int64_t edges_linked;    /* stored entries that went through the link step after the sampling rounds          */
    int32_t largest_label;   /* its label (the smallest one among components of that size)                        */
    int32_t sample_rounds;   /* neighbour-sampling rounds run                                                     */
    int32_t skipped;         /* 1: vertices of the sampled largest component were skipped in the link step        */
    int32_t host_waits;      /* times the call waited for the device                                              */
} g4s_cc_info;               /* 40 bytes */
g4s_status g4s_connected_components(int32_t n, const int32_t *rowptr, const int32_t *colids,
                                    int32_t *labels, unsigned flags, g4s_cc_info *info, void *stream);

/* k-core decomposition: core[v] (n int32, device or host like the other arrays, only written) = the largest k such that v belongs to a subgraph in
 * which every vertex has at least k neighbours — what networkx.core_number returns on the graph without self-loops; an isolated vertex has core 0.
 * Raw arrays, no handle, no plan, no values: the call reads the pattern only.
 *   Pattern: the adjacency of a simple undirected graph. Rows strictly ascending with ids in [0, n), rowptr non-decreasing from 0: all of it checked
 *     on the device before any id is an index (G4S_ERR_INVALID, outputs unspecified afterwards: the rule of g4s_triangle_count). The caller declares
 *     the pattern symmetric; symmetry is not checked. On a pattern that is not, the call still terminates and writes core[v] in [0, row length], but
 *     the values are outside the contract. A stored diagonal entry is ignored: not counted in a degree, not walked.
 *   round[v] (n int32, may be NULL): the graph is peeled level by level — k = the smallest remaining degree, never decreasing — and inside a level
 *     frontier by frontier: a frontier is ALL remaining vertices of degree <= k, removed at once; the next frontier is the vertices that this removal
 *     brought to <= k. round[v] is the 0-based index, over the whole call, of the non-empty frontier that removed v. That partition is a function of
 *     the graph alone, so core and round are the same on every run, stream and launch grid and are compared with ==. Sorting the vertices by
 *     (round, id) gives a degeneracy ordering: every vertex has at most core[v] neighbours at or after its own position.
 *   max_k: only the levels k < max_k are peeled. The vertices still present afterwards — exactly the max_k-core — get core = max_k and round = −1, and
 *     info.capped = 1. INT32_MAX asks for the full decomposition; a negative max_k is G4S_ERR_INVALID.
 *   Checks before any HIP call (G4S_ERR_INVALID): any flag bit other than G4S_DEVICE_POINTERS, a NULL rowptr or core, a NULL colids with n > 0, a
 *     negative n or max_k, and with host pointers outputs that overlap the inputs or each other. n == 0 is valid and writes nothing; nnz == 0 is
 *     valid: every core is 0 and every round is 0. info may be NULL.
 *   Algorithm: deg[v] = row length minus the diagonal. A scan over all vertices collects those with deg <= k into the frontier; when it
 *     collects none it raises k to the smallest remaining degree, so a non-empty level costs at most two scans. A peel walks the frontier's rows
 *     balanced over entries (rows above 4096 entries in chunks of 1024 over all workgroups): a plain load of deg[v], skipped when <= k, else one
 *     atomic decrement — the lane that brings v from k + 1 to k appends it. Every vertex is queued once, so one array of n ints holds all frontiers.
 *   Synchronous: runs on `stream` and returns when core, round and info are complete. Scans and peels are enqueued blind in batches of at least
 *     G4S_KCORE_BATCH launches (doubling to 64) with one read of the 104-byte state per batch: info.host_waits <= info.launches / 16 + 2. The peel
 *     grid follows the frontier seen at the last read; a frontier that outgrows it stops the batch, which resumes on a larger grid (info.resumes).
 *     On a capturing stream it returns G4S_ERR_INVALID and enqueues nothing. Scratch — a 256-byte state block, 4·n bytes of remaining degrees, 4·n
 *     for the queue, two lists of 4·min(n, 2^19) for long rows, plus device copies of the arrays with host pointers — comes from the library's
 *     caching allocator and is released before the call returns. No process-wide state: different host threads may call at the same time.
 *   Environment: G4S_KCORE_SCAN_WGS (the cap on the scan's workgroups, default one per CU), G4S_KCORE_MIN_GRID (the smallest peel grid,
 *     default 8). The outputs do not depend on them.
 *   Where it loses (profiles/kcore.txt, one MI355X): against the host loop of g4s_spmv on an alive vector plus torch compares it wins on all three
 *     graphs measured — 18.8 against 61.2 ms on the 1000 × 1000 grid, 246 against 822 ms on configs[1] symmetrised — but only 1.6x on the symmetrised
 *     R-MAT-20 (54.6 against 87.8 ms), and it runs far below the walk's own rate everywhere (0.29 G entries/s there): it is bound by the number of
 *     dependent kernels, and inside the few dense rounds by one atomic per entry and one tail counter per append. A small-diameter graph of few dense
 *     rounds is its worst case, a graph of many sparse levels pays two scans over all vertices per level. */
#define G4S_KCORE_BATCH 16          /* step launches enqueued behind one read of the state, at least (doubles up to 64 within a call) */
typedef struct g4s_kcore_info {
    int64_t edges_walked;    /* stored entries walked by peel rounds                                  */
    int64_t top_core_size;   /* vertices whose core number equals `degeneracy`                        */
    int32_t degeneracy;      /* the largest core number written (max_k when capped)                   */
    int32_t levels;          /* distinct k at which at least one vertex was removed                   */
    int32_t rounds;          /* non-empty frontiers peeled = 1 + the largest value written to `round` */
    int32_t scans;           /* passes over all vertices that did work                                */
    int32_t launches;        /* kernels enqueued, those that returned at once included                */
    int32_t resumes;         /* batches restarted because the frontier outgrew the launch grid        */
    int32_t host_waits;      /* times the call waited for the device                                  */
    int32_t capped;          /* 1: max_k ended the peeling with vertices left                         */
} g4s_kcore_info;            /* 48 bytes */
g4s_status g4s_kcore(int32_t n, const int32_t *rowptr, const int32_t *colids, int32_t max_k,
                     int32_t *core, int32_t *round /* may be NULL */, unsigned flags,
                     g4s_kcore_info *info /* may be NULL */, void *stream);

/* Strongly connected components: labels[v] (n int32, device or host like the other arrays, only written) = the smallest vertex id in v's strongly
 * connected component, for the directed graph on vertices 0 … n−1 in which every stored entry (u, v) of the n×n pattern is an edge u → v — the
 * directed counterpart of g4s_connected_components, and scipy.sparse.csgraph.connected_components(connection="strong") with canonical labels. Raw
 * arrays, no handle, no plan, no values: a stored entry is an edge whatever its value.
 *   Self-loops, repeated columns, unsorted rows and empty rows are valid and change nothing; a vertex on no cycle through another vertex is a
 *     component of its own, with or without a self-loop.
 *   Labels are canonical as g4s_connected_components': labels[v] <= v, labels[labels[v]] == labels[v]. They are the same on every run, stream, launch
 *     grid and tuning switch, and are compared with ==, never up to a relabelling.
 *   trowptr / tcolids: the pattern of Aᵀ (n + 1 and rowptr[n] entries), for a caller who has it — from g4s_csr_transpose, or because the same graph
 *     is used again. Both given or both NULL; one without the other is G4S_ERR_INVALID. With both NULL the call builds them itself through
 *     g4s_csr_transpose on device arrays (info.built_transpose = 1): 4·(n + 1) + 4·nnz bytes for the result plus that call's own scratch (about
 *     28·nnz + 4·n bytes) and its three waits. A given pair that is NOT the transpose of the pattern is outside the contract: the call still
 *     terminates, indexes nothing out of bounds and writes ids in [0, n).
 *   Checks before any HIP call (G4S_ERR_INVALID, g4s_last_error names the argument): any flag bit other than G4S_DEVICE_POINTERS, a NULL rowptr or
 *     labels, a NULL colids with n > 0, a negative n, one of trowptr / tcolids without the other, and with host pointers a labels array that overlaps
 *     an input. On the device, for both patterns and before any id is an index: rowptr[0] == 0, rowptr non-decreasing, ids in [0, n), and
 *     trowptr[n] == rowptr[n] — G4S_ERR_INVALID, outputs unspecified afterwards. n == 0 is valid and writes nothing; nnz == 0 is valid: labels[v] = v.
 *     info may be NULL.
 *   Algorithm (the Multistep shape of Slota, Rajamanickam, Madduri 2014). din[v] / dout[v] = the stored off-diagonal entries of v's row
 *     in Aᵀ / in A. (1) Trim to the fixpoint: every live vertex with din == 0 or dout == 0 is a component of its own; removing it walks its two rows
 *     with one atomic decrement per entry, and the lane that brings a counter to 0 claims that vertex: g4s_kcore's peel. (2) One pivot: the live
 *     vertex with the largest din·dout (64 bits; the smallest id at ties); forward reach over A, backward reach over Aᵀ inside the forward set; what
 *     the backward reach enters is the pivot's component and gets its smallest id; it is removed through the same peel. (3) Colouring rounds until
 *     nobody is live: colour[v] = v, atomicMin along live out-edges to the fixpoint; the vertices that kept their own id are roots, and from all of
 *     them at once a backward reach through vertices of the root's colour claims labels = colour — a root is the smallest id of everything that
 *     reaches it, hence of its component; removal and trimming as before. The smallest live id is always a root, so every round removes a component.
 *     The route is fixed, so components, largest, largest_label, trimmed, pivot, pivot_size and color_rounds are functions of the graph alone.
 *   Synchronous: runs on `stream` and returns when labels and info are complete. Which phase runs next is decided on the device; the host enqueues
 *     phase kernels blind in batches of at least G4S_SCC_BATCH launches (doubling to 64) with one read of the 208-byte state per batch, and a kernel
 *     whose phase it is not returns at once. Hence info.host_waits <= info.launches / 16 + 5: one wait per batch of the loop, one for the statistics,
 *     one for the copy to host arrays, three when the call builds the transpose — and no term in the number of steps, rounds or phases. The grid of
 *     the stepped kernels follows the frontier seen at the last read; a frontier that outgrows it stops the batch, which resumes on a larger grid
 *     (info.resumes). On a capturing stream the call returns G4S_ERR_INVALID and enqueues nothing. Scratch — a 256-byte state block, 28·n bytes
 *     (two counters, the queue, the colours, the stamps, two work queues), four lists of 4·min(n, 2^19) for long rows, the transpose when it is built,
 *     plus device copies of the arrays with host pointers — comes from the library's caching allocator and is released before the call returns. No
 *     process-wide state: different host threads may call at the same time.
 *   Environment: G4S_SCC_MIN_GRID (the smallest grid of a stepped kernel, default 8). The outputs do not depend on it.
 *   Where it loses (profiles/scc.txt, one MI355X, tools/bench_scc.py): with a given transpose it takes 51.8 ms on configs[1] as given (98.7 M edges) and
 *     8.3 ms on the directed R-MAT-20 against 2660 and 101 ms for scipy on the host with its copies (74.6 and 11.4 ms when it builds the transpose),
 *     and 1.8x / 1.5x the time of two g4s_bfs calls that find the giant component alone. It LOSES on long acyclic chains, which are trimmed one
 *     level per kernel: the 1000 × 1000 grid with every edge stored one way is 1999 dependent peels of at most 1000 vertices — 19.4 ms, 2.1x slower
 *     than scipy on the host (9.1 ms). From the algorithm alone, not measured at size: a chain of small components whose ids ascend downstream costs
 *     one colouring round per component, because each round's only root is the chain's first live component, and a long cycle costs one forward and
 *     one backward step per vertex. A host algorithm (Tarjan) is linear in all three. */
#define G4S_SCC_BATCH 16            /* phase launches enqueued behind one read of the state, at least (doubles up to 64 within a call) */
typedef struct g4s_scc_info {
    int64_t components;      /* number of distinct labels                                                       */
    int64_t largest;         /* vertices in the largest component                                                */
    int32_t largest_label;   /* its label (the smallest one among components of that size)                       */
    int32_t trimmed;         /* vertices labelled by trimming, over the whole call                               */
    int32_t pivot;           /* the pivot vertex; −1 when trimming left nobody                                   */
    int32_t pivot_size;      /* vertices in the pivot's component (0 without a pivot)                            */
    int32_t color_rounds;    /* colouring rounds run                                                             */
    int32_t reserved;
    int64_t edges_walked;    /* stored entries walked by peels, reaches and colour pushes                        */
    int32_t launches;        /* kernels enqueued, those that returned at once included                           */
    int32_t resumes;         /* batches restarted because the frontier outgrew the launch grid                   */
    int32_t host_waits;      /* times the call waited for the device                                             */
    int32_t built_transpose; /* 1: the call built the pattern of Aᵀ itself                                       */
} g4s_scc_info;              /* 64 bytes */
g4s_status g4s_strongly_connected_components(int32_t n, const int32_t *rowptr, const int32_t *colids,
                                             const int32_t *trowptr /* may be NULL */, const int32_t *tcolids /* may be NULL */,
                                             int32_t *labels, unsigned flags, g4s_scc_info *info /* may be NULL */, void *stream);

/* Minimum (or maximum) spanning forest: edges[0 … info.edges) (int32, device or host like the other arrays, only written) = the positions k in colids
 * of the forest's entries, ascending, for the undirected weighted graph on vertices 0 … n−1 in which every stored entry (i, j) with i != j of the n×n
 * CSR is an edge {i, j} of weight values[k], direction ignored — scipy.sparse.csgraph.minimum_spanning_tree and networkx's minimum_spanning_edges with
 * one fixed answer. Raw arrays, no handle, no plan.
 *   Graph: the rule of g4s_connected_components. Self-loops (never chosen), repeated columns, unsorted rows, empty rows, an upper triangle alone and a
 *     fully symmetric pattern are all valid; a symmetric pattern and its upper triangle give the same forest as sets of vertex pairs. values == NULL: all
 *     weights equal, which gives a spanning forest.
 *   Order: entries are ordered by the strict total order (w, min(i,j), max(i,j), k), w compared as a double; −0.0 equals +0.0 (canonicalised before the
 *     bit-ordered key), ±inf are ordinary weights, a NaN is found on the device and returns G4S_ERR_INVALID. The result is the forest Kruskal builds
 *     when it scans the entries in that order: unique, so the outputs are the same integers and the same weight bits on every run, stream, launch grid,
 *     batch size and tuning switch. G4S_MSF_MAXIMUM (no other entry point accepts it) orders by (−w, min, max, k): the maximum spanning forest; only
 *     the weight is reversed, ties still go to the smaller pair and position.
 *   Outputs: edges has room for max(n − 1, 0) values; info.edges of them are written, ascending, the rest is left untouched. labels (n int32, may be
 *     NULL) = the canonical component labels, the integers g4s_connected_components writes on the same pattern. info.weight = the sum of the forest's
 *     weights added in ascending position order in a shape fixed by info.edges alone (tiles of 2048, 8 consecutive values per lane, a shuffle ladder,
 *     four waves left to right; then the tile sums the same way): the same bits on every run; 0.0 with values == NULL. info may be NULL.
 *   Checks before any HIP call (G4S_ERR_INVALID, g4s_last_error names the argument): any flag bit other than G4S_DEVICE_POINTERS and G4S_MSF_MAXIMUM,
 *     a NULL rowptr with n > 0, a NULL edges with n > 1, a NULL colids with n > 0, a negative n, and edges or labels that overlap an input or each
 *     other (with device pointers, where rowptr[n] is not known yet, colids and values stand in with their first element). On the device, before any
 *     id is an index: rowptr[0] == 0, rowptr non-decreasing, ids in [0, n), no NaN — G4S_ERR_INVALID, outputs unspecified afterwards. n == 0 and
 *     nnz == 0 are valid (labels[v] = v, info.edges = 0). On a capturing stream the call returns G4S_ERR_INVALID and enqueues nothing.
 *   Algorithm: Borůvka rounds on the union-find forest of g4s_connected_components. A round walks the live rows (rows above 4096 entries
 *     by all workgroups) once per stage of the key — the 64-bit image of the weight, then (min << 32 | max) among the entries that have the winning
 *     weight, then k among those that have both; two stages with values == NULL —, each a 64-bit (32-bit) atomicMin per root behind a reduction across
 *     the wave where its lanes share the root; then one thread per root with a winner appends k to the forest (of two roots that chose the same entry
 *     the smaller one) and hooks the two trees by compare-and-swap, the smaller id winning; pointer jumping flattens the forest; rows that saw no
 *     outgoing entry leave the live list. rounds <= ceil(log2 n) + 1. Then the positions are sorted and the weights summed.
 *   Synchronous: runs on `stream` and returns when the outputs and info are complete. The host enqueues whole rounds (13 or 14 launches) blind, at least
 *     G4S_MSF_BATCH launches behind one read of the 120-byte state, doubling up to 64; every kernel returns at once when the stop word is set. Hence
 *     info.host_waits <= info.launches / 16 + 3: one wait per batch, one behind the sort and the sum, one for the copy to host arrays. The grid of the
 *     walks follows the live entries seen at the last read; live rows that outgrow the grid of the first batch stop it, and the next batch resumes on a
 *     larger grid (info.resumes) — the live rows only shrink afterwards, and by default the first grid is large enough, so only G4S_MSF_FIRST_GRID
 *     makes a resume happen. Scratch: a 256-byte state block, 36·n bytes (two 8-byte and one 4-byte key word per vertex, the stamps, two live lists, the
 *     forest list; 40·n with labels == NULL), two hub lists of 4·min(n, 2^19), nothing of the size of nnz, plus device copies of the arrays with host
 *     pointers; from the library's caching allocator, released before the call returns. No process-wide state: different host threads may call at the
 *     same time (tests/test_msf_threads_gpu.py).
 *   Environment: G4S_MSF_FIRST_GRID (workgroups of the first batch's walks; default 0 = automatic), G4S_MSF_WAVE_MIN (default 1; 0: every
 *     lane sends its own atomic). The outputs do not depend on them.
 *   Where it loses (profiles/msf.txt, one MI355X, tools/bench_msf.py, seeded symmetric integer weights): against scipy's minimum_spanning_tree on the
 *     host with its copy, on none of the measured graphs — the configs[0] grid (5.0 M entries) takes 5.58 ms in 10 rounds (8.6 M entries walked per
 *     round) against 297 ms, the symmetrised R-MAT-20 21.2 ms in 7 rounds against 2233 ms, configs[1] symmetrised (195.8 M entries) 147.0 ms in 6 rounds
 *     (scipy not measured at that size). The expected bad case, a path of 4 M vertices with increasing weights — one round whose hooks form a single
 *     chain of n − 1 — has the smallest margin: 6.0 ms against 75 ms, 12.5x; pointer jumping takes the chain 16 hops a pass. It loses to itself by 3x
 *     when weights are given (three walks of the live entries per round instead of two, and more rounds: values == NULL takes 1.86 / 6.5 / 48.5 ms on
 *     the three graphs), and every call pays 13 or 14 launches per round and at least two waits, which is all a tiny graph costs: a path of 1000
 *     vertices takes 0.23 ms against 0.66 ms for scipy, 2.8x, a floor of about 0.2 ms below which a host algorithm is ahead. Per-kernel times and the two switches as A/B timings were not measured. */
#define G4S_MSF_MAXIMUM 1048576u    /* the maximum spanning forest: the order is (−w, min, max, k) */
#define G4S_MSF_BATCH 16            /* launches enqueued behind one read of the state, at least (whole rounds; doubles up to 64 within a call) */
typedef struct g4s_msf_info {
    int64_t components;      /* number of distinct labels: n − edges                                             */
    int64_t edges;           /* positions written to `edges`                                                     */
    double weight;           /* the sum of their weights; 0.0 with values == NULL                                */
    int64_t entries_walked;  /* stored entries walked by the find stages, all rounds and stages                  */
    int32_t rounds;          /* Borůvka rounds run, the last one (which may find nothing) included               */
    int32_t launches;        /* kernels enqueued, those that returned at once included (the sort: 3 per pass)    */
    int32_t resumes;         /* batches restarted because the live rows outgrew the launch grid                  */
    int32_t host_waits;      /* times the call waited for the device                                             */
} g4s_msf_info;              /* 48 bytes */
g4s_status g4s_minimum_spanning_forest(int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values /* may be NULL */,
                                       int32_t *edges, int32_t *labels /* may be NULL */, unsigned flags,
                                       g4s_msf_info *info /* may be NULL */, void *stream);

/* Greedy colouring and independent sets: color[v] (n int32, device or host like the other arrays, only written) = the first-fit colour of v — the
 * smallest colour >= 0 not held by a neighbour of higher priority — i.e. sequential greedy colouring of the vertices in decreasing priority: what
 * networkx.greedy_color(G, strategy=<that order>) returns on the graph without self-loops. Raw arrays, no handle, no plan, no values.
 *   Pattern: exactly g4s_kcore's. The adjacency of a simple undirected graph, rows strictly ascending with ids in [0, n), rowptr non-decreasing from
 *     0: all of it checked on the device before any id is an index (G4S_ERR_INVALID, outputs unspecified afterwards). The caller declares the pattern
 *     symmetric; symmetry is not checked. On a pattern that is not, the call still terminates and gives every vertex a colour >= 0 and at most 64 +
 *     its row length, but the values are outside the contract. A stored diagonal entry is ignored: not counted, not walked.
 *   Priority: a strict total order, the pair (key[v], h(v)) compared lexicographically, larger first. key (n int32, may be NULL: all keys equal; any
 *     int32 is valid); h(v) = fmix32((uint32_t)v ^ seed) with the murmur3 finaliser x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35;
 *     x ^= x >> 16 — a bijection on 32 bits, so there are no ties. Distinct keys give any explicit order; key = the round of g4s_kcore gives
 *     smallest-last, which uses at most degeneracy + 1 colours; G4S_COLOR_LARGEST_FIRST (key must then be NULL) takes the degree without the diagonal,
 *     computed inside, as the key.
 *   round[v] (n int32, may be NULL): 0 when no neighbour has higher priority, else 1 + the largest round among those neighbours — the depth of v in
 *     the priority DAG and the step that coloured it; sorted by (round, id) the vertices are in a level schedule.
 *   Both outputs are functions of the pattern, the keys and the seed alone: the same on every run, stream, launch grid and tuning switch, compared
 *     with ==. {v : color[v] == 0} is a maximal independent set, the greedy one in priority order.
 *   info (may be NULL): colors = 1 + the largest colour, rounds = 1 + the largest round, class0 = the vertices coloured 0, overflow = the vertices whose
 *     higher-priority neighbours hold all of the colours 0 … 63 (a function of graph and order like the outputs), edges_walked = the stored
 *     off-diagonal entries (every row is walked once), and what the call did: launches, resumes, scan_resumes, host_waits.
 *   Checks before any HIP call (G4S_ERR_INVALID): any flag bit other than G4S_DEVICE_POINTERS and G4S_COLOR_LARGEST_FIRST, a NULL rowptr or color, a
 *     NULL colids with n > 0, a negative n, a non-NULL key together with G4S_COLOR_LARGEST_FIRST, and with host pointers outputs that overlap the
 *     inputs or each other. n == 0 is valid and writes nothing; nnz == 0 is valid: every colour is 0 and every round is 0.
 *   Algorithm: a Jones–Plassmann sweep. pred[v] = the higher-priority neighbours of v, by one walk over all rows; the vertices with
 *     pred == 0 are frontier 0. A step walks the frontier's rows balanced over entries (rows above 4096 entries in chunks of 1024 over all
 *     workgroups): v takes the lowest clear bit of its 64-bit mask, and for every lower-priority neighbour w sets that bit in w's mask and takes one
 *     off pred[w] — the lane that brings it to 0 appends w. Every vertex is queued once, so one array of n ints holds all frontiers. A vertex whose
 *     mask is full goes to an overflow list; a scan kernel behind the step marks the colours >= 64 of its higher-priority neighbours in an LDS bitmap
 *     of G4S_COLOR_WINDOW colours, window after window, and takes the first clear one. The scan joins the batches only once the list has an entry
 *     (info.scan_resumes = 1), so a graph below 65 colours never pays for it.
 *   Synchronous: runs on `stream` and returns when color, round and info are complete. Steps are enqueued blind in batches of at least G4S_COLOR_BATCH
 *     (doubling to 64) with one read of the 96-byte state per batch and one behind the opening pass: info.host_waits <= info.launches / 16 + 2 + info.resumes + info.scan_resumes. The
 *     grid follows the frontier seen at the last read; a frontier that outgrows it stops the batch, which resumes on a larger grid (info.resumes).
 *     On a capturing stream it returns G4S_ERR_INVALID and enqueues nothing. Scratch — a 256-byte state block, 8·n bytes of masks, 4·n each for pred,
 *     the queue and the overflow list (and the degrees under G4S_COLOR_LARGEST_FIRST), two lists of 4·min(n, 2^19) for long rows, plus device copies
 *     of the arrays with host pointers — comes from the library's caching allocator and is released before the call returns. No process-wide state:
 *     different host threads may call at the same time.
 *   Environment: G4S_COLOR_MIN_GRID (the smallest step grid, default 8). The outputs do not depend on it.
 *   Where it loses (profiles/color.txt, one MI355X): against the host loop of independent-set rounds over g4s_spmv_semiring max-plus — whose colouring
 *     is proper but spends one colour per round — it wins wherever the priority DAG is deep: 25.5 against 70.5 ms on the 1000 x 1000 grid under
 *     smallest-last (1262 rounds), 80 … 93 against 121 … 131 ms on the symmetrised R-MAT-20, 490 … 536 against 2073 … 2205 ms on configs[1]
 *     symmetrised. It loses 3x on that grid under a hash or largest-first order (2.56 against 0.85 ms): 14 rounds, where the loop is 14 products at
 *     the SpMV rate and the call pays its opening pass, two atomics per live entry and the largest grid for every step. It runs far below the walk's
 *     own rate everywhere (0.17 … 0.40 G entries/s on the R-MATs): one dependent kernel per level of the priority DAG, 20 us each on the grid, 80 us
 *     on the R-MATs. */
#define G4S_COLOR_LARGEST_FIRST 524288u  /* key := the degree without the diagonal, computed inside; `key` must be NULL */
#define G4S_COLOR_BATCH 16               /* step launches enqueued behind one read of the state, at least (doubles up to 64 within a call) */
#define G4S_COLOR_MASK_COLORS 64         /* the colours 0 … 63 travel as a pushed bitmask; above them a row scan decides */
#define G4S_COLOR_WINDOW 256             /* colours examined per pass of that row scan */
typedef struct g4s_color_info {
    int64_t edges_walked;    /* stored off-diagonal entries walked by the steps                        */
    int64_t class0;          /* vertices with colour 0: the size of the maximal independent set        */
    int32_t colors;          /* 1 + the largest colour written                                         */
    int32_t rounds;          /* non-empty frontiers coloured = 1 + the largest value written to `round` */
    int32_t overflow;        /* vertices whose higher-priority neighbours hold all of the colours 0 … 63 */
    int32_t launches;        /* kernels enqueued, those that returned at once included                 */
    int32_t resumes;         /* batches restarted because the frontier outgrew the launch grid         */
    int32_t scan_resumes;    /* batches restarted to bring the overflow scan in: 0 or 1                */
    int32_t host_waits;      /* times the call waited for the device                                   */
    int32_t reserved;
} g4s_color_info;            /* 48 bytes */
g4s_status g4s_color(int32_t n, const int32_t *rowptr, const int32_t *colids, const int32_t *key /* may be NULL */, uint32_t seed,
                     int32_t *color, int32_t *round /* may be NULL */, unsigned flags,
                     g4s_color_info *info /* may be NULL */, void *stream);

/* k-truss decomposition: truss[p] (one int32 per STORED ENTRY, device or host like the other arrays, only written) = the truss number of the edge
 * that entry p stores — the largest k such that the edge belongs to a subgraph in which every edge lies in at least k − 2 triangles of the subgraph;
 * the k-truss of the graph is the edges with truss >= k, what networkx.k_truss(G, k) keeps. Every edge has truss >= 2. Raw arrays, no handle, no
 * plan, no values.
 *   Pattern: exactly g4s_kcore's. The adjacency of a simple undirected graph, rows strictly ascending with ids in [0, n), rowptr non-decreasing from
 *     0: all of it checked on the device before any id is an index (G4S_ERR_INVALID, outputs unspecified afterwards). The caller declares the pattern
 *     symmetric; symmetry is not checked. On a pattern that is not, the call still terminates and indexes nothing out of bounds — an entry left of the
 *     diagonal without a mirror is treated like a diagonal entry — but the values are outside the contract. A stored diagonal entry is ignored and gets
 *     truss = 0, round = −1, support = 0. Both stored copies of an edge carry the same values.
 *   support[p] (nnz int32, may be NULL): the triangles through the edge in the INPUT graph — the values of C<A> = A·A on the pattern without its
 *     diagonal (g4s_spgemm_masked).
 *   round[p] (nnz int32, may be NULL): the graph is peeled level by level — j = the smallest remaining support, never decreasing — and inside a level
 *     frontier by frontier: a frontier is ALL remaining edges of support <= j, removed at once, each with truss = j + 2. A triangle all of whose edges
 *     were present before the removal and which holds at least one frontier edge dies ONCE: each of its edges outside the frontier loses exactly 1,
 *     whether one or two of its edges are in the frontier. The next frontier is the edges that this removal brought to <= j. round[p] is the 0-based
 *     index, over the whole call, of the non-empty frontier that removed the edge. That partition is a function of the graph alone, so truss, round
 *     and support are the same on every run, stream, pointer kind and launch grid and are compared with ==.
 *   max_k (>= 2): only the levels with truss < max_k are peeled. The edges still present afterwards — exactly the max_k-truss — get truss = max_k and
 *     round = −1, and info.capped = 1: truss == min(full truss, max_k). INT32_MAX asks for the full decomposition; max_k < 2 is G4S_ERR_INVALID.
 *   Checks before any HIP call (G4S_ERR_INVALID): any flag bit other than G4S_DEVICE_POINTERS, a NULL rowptr or truss, a NULL colids with n > 0, a
 *     negative n, max_k < 2, and with host pointers outputs that overlap the inputs or each other. n == 0 is valid and writes nothing; nnz == 0 is
 *     valid and writes nothing either. info may be NULL.
 *   Algorithm: every undirected edge gets a compact id — the rank of its entry right of the diagonal (one scan) — and every stored entry
 *     the id of its edge (the entry left of the diagonal finds its mirror by a binary search). An edge is walked along the SHORTER of its endpoints'
 *     rows, balanced over entries (rows above 4096 entries in chunks of 1024 over all workgroups); each entry is searched in the other row, a hit is a
 *     triangle. The support pass walks all edges once. A scan over the edges collects those with support <= j; when it collects none it raises j to the
 *     smallest remaining support, so a non-empty level costs at most two scans. A peel walks the frontier's edges: per triangle two plain loads of the
 *     other edges' rounds decide whether it is dead, and who decrements whom (of two frontier edges in one triangle the one with the smaller id); a
 *     decrement is one atomic, and the lane that brings an edge from j + 1 to j appends it. Every edge is queued once: one array holds all frontiers.
 *   Synchronous: runs on `stream` and returns when the outputs and info are complete. With device pointers the call waits once behind the row check
 *     (it sizes its scratch from rowptr[n]). Scans and peels are enqueued blind in batches of at least G4S_KTRUSS_BATCH launches (doubling to 64) with
 *     one read of the 128-byte state per batch: info.host_waits <= info.launches / 16 + 2. The peel grid follows the frontier seen at the last read; a
 *     frontier that outgrows it stops the batch, which resumes on a larger grid (info.resumes). On a capturing stream it returns G4S_ERR_INVALID and
 *     enqueues nothing. Scratch — a 256-byte state block, eight arrays of 4·nnz bytes (rank, edge of an entry, the two endpoints, support, round,
 *     truss, queue), two lists of 4·min(nnz, 2^19) for long rows, plus device copies of the arrays with host pointers — comes from the library's
 *     caching allocator and is released before the call returns. No process-wide state: different host threads may call at the same time. A graph
 *     with more than 2^19 edges BOTH of whose endpoints have rows above 4096 entries is refused (G4S_ERR_INVALID).
 *   Environment: G4S_KTRUSS_SCAN_WGS (the cap on the scan's workgroups, default one per CU), G4S_KTRUSS_MIN_GRID (the smallest peel grid,
 *     default 8). The outputs do not depend on them.
 *   Where it loses (profiles/ktruss.txt, one MI355X): against the host loop of INTEGRATION.md — supports by g4s_spgemm_masked on the remaining graph, a select,
 *     an intersect, repeated level by level to the same truss numbers — it wins on all three graphs measured (tools/bench_ktruss.py): 52.9 ms against
 *     1641 ms on the 1000 x 1000 grid with one diagonal per cell (1000 rounds), 122.9 against 3356 ms on the symmetrised R-MAT-16 (923 rounds), 330.6
 *     against 36 125 ms on the symmetrised R-MAT-18 (1267 rounds). It loses against itself: the support pass walks the 163 M entries of R-MAT-16 in
 *     3.3 ms, the peels walk the same entries once more in 104 ms, 2186 dependent kernels of 47 us on average, and the scans add 16 ms (two per level,
 *     each over all edges). On the grid a peel is 50 us for 18 000 entries: the call is bound by the number of dependent kernels, as g4s_kcore is. A
 *     graph of few rounds and one level is the case in which the loop comes closest; none was measured. */
#define G4S_KTRUSS_BATCH 16         /* step launches enqueued behind one read of the state, at least (doubles up to 64 within a call) */
typedef struct g4s_ktruss_info {
    int64_t triangles;       /* triangles of the input graph                                          */
    int64_t edges_walked;    /* stored entries walked by peel rounds (the shorter row of each edge)   */
    int64_t support_walked;  /* stored entries walked by the support pass                             */
    int64_t top_truss_edges; /* undirected edges whose truss equals `max_truss`                       */
    int32_t max_truss;       /* the largest truss written (max_k when capped; 0 without any edge)     */
    int32_t levels;          /* distinct truss values below max_k at which an edge was removed        */
    int32_t rounds;          /* non-empty frontiers peeled = 1 + the largest value written to `round` */
    int32_t scans;           /* passes over all edges that did work                                   */
    int32_t launches;        /* kernels enqueued, those that returned at once included                */
    int32_t resumes;         /* batches restarted because the frontier outgrew the launch grid        */
    int32_t host_waits;      /* times the call waited for the device                                  */
    int32_t capped;          /* 1: max_k ended the peeling with edges left                            */
} g4s_ktruss_info;           /* 64 bytes */
g4s_status g4s_ktruss(int32_t n, const int32_t *rowptr, const int32_t *colids, int32_t max_k,
                      int32_t *truss, int32_t *round /* may be NULL */, int32_t *support /* may be NULL */, unsigned flags,
                      g4s_ktruss_info *info /* may be NULL */, void *stream);

/* Sparse triangular solve, level-scheduled: T x = b for the lower (default) or upper (G4S_TRSV_UPPER) triangle T of an n × n CSR with
 * int32 indices and fp64 values — the kernel behind Gauss–Seidel and SSOR sweeps and IC(0) / ILU(0) preconditioners. An analysis that is paid once
 * (g4s_sptrsv_analyse: the levels of the dependency DAG, the schedule, the handle) and a solve that is paid per right-hand side (g4s_sptrsv_solve).
 *   Matrix: raw arrays on the host or the device (flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS), as g4s_kcore takes them. Only the entries of the
 *     chosen triangle are read (col <= row for lower, col >= row for upper); everything else is ignored, values included, so (D + L) and (D + U) of a
 *     general A are solved from A itself without a select. Columns inside a row need not ascend and may repeat: every stored off-diagonal entry
 *     contributes its own product, in stored order; repeated diagonal entries are summed from the left, d = (d0 + d1) + …. With
 *     G4S_TRSV_UNIT_DIAGONAL stored diagonal entries are ignored. Without it a row that stores no diagonal entry is G4S_ERR_INVALID, info.bad_row is
 *     the smallest such row and no handle is made. A stored zero, inf or NaN on the diagonal is no error: the division is IEEE.
 *   Checks: before any HIP call (G4S_ERR_INVALID) any flag bit other than G4S_DEVICE_POINTERS and the three G4S_TRSV_* bits, a NULL out or rowptr,
 *     NULL colids or values with n > 0, a negative n, and with host pointers a level that overlaps the inputs. On the device, before any id is an
 *     index: rowptr non-decreasing from 0 and ids in [0, n) (G4S_ERR_INVALID). After every refusal *out is untouched and level unspecified. n == 0 is
 *     valid: a handle with no level, whose solve does nothing.
 *   The handle keeps its own copy of the triangle, laid out by (level, row): the caller's arrays need not outlive the analysis.
 *     g4s_sptrsv_update_values takes new values in the layout of the arrays the handle was analysed from (all of them, rowptr[n] entries; host or
 *     device by its own flags) and refreshes the copy and the diagonal sums in one pass through a kept position map, on `stream`, asynchronous with
 *     device pointers; with host pointers it copies the array in and waits (not capturable). The pattern is fixed for the handle's life.
 *   level[i] (n int32, may be NULL, host or device like the inputs): 0 when row i has no off-diagonal entry in the triangle, else 1 + the largest
 *     level among the columns of those entries. Exact integers, the same on every run; info.levels = 1 + the largest. Rows are scheduled by
 *     (level, id).
 *   Arithmetic, fixed so that the bits can be pinned: x[i] = (b[i] − s_i) / d_i, with a unit diagonal x[i] = b[i] − s_i. s_i sums the products
 *     v·x[col] of row i's m off-diagonal triangle entries, in stored order, in a shape that depends on m alone — never on the level's width, the grid
 *     or the kernel. Products and sums round separately (no FMA).
 *       m <= G4S_TRSV_WAVE_ROW          s = +0.0; s = s + p_k for k = 0 … m − 1.
 *       G4S_TRSV_WAVE_ROW < m <= 4096   64 partial sums: a_l = +0.0, a_l = a_l + p_k for k = l, l + 64, …; then for o = 32, 16, … 1:
 *                                       a_l = a_l + a_(l+o) for l < o (the ladder of wave_reduce.hpp); s = a_0.
 *       m > 4096                        256 partial sums over k = t, t + 256, …; the ladder over each 64 consecutive ones gives w0 … w3;
 *                                       s = ((w0 + w1) + w2) + w3. One workgroup sums such a row, so it does not hold a level behind one wave.
 *     An x[i] that is a NaN is stored as the quiet NaN 0x7FF8000000000000: IEEE leaves the sign and the payload of a NaN result open (the device
 *     subtracts by adding the negated operand, which flips a NaN's sign), so the solve fixes them. ±0.0 and ±inf are what the operations give.
 *   Solve: b_dev and x_dev are device arrays of n doubles; x_dev may be b_dev (row i is the only reader of b[i] and the only writer of x[i]). It
 *     enqueues info.launches_per_solve kernels on `stream`, waits for nothing on the host and can be captured into a graph. No wave waits for a value
 *     another workgroup produces in the same kernel: dependencies between workgroups are kernel boundaries on the stream, nothing spins.
 *   Launches — the rule, restated by tests/trsv_ref.py: a level of at most G4S_TRSV_CHAIN_WIDTH rows is narrow. A maximal run of consecutive narrow
 *     levels is cut, from its first level on, into pieces of at most G4S_TRSV_CHAIN_LEVELS levels; every piece (one of a single level included) is a
 *     chain: ONE launch of ONE workgroup that steps through its levels behind a fence and a barrier, reading x with loads performed in L2. Every other
 *     level is one launch over its rows alone, 256 rows a workgroup and fewer where the level's rows are long. info.chains counts the chains, info.launches_per_solve = chains + the other
 *     levels. G4S_TRSV_NO_CHAINS (for tests) makes every level a launch of the second kind: chains = 0, launches_per_solve = levels, the same bits.
 *   The analysis is synchronous and not capturable (G4S_ERR_INVALID on a capturing stream, nothing enqueued). It is a Kahn peel of the DAG on the
 *     stepped driver of the graph calls — one step kernel per level, at least 16 (doubling to 64) behind one read of the state:
 *     info.host_waits <= info.launches / 16 + 5 (the counts, the seed, the level offsets, level to the host, and the last batch). A deep DAG pays one
 *     launch per level here too. Scratch is O(nnz_triangle + n + levels), released before it returns.
 *   Threads and streams: a solve only reads the handle, so solves on ONE handle may be enqueued on different streams and from different threads at
 *     the same time, given different x. g4s_sptrsv_update_values writes the handle: it must be ordered against every solve on it (same stream, or
 *     an event). Different handles are independent; analyses may run in different host threads at the same time (tests/test_trsv_threads_gpu.py).
 *   A block of k right-hand sides (g4s_sptrsv_solve_multi): T X = B for n × k blocks on the launches of ONE solve — exactly
 *     info.launches_per_solve kernels whatever k is, the same launch list, chaining rule and row spreading; a chain is one workgroup per tile of
 *     G4S_TRSV_RHS_TILE columns, and column tiles share nothing, so still no workgroup waits for another and nothing spins. Layout as g4s_spmm:
 *     element (i, j) at [i·ld + j] with ld >= k (row-major, the default) or, with G4S_TRSV_COL_MAJOR, at [i + j·ld] with ld >= n; the one flag
 *     covers both blocks; elements outside the n × k window are never written. X_dev may be B_dev with ldx == ldb ((i, j) is the only reader of
 *     B(i, j) and the only writer of X(i, j)); the same pointer with different leading dimensions is G4S_ERR_INVALID, any other overlap undefined.
 *     Column j of X holds, bit for bit, what g4s_sptrsv_solve gives for column j of B — the arithmetic above, per column —; columns never meet: a
 *     NaN or inf in one leaves every other column's bits alone. Refused before any HIP call (G4S_ERR_INVALID): a NULL handle, k < 0 or
 *     k > G4S_TRSV_MAX_RHS, a flag bit other than G4S_TRSV_COL_MAJOR, and with n > 0 and k > 0 a NULL B or X, an ld too small for its layout, and
 *     the aliasing case. k == 0 or n == 0 is valid and enqueues nothing. It waits for nothing on the host, allocates nothing, can be captured into
 *     a graph, and only reads the handle: the rule for threads and streams above is g4s_sptrsv_solve's.
 *   Out of scope: a transposed solve (transpose with g4s_csr_transpose and solve the other triangle),
 *     IC(0), ILU(k) (ILU(0) is g4s_ilu0 below), a preconditioner slot in g4s_conj_grad, several devices. */
#define G4S_TRSV_UPPER          2097152u /* solve with the upper triangle (default: lower) */
#define G4S_TRSV_UNIT_DIAGONAL  4194304u /* the diagonal is 1: stored diagonal entries are ignored, none is required */
#define G4S_TRSV_NO_CHAINS      8388608u /* tests: one launch per level */
#define G4S_TRSV_WAVE_ROW     32         /* a row of more off-diagonal triangle entries is summed by a wave */
#define G4S_TRSV_CHAIN_WIDTH  256        /* a level of at most this many rows is narrow */
#define G4S_TRSV_CHAIN_LEVELS 1024       /* levels per chain, at most */
#define G4S_TRSV_COL_MAJOR   (33554432u) /* g4s_sptrsv_solve_multi, g4s_ilu0_apply_multi: both blocks column-major, (i, j) at [i + j·ld]; default row-major: [i·ld + j] */
#define G4S_TRSV_RHS_TILE    (8)         /* columns of a block that one thread carries for its row */
#define G4S_TRSV_MAX_RHS     (32768)     /* k, at most */
typedef struct g4s_trsv_s *g4s_trsv_t;
typedef struct g4s_trsv_info {
    int64_t nnz_triangle;        /* entries kept: off-diagonal ones of the triangle and (without UNIT_DIAGONAL) diagonal ones */
    int32_t n;
    int32_t levels;              /* 1 + the largest level; 0 for n == 0                                   */
    int32_t widest_level;        /* rows of the widest level                                              */
    int32_t launches_per_solve;  /* kernels one g4s_sptrsv_solve enqueues                                 */
    int32_t chains;              /* of them chains                                                        */
    int32_t bad_row;             /* the smallest row without a stored diagonal entry, −1 when there is none */
    int32_t launches;            /* the analysis: kernels enqueued, those that returned at once included  */
    int32_t host_waits;          /* the analysis: times it waited for the device                          */
    int32_t resumes;             /* the analysis: batches restarted because the frontier outgrew the grid */
    int32_t reserved;
} g4s_trsv_info;                 /* 48 bytes */
g4s_status g4s_sptrsv_analyse(g4s_trsv_t *out, int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values,
                              int32_t *level /* n, may be NULL */, unsigned flags, g4s_trsv_info *info /* may be NULL */, void *stream);
g4s_status g4s_sptrsv_solve(g4s_trsv_t T, const double *b_dev, double *x_dev /* may be b_dev */, void *stream);
g4s_status g4s_sptrsv_solve_multi(g4s_trsv_t T, int32_t k, const double *B_dev, int64_t ldb, double *X_dev /* may be B_dev, ldx == ldb */, int64_t ldx,
                                  unsigned flags, void *stream);
g4s_status g4s_sptrsv_update_values(g4s_trsv_t T, const double *values, unsigned flags, void *stream);
g4s_status g4s_sptrsv_get_info(g4s_trsv_t T, g4s_trsv_info *info);
g4s_status g4s_sptrsv_destroy(g4s_trsv_t T);

/* ILU(0), level-scheduled: the incomplete factorisation A ≈ L U on the pattern of A itself, and its apply z = U⁻¹ (L⁻¹ r) — the
 * preconditioner g4s_sptrsv solves with. Factorise once per operator (g4s_ilu0_analyse), apply per Krylov iteration (g4s_ilu0_apply), refactorise when
 * the values change (g4s_ilu0_factor).
 *   Matrix: an n × n CSR with int32 ids and fp64 values, raw arrays on the host or the device (flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS). Unlike
 *     the solve, the factorisation needs canonical rows: columns strictly ascending inside a row, and every row stores its diagonal entry
 *     (host.csr_canonical, g4s::SortAndMerge give such rows).
 *   Checks: before any HIP call (G4S_ERR_INVALID) any flag bit other than G4S_DEVICE_POINTERS and G4S_ILU0_NO_CHAINS, a NULL out or rowptr, NULL
 *     colids or values with n > 0, a negative n, with host pointers a negative rowptr[n]. On the device, before any id is an index: rowptr
 *     non-decreasing from 0; then per row ids in [0, n), strictly ascending, the diagonal stored (G4S_ERR_INVALID). info.bad_row is the smallest row
 *     that offends in one of the three ways (the message names what that row does; −1 for a bad rowptr) and *out is untouched. n == 0 is valid.
 *   The handle keeps its own copy of the pattern and of the values it last factorised, the position of every diagonal entry, ONE array f of
 *     rowptr[n] factor values in the layout of the input arrays — L strictly below the diagonal (its unit diagonal implied), U on and above it —
 *     which g4s_ilu0_get_factors copies out (host or device by its flags; the host form waits), and two g4s_trsv_t plans analysed from
 *     (rowptr, colids, f) through g4s_sptrsv_analyse: the lower one with G4S_TRSV_UNIT_DIAGONAL, the other G4S_TRSV_UPPER. The caller's arrays need
 *     not outlive the analysis.
 *   Arithmetic, fixed so that every stored double can be pinned. Row i has the columns c_0 < … < c_(m−1) and working values w, initialised from A.
 *     For p = 0, 1, … while c_p = k < i, in that order: (1) w_p = w_p / u_kk, u_kk being row k's finished diagonal value; (2) for every entry (k, j)
 *     of row k with j > k whose column j row i stores at position t: w_t = w_t − (w_p · u_kj), product and difference rounded separately (no FMA).
 *     Updates for a j that row i does not store are dropped. Every w_t so receives its updates in ascending k whichever lane performs them: the
 *     bits depend neither on the grid nor on the row class nor on chaining. When a row finishes, every value of it that is a NaN is stored as
 *     0x7FF8000000000000 (the reason is the solve's: a − p is a + (−p) on the device); ±0.0 and ±inf are what the operations give.
 *   Pivots: a zero, inf or NaN pivot is no error. bad_pivot is the smallest row whose finished u_ii is zero or not finite, −1 when there is none:
 *     info.bad_pivot for the factorisation g4s_ilu0_analyse ends with; g4s_ilu0_factor writes it to the device word bad_pivot_dev (may be NULL; the
 *     word is set to −1 and lowered by the factor kernels with a vector atomicMin on the stream) and the caller reads it when they like.
 *   Launches: the dependency DAG of the row-wise factorisation is the DAG of the strictly lower triangle — row i waits for every k < i with a
 *     stored (i, k) — so the factorisation runs on the lower plan's (level, row) schedule under the rule of g4s_sptrsv: one launch per wide level,
 *     one workgroup per chain of narrow levels, behind every level of a chain a fence and a barrier, the values of rows finished earlier in the same
 *     kernel read with loads performed in L2. No wave waits for another workgroup, nothing spins. info.launches_per_factor equals the lower
 *     plan's launches_per_solve, info.chains its chains; info.launches_per_apply is the sum of the two plans' launches_per_solve.
 *     G4S_ILU0_NO_CHAINS (for tests) makes every level one launch, in the factorisation and in both solves: the same bits.
 *   Row classes, which never decide a bit: a row of at most G4S_ILU0_LANE_ROW stored entries is one lane's, w in registers; one of at most
 *     G4S_ILU0_WAVE_ROW is one wave's, w and its columns in LDS, the k loop sequential, the j loop over the lanes with a binary search in the row's
 *     columns; a longer one is one workgroup's, w in f itself, re-read with loads performed in L2 behind a fence and a barrier per k.
 *   Synchrony: g4s_ilu0_analyse is synchronous and not capturable (G4S_ERR_INVALID on a capturing stream, nothing enqueued); it ends with the first
 *     factorisation. info.launches / info.host_waits count the two inner analyses and its own work:
 *     host_waits <= launches / 16 + 13 (the two solve analyses' 5 each, the row check, the id check and the pivot word). g4s_ilu0_factor copies `values` in (rowptr[n] doubles in the layout of the analysed arrays, host or device by its flags; NULL:
 *     refactorise the values the handle holds), enqueues info.launches_per_factor factor kernels and refreshes both plans with
 *     g4s_sptrsv_update_values. With device pointers (and with NULL) it waits for nothing and can be captured; with host pointers it copies in and
 *     waits. g4s_ilu0_apply is two solves, L then U, with z as the intermediate (no scratch; z_dev may be r_dev); it never waits and can be captured.
 *     g4s_ilu0_apply_multi applies to an n × k block: g4s_sptrsv_solve_multi on the lower plan (R → Z), then on the upper plan (Z → Z) — its
 *     layout, flag (G4S_TRSV_COL_MAJOR), aliasing rule, refusals and bits (column j is g4s_ilu0_apply of column j), info.launches_per_apply kernels
 *     whatever k is, no scratch, nothing waited for, capturable; it only reads the handle, like g4s_ilu0_apply.
 *   Threads and streams: g4s_ilu0_apply only reads the handle, so applies on ONE handle may be enqueued on different streams and from different
 *     threads at the same time, given different z. g4s_ilu0_factor writes the handle: it must be ordered against every apply and every
 *     g4s_ilu0_get_factors on it (same stream, or an event). Different handles are independent; analyses may run in different host threads at the same
 *     time (tests/test_ilu_threads_gpu.py).
 *   Out of scope: IC(0), fill levels above 0, pivoting or a shift for a bad pivot, a preconditioner slot in g4s_conj_grad (host.pcg wires a
 *     preconditioned CG from g4s_spmv, this apply and torch), several devices. */
#define G4S_ILU0_NO_CHAINS 16777216u /* tests: one launch per level, in the factorisation and in both solves */
#define G4S_ILU0_LANE_ROW  8         /* a row of more stored entries is factorised by a wave */
#define G4S_ILU0_WAVE_ROW  512       /* a row of more stored entries is factorised by a workgroup */
typedef struct g4s_ilu0_s *g4s_ilu0_t;
typedef struct g4s_ilu0_info {
    int64_t nnz;                 /* stored entries: rowptr[n]                                                 */
    int32_t n;
    int32_t levels;              /* of the lower DAG; 0 for n == 0                                            */
    int32_t widest_level;        /* rows of its widest level                                                  */
    int32_t launches_per_factor; /* factor kernels one g4s_ilu0_factor enqueues                               */
    int32_t chains;              /* of them chains                                                            */
    int32_t launches_per_apply;  /* kernels one g4s_ilu0_apply enqueues                                       */
    int32_t bad_row;             /* the smallest row that is not canonical, −1 when there is none             */
    int32_t bad_pivot;           /* the smallest row whose u_ii is zero or not finite in the analysis's factorisation, −1: none */
    int32_t launches;            /* the analysis: kernels enqueued, the two inner analyses' included          */
    int32_t host_waits;          /* the analysis: times it waited for the device                              */
} g4s_ilu0_info;                 /* 48 bytes */
g4s_status g4s_ilu0_analyse(g4s_ilu0_t *out, int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags,
                            g4s_ilu0_info *info /* may be NULL */, void *stream);
g4s_status g4s_ilu0_factor(g4s_ilu0_t P, const double *values /* NULL: what is held */, unsigned flags, int32_t *bad_pivot_dev /* may be NULL */,
                           void *stream);
g4s_status g4s_ilu0_apply(g4s_ilu0_t P, const double *r_dev, double *z_dev /* may be r_dev */, void *stream);
g4s_status g4s_ilu0_apply_multi(g4s_ilu0_t P, int32_t k, const double *R_dev, int64_t ldr, double *Z_dev /* may be R_dev, ldz == ldr */, int64_t ldz,
                                unsigned flags, void *stream);
g4s_status g4s_ilu0_get_factors(g4s_ilu0_t P, double *values_out, unsigned flags, void *stream);
g4s_status g4s_ilu0_get_info(g4s_ilu0_t P, g4s_ilu0_info *info);
g4s_status g4s_ilu0_destroy(g4s_ilu0_t P);

/* Element-wise combination of two CSR matrices of the same shape, and filtering of one, on the device. Two calls each, on the model of
 * g4s_spgemm_symbolic / g4s_spgemm_numeric, with caller-allocated outputs: the symbolic call writes crpt (rows + 1) and *cnnz, the caller allocates
 * ccol (and cval) of *cnnz entries, the numeric call fills them. Nothing is kept between the two calls — no process-wide state, so different host
 * threads may call at the same time; the numeric call works the row split out again from the inputs and refuses a crpt whose last element is not
 * the entry count it arrives at itself.
 *   op: G4S_EWISE_UNION (every position stored in A or in B), G4S_EWISE_INTERSECT (stored in both), G4S_EWISE_DIFFERENCE (the entries of A whose
 *     position is not stored in B, with A's values). combine: G4S_COMBINE_PLUS, TIMES, MIN, MAX, FIRST (A's value), SECOND (B's), applied where
 *     both matrices store the position; under union an entry stored in only one matrix is copied bit for bit. op, combine and pred are plain ints,
 *     not flag bits.
 *   Input contract: the rows of A and B are strictly ascending with ids in [0, cols); rowptr is non-decreasing from 0. The symbolic call checks all
 *     of it on the device, the row pointers before any of them is used as an index; a violation returns G4S_ERR_INVALID and leaves the outputs
 *     unspecified (the mask rule of g4s_spgemm_masked). Column ids are only ever compared, never used as an index. Unsorted rows are sorted, and
 *     duplicates merged, by g4s_csr_row_indices followed by g4s_csr_from_coo_symbolic / _numeric (below; host.csr_canonical, g4s::SortAndMerge). A and B
 *     may be the very same arrays. The numeric call repeats the row-pointer check, not the one on the ids.
 *   Output: rows strictly ascending. A stored position is an entry whatever its value: explicit zeros are kept, and a sum that is 0.0 stays stored.
 *     Every value is one IEEE operation on two doubles or a copy, so the result is the same bits on every run. NaN and the sign of zero under
 *     MIN / MAX are outside the contract, as for the semirings (MIN is b < a ? b : a, MAX is a < b ? b : a).
 *   Pattern-only: aval == bval == cval == NULL writes ccol only. Any other mix of NULL value arrays is G4S_ERR_INVALID.
 *   Select keeps the entries that satisfy pred, in their stored order and with their bits (stable), so rows may be in any order, with repeats, and
 *     ids are not range-checked (they are never an index): G4S_SELECT_TRIL col − row <= k, TRIU col − row >= k (in 64 bits), OFFDIAG col != row,
 *     DIAG col == row, NONZERO val != 0, GT / GE / LT / LE val against thr with the plain C comparison — NaN fails all four and passes NONZERO.
 *     k and thr are ignored by the predicates that do not name them. A value predicate needs val (NULL: G4S_ERR_INVALID); a positional one accepts
 *     val == NULL. cval may be NULL (ccol only); cval without val is G4S_ERR_INVALID.
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays (cnnz and info are always host memory); any other bit returns G4S_ERR_INVALID.
 *     Checked before any HIP call (G4S_ERR_INVALID): flag bits, op / combine / pred, negative rows or cols, a NULL row pointer, crpt or cnnz, a
 *     NULL column array unless rows == 0, the NULL rules of the value arrays, and — with host pointers, where every length is known — an output
 *     that overlaps an input or another output. With device pointers the lengths of the column arrays are on the device: the symbolic call checks
 *     crpt against the row pointers before any HIP call and against the column arrays after its one wait (G4S_ERR_INVALID, the arrays involved
 *     unspecified); the numeric call reads the three counts first and checks before it enqueues anything.
 *   cnnz is summed in 64 bits; more than INT32_MAX entries return G4S_ERR_OVERFLOW from the symbolic call (crpt unspecified). rows, cols or an
 *     entry count of 0 are valid.
 *   Synchronous on `stream`: the symbolic calls wait for the device once (info.host_waits), the numeric ones twice with device pointers (the counts,
 *     the end) and once with host pointers. On a capturing stream all four return G4S_ERR_INVALID and enqueue nothing. Scratch — 12·rows bytes, in
 *     the numeric calls 8 more per unit, plus device copies of the arrays with host pointers — comes from the library's caching allocator and is
 *     released before return.
 *   Work units (info): every row's merged sequence of la + lb positions (select: its la entries) is cut into units of unit_entries = 64; 16 lanes
 *     take a unit, so short rows share a wave and a hub row spreads over the whole grid. Where it loses: rows much shorter than 64 positions leave
 *     most of a unit's lanes idle, and the numeric call reads the column ids twice (profiles/ewise.txt). */
#define G4S_EWISE_UNION       0
#define G4S_EWISE_INTERSECT   1
#define G4S_EWISE_DIFFERENCE  2
#define G4S_COMBINE_PLUS      0
#define G4S_COMBINE_TIMES     1
#define G4S_COMBINE_MIN       2
#define G4S_COMBINE_MAX       3
#define G4S_COMBINE_FIRST     4
#define G4S_COMBINE_SECOND    5
#define G4S_SELECT_TRIL       0
#define G4S_SELECT_TRIU       1
#define G4S_SELECT_OFFDIAG    2
#define G4S_SELECT_DIAG       3
#define G4S_SELECT_NONZERO    4
#define G4S_SELECT_GT         5
#define G4S_SELECT_GE         6
#define G4S_SELECT_LT         7
#define G4S_SELECT_LE         8
typedef struct g4s_ewise_info {
    int64_t nnz_a, nnz_b;    /* stored entries of A and of B                                                     */
    int64_t nnz_c;           /* entries of the result (what *cnnz receives)                                      */
    int64_t units;           /* work units: Σ over rows of ceil((la + lb) / unit_entries)                        */
    int32_t unit_entries;    /* merged positions per unit (a constant of the build)                              */
    int32_t rows_split;      /* rows cut into more than one unit                                                 */
    int32_t host_waits;      /* times the call waited for the device                                             */
    int32_t reserved;
} g4s_ewise_info;            /* 48 bytes */
g4s_status g4s_csr_ewise_symbolic(int op, int32_t rows, int32_t cols, const int32_t *arpt, const int32_t *acol, const int32_t *brpt,
                                  const int32_t *bcol, int32_t *crpt, int64_t *cnnz, unsigned flags, g4s_ewise_info *info, void *stream);
g4s_status g4s_csr_ewise_numeric(int op, int combine, int32_t rows, int32_t cols, const int32_t *arpt, const int32_t *acol, const double *aval,
                                 const int32_t *brpt, const int32_t *bcol, const double *bval, const int32_t *crpt, int32_t *ccol, double *cval,
                                 unsigned flags, void *stream);
g4s_status g4s_csr_select_symbolic(int pred, int64_t k, double thr, int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col,
                                   const double *val, int32_t *crpt, int64_t *cnnz, unsigned flags, void *stream);
g4s_status g4s_csr_select_numeric(int pred, int64_t k, double thr, int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col,
                                  const double *val, const int32_t *crpt, int32_t *ccol, double *cval, unsigned flags, void *stream);

/* ---- CSR from an edge list: (row, col[, val]) triples in any order, with repeats, to a CSR with ascending rows on the device — the role of the
 * reference's CSR(graph&) (mm/inc/CSR.h:255-329: each source's edges sorted, duplicates summed), of CSC::MergeDuplicates (mm/inc/CSC.h:297-342) and of
 * the sort in CSR::construct (mm/inc/CSR.h:640-668) — and its inverse, g4s_csr_row_indices. Two calls with caller-allocated outputs, the model of
 * g4s_csr_ewise_symbolic / _numeric: the symbolic call sorts and writes crpt, perm and *cnnz, the caller allocates ccol / cval of *cnnz entries, the
 * numeric call fills them. Nothing is kept inside the library between the calls (nothing process-wide: different host threads may call at the same
 * time).
 *   Order of the output: perm[p] is the input index of the p-th triple in (row, col, input index) order. The sort is stable, so perm is a function of
 *     the input alone: perm == lexsort((arange(nnz), col, row)), element for element.
 *   dup: G4S_DUP_KEEP — every triple stays an entry: *cnnz == nnz, ccol[p] = col[perm[p]], cval[p] = val[perm[p]] (rows ascending, repeats in input
 *     order). Otherwise a G4S_COMBINE_* value (PLUS, TIMES, MIN, MAX, FIRST: the earliest triple, SECOND: the latest): one entry per distinct
 *     position, rows strictly ascending, its value the combiner folded from left to right over the run in input order, acc = combine(acc, next).
 *     Every result is the same bits on every run. NaN and the sign of zero under MIN / MAX are outside the contract, as above. (The reference's
 *     constructor sorts a source's edges by (col, value) and so adds repeats in ascending value; the two agree bit for bit wherever the sums are
 *     exact, as for the integer weights of mm/inc/graph.h.)
 *   Bounds and sizes: ids must lie in [0, rows) × [0, cols); an id outside its range returns G4S_ERR_INVALID from the symbolic call and is never
 *     used as an index before it has been checked. nnz > INT32_MAX returns G4S_ERR_OVERFLOW before any HIP call. rows, cols or nnz of 0 are valid.
 *   Pattern-only: val == cval == NULL writes ccol only. Any other mix of NULL value arrays is G4S_ERR_INVALID.
 *   The numeric call trusts nothing in perm or crpt: a perm element outside [0, nnz), an id outside its range, a sequence whose keys decrease (or whose
 *     input indices do not increase inside a run of equal keys) and a crpt[rows] that is not the count the call arrives at itself return
 *     G4S_ERR_INVALID, and nothing is read or written out of bounds in any of these cases (ccol / cval hold crpt[rows] entries; they are unspecified
 *     after a refusal). It may be called again with new val on the same perm and crpt: the value refresh of a matrix whose pattern is fixed — what
 *     g4s_csr_update_values then takes.
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays (cnnz and info are always host memory); any other bit returns G4S_ERR_INVALID.
 *     Checked before any HIP call: flag bits and dup, negative sizes, the nnz limit, NULL crpt, perm or cnnz (numeric: crpt, perm), NULL row or col
 *     (numeric: or ccol) with nnz > 0, the NULL rule of the value arrays and — with host pointers — an output that overlaps an input or another output.
 *   Synchronous on `stream`. On a capturing stream all three calls return G4S_ERR_INVALID and enqueue nothing. The symbolic call waits for the device
 *     at most twice (the verdict on the ids and on the order; the counts), the numeric call once, with device and with host pointers alike (the
 *     copies back to host arrays are enqueued in front of the last wait); info.host_waits reports the count.
 *   Scratch comes from the library's caching allocator and is released before return: 20 bytes per triple in the symbolic call (two 64-bit keys and
 *     one payload partner; the head flags and their scan reuse the key partner) plus 2 KiB per tile for the digit tables, 16 bytes per triple in the
 *     numeric call, plus device copies of the arrays with host pointers.
 *   How (g4s_coo_info): the key row·2^col_bits + col over the significant bits of (rows − 1, cols − 1) only, sorted by a stable radix
 *     sort with digit_bits = 8 in sort_passes = ceil((row_bits + col_bits) / 8) passes, one workgroup per tile of tile_entries consecutive triples.
 *     An input already in (row, col) order skips the sort (presorted = 1, perm the identity). Where it loses: a run of L duplicates is folded by one
 *     lane in L sequential operations.
 * g4s_csr_row_indices writes the row of every stored entry — the array a CSR lacks to be a COO — with the row-pointer checks of g4s_csr_transpose
 * (zero-based, non-decreasing, ending at nnz: G4S_ERR_INVALID before anything is written) read back first. Two waits.
 * A CSR with unsorted rows or repeats becomes canonical — what g4s_csr_ewise_*, g4s_spgemm_masked and g4s_triangle_count ask for — by
 * g4s_csr_row_indices followed by the two calls here (host.csr_canonical, g4s::SortAndMerge). */
#define G4S_DUP_KEEP (-1)   /* every triple stays an entry (CSR::construct, CSR.h:640-668); otherwise a G4S_COMBINE_* */
typedef struct g4s_coo_info {
    int64_t nnz_in, nnz_out; /* triples given, entries of the result (what *cnnz receives)                       */
    int64_t longest_run;     /* the most triples on one position (1 without repeats, 0 for an empty list)        */
    int32_t row_bits;        /* significant bits of rows − 1                                                     */
    int32_t col_bits;        /* significant bits of cols − 1                                                     */
    int32_t digit_bits;      /* bits per radix pass (a constant of the build)                                    */
    int32_t sort_passes;     /* ceil((row_bits + col_bits) / digit_bits): what a sort costs, also when skipped   */
    int32_t tile_entries;    /* triples one workgroup ranks per pass (a constant of the build)                   */
    int32_t presorted;       /* 1: the input was in (row, col) order and no pass ran                             */
    int32_t host_waits;      /* times the call waited for the device                                             */
    int32_t reserved[3];
} g4s_coo_info;              /* 64 bytes */
g4s_status g4s_csr_from_coo_symbolic(int dup, int32_t rows, int32_t cols, int64_t nnz, const int32_t *row, const int32_t *col,
                                     int32_t *crpt /* rows+1 */, int32_t *perm /* nnz */, int64_t *cnnz, unsigned flags, g4s_coo_info *info /* may be NULL */,
                                     void *stream);
g4s_status g4s_csr_from_coo_numeric(int dup, int32_t rows, int32_t cols, int64_t nnz, const int32_t *row, const int32_t *col, const double *val,
                                    const int32_t *crpt, const int32_t *perm, int32_t *ccol, double *cval, unsigned flags, void *stream);
g4s_status g4s_csr_row_indices(int32_t rows, int64_t nnz, const int32_t *rowptr, int32_t *row_out /* nnz */, unsigned flags, void *stream);

/* ---- Extract: C = A[I, J], the ni × nj matrix with C(p, q) = A(I[p], J[q]) — GraphBLAS extract, MATLAB's A(I, J): induced subgraphs (A[S, S]),
 * relabellings (A[p, p]), leading and rectangular sub-matrices. The reference has the contiguous block as a constructor,
 * CSR(const CSR&, M_, N_, M_start, N_start) (mm/inc/CSR.h:691-733, used by mm/src/mkl_spgemm.cpp:50-57), and CSC::SpRef / SpRef2
 * (mm/inc/CSC.h:513-690), which want sorted lists and keep the original row ids; this call implements the MATLAB meaning SpRef's own comment
 * states. Two calls with caller-allocated outputs, the model of g4s_csr_ewise_* and g4s_csr_from_coo_*: the symbolic call writes crpt (ni + 1) and
 * *cnnz, the caller allocates ccol (cval, src) of *cnnz entries, the numeric call fills them. Nothing is kept inside the library between the calls
 * (nothing process-wide: different host threads may call at the same time).
 *   Result: C(p, q) is stored exactly where A(I[p], J[q]) is. I and J may be in any order and may repeat ids. I == NULL means every row in order
 *     and ni must equal rows; J == NULL means every column and nj must equal cols. An id outside [0, rows) or [0, cols) returns G4S_ERR_INVALID
 *     from the symbolic call and is never used as an index before it has been checked; the row pointers are checked the same way (zero-based,
 *     non-decreasing), as in g4s_csr_ewise_*, and so is every column id of A before it indexes the column map.
 *   Input rows: a row of A may be in any order and may repeat a column (each stored entry is extracted on its own).
 *   Output rows: ordered by (q, stored position of the source entry in A's row). The output is a function of the input alone and the same bits on
 *     every run. A canonical A (rows strictly ascending) gives strictly ascending output rows, also where J repeats ids.
 *   src (optional, *cnnz int32; NULL: not wanted): the index into col / val of the entry behind each output entry — cval[e] == val[src[e]] bit
 *     for bit and col[src[e]] == J[ccol[e]]. It is the perm of g4s_csr_from_coo_*: a caller refreshes the values of a fixed extraction, or carries a
 *     second per-edge attribute, with one gather.
 *   Pattern-only: val == cval == NULL writes ccol (and src) only. Any other mix of NULL value arrays is G4S_ERR_INVALID.
 *   flags: G4S_HOST_POINTERS / G4S_DEVICE_POINTERS for all arrays (cnnz and info are always host memory); any other bit returns G4S_ERR_INVALID.
 *     Checked before any HIP call (G4S_ERR_INVALID): flag bits, negative sizes, a NULL rpt, crpt or cnnz, a NULL col unless rows == 0 (numeric:
 *     a NULL ccol unless ni or nj is 0), ni != rows with I == NULL and nj != cols with J == NULL, the NULL rule of the value arrays and — with
 *     host pointers — an output that overlaps an input or another output. With device pointers the numeric call makes the overlap check after
 *     its first wait, when the lengths are known, and before it writes anything.
 *   Sizes: cnnz is summed in 64 bits; more than INT32_MAX entries return G4S_ERR_OVERFLOW from the symbolic call (crpt unspecified, *cnnz the
 *     exact count), and so do more than 2^31 work units. ni, nj, rows, cols or an entry count of 0 are valid.
 *   The numeric call trusts nothing: it works the counts out again from the inputs and refuses a crpt any of whose ni + 1 elements is not what
 *     it arrives at itself (G4S_ERR_INVALID, nothing written out of bounds, the outputs unspecified).
 *   Synchronous on `stream`; on a capturing stream both calls return G4S_ERR_INVALID and enqueue nothing. Every small device-to-host read goes
 *     through the pinned read ledger. Waits (info.host_waits): the symbolic call one. The numeric call two when the fill leaves every row in
 *     order (the sizes; the end) — always so for a canonical A with a non-decreasing or NULL J — three when rows are sorted, and where rows of
 *     more than lds_sort_max entries are sorted those of g4s_csr_from_coo_symbolic (at most two) and one more. Host pointers add none.
 *   Scratch comes from the library's caching allocator and is released before return: 12·ni + 8·cols bytes in the symbolic call; in the numeric
 *     call 20·ni + 8·cols, 8 per unit, 4·nj + 4·cols more for a J that decreases somewhere, 4·cnnz when src is NULL, and 16 bytes per entry of the
 *     rows that take the radix path plus the scratch of g4s_csr_from_coo_symbolic; device copies of the arrays with host pointers.
 *   How (g4s_extract_info): a unit is unit_entries = 64 stored entries of a source row, taken by 16 lanes, so short rows share a
 *     wave and a hub row spreads over the grid. mult[c] = #{q : J[q] == c} and its scan turn a column into its run of q's (j_kind 1: a range;
 *     j_kind 2: a list filled through cursors; j_kind 0: q = c, no map); a unit's count is Σ mult, a scan gives its first slot, the fill writes
 *     (q, src) runs. Rows the fill left non-decreasing in q are done (rows_in_order). The others are sorted by the distinct 64-bit keys
 *     (q << 32 | position): up to 64 entries in one wave (rows_sorted_wave), up to lds_sort_max in one workgroup's LDS (rows_sorted_lds), longer
 *     ones through the stable radix sort of g4s_csr_from_coo_symbolic (rows_sorted_radix). With j_kind 2 and ids repeated in J the order inside a
 *     column's list depends on arrival, so WHICH rows count as in order may differ between runs; the result does not.
 *   Where it loses: a J that names one column very many times makes one lane write that run sequentially; rows much shorter than 64 entries
 *     leave most of a unit's lanes idle; the numeric call reads the column ids twice and always writes src (into scratch when not asked for),
 *     the values following in a gather of their own; a relabelling of a graph with many rows over lds_sort_max entries pays the radix sort's
 *     passes over those rows. */
typedef struct g4s_extract_info {
    int64_t nnz_a;           /* stored entries of A                                                              */
    int64_t nnz_rows;        /* entries of A in the selected rows, Σ over p of the length of row I[p]            */
    int64_t nnz_c;           /* entries of the result (what *cnnz receives)                                      */
    int64_t units;           /* work units: Σ over p of ceil(length of row I[p] / unit_entries)                  */
    int32_t unit_entries;    /* stored entries per unit (a constant of the build)                                */
    int32_t j_kind;          /* 0: J == NULL (every column), 1: J never decreases, 2: otherwise                  */
    int32_t rows_in_order;   /* numeric: output rows the fill left in order (empty ones included): not sorted    */
    int32_t rows_sorted_wave;  /* numeric: rows of at most 64 entries sorted by one wave                         */
    int32_t rows_sorted_lds;   /* numeric: rows of at most lds_sort_max entries sorted in one workgroup's LDS    */
    int32_t rows_sorted_radix; /* numeric: longer rows, sorted by the radix sort of g4s_csr_from_coo_symbolic    */
    int32_t lds_sort_max;    /* the longest row the LDS class takes (a constant of the build)                    */
    int32_t host_waits;      /* times the call waited for the device                                             */
    int32_t reserved[4];
} g4s_extract_info;          /* 80 bytes */
g4s_status g4s_csr_extract_symbolic(int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, int32_t ni, const int32_t *I, int32_t nj,
                                    const int32_t *J, int32_t *crpt /* ni+1 */, int64_t *cnnz, unsigned flags, g4s_extract_info *info /* may be NULL */,
                                    void *stream);
g4s_status g4s_csr_extract_numeric(int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, const double *val, int32_t ni, const int32_t *I,
                                   int32_t nj, const int32_t *J, const int32_t *crpt, int32_t *ccol, double *cval, int32_t *src /* may be NULL */,
                                   unsigned flags, g4s_extract_info *info /* may be NULL */, void *stream);

/* ------------------------------------------------------------------ B3: graph gather/apply */

typedef void (*fun_gather)(int, int, const double **, const double *, double *); /* citcoms/lib/global_defs.h:48 */
typedef void (*fun_apply)(int, const double **, const double *, double *);       /* citcoms/lib/global_defs.h:49 */

/* Known gather/apply patterns the device can execute (host callbacks cannot run on the GPU).            */
#define G4S_PATTERN_ELEMENT_BLOCK_MATVEC   1 /* CitcomS e_assemble_del2_u gather, Element_calculations.c:453-471 */
#define G4S_PATTERN_DENSE_ROW_TIMES_MATRIX 2 /* DeePMD OptMatmul gather, opt_matmul.cc:52-58                     */
#define G4S_PATTERN_SYM_QUADRATIC_FORM     3 /* Cantera gather1/apply1, gather2/apply2, RedlichKwongMFTP.cpp:927-970 */

typedef struct g4s_pattern_desc {
    int32_t kind;
    /* ELEMENT_BLOCK_MATVEC: result[eq(e,a,i)] += Σ_b Σ_d K_e[(dof·a+i)·(npe·dof) + dof·b+d] · u[eq(e,b,d)],
     * eq(e,a,i) = id[ ien[e·npe + a]·dof + i ]   (0-based restatement of IEN/ID, Element_calculations.c:460-468). */
    int32_t num_elems;        /* nel: number of elements (= numNodes of the spmm_dense calls that follow)                */
    int32_t nodes_per_elem;   /* 8  (enodes[3])                                                          */
    int32_t dof;              /* 3  (mesh.nsd)                                                           */
    const int32_t *ien;       /* [numNodes · nodes_per_elem] element → node, 0-based, host memory         */
    const int32_t *id;        /* [nno · dof] node,dof → equation, 0-based, host memory                    */
    int32_t nno;              /* number of nodes                                                         */
    int32_t neq;              /* number of equations (length of vertexStates / result)                   */
    int32_t edge_weight_base; /* 1 if edgeWeight[0] is unused and element e lives at edgeWeight[e+1] (CitcomS, Drive_solvers.c:52-55), else 0 */
    int32_t static_weights;   /* 1: the element matrices behind an edgeWeight pointer do not change between calls (true inside one
                                 CitcomS CG solve); they are uploaded once per distinct edgeWeight pointer. Re-register to invalidate. */
    /* DENSE_ROW_TIMES_MATRIX: result[e·degree + a] = Σ_k edgeWeight[e][k] · states[k·degree + a]        */
    int32_t inner;            /* N (opt_matmul.cc:33, global Nsize)                                      */
    /* SYM_QUADRATIC_FORM: see RedlichKwongMFTP.cpp:927-970                                              */
    int32_t numbers;          /* coefficient stride (1 = gather1/apply1 form, >1 = gather2/apply2 form)   */
} g4s_pattern_desc;

/* Register a (gather, apply) pair as an instance of a known pattern; later spmm_dense calls with that
 * pair run on the device. desc (and the ien/id arrays) are copied. */
g4s_status g4s_register_pattern(fun_gather gather, fun_apply apply, const g4s_pattern_desc *desc);
g4s_status g4s_unregister_pattern(fun_gather gather, fun_apply apply);

/* What an UNREGISTERED (gather, apply) pair gets. Callbacks are host code the device cannot execute, and the interface
 * promises every pair "gather degree times per vertex, then apply" (deepmd/source/op/graph.h:21-32), so by default the
 * reference's driver loop runs on the host, one thread, vertices in ascending order (the reference itself hard-codes
 * 8 OpenMP threads, graph.h:23, racing on gathers that scatter — e.g. CitcomS' Au[aa] +=, Element_calculations.c:466).
 *   SERIAL    (default) one host thread;
 *   PARALLEL  the caller declares its gathers race-free: threadNum threads, vertices handed out one at a time
 *             (schedule(dynamic,1), graph.h:24);
 *   REFUSE    G4S_ERR_UNSUPPORTED (spmm_dense: abort) — for deployments that must never fall off the device. */
#define G4S_HOST_CALLBACKS_SERIAL   0
#define G4S_HOST_CALLBACKS_PARALLEL 1
#define G4S_HOST_CALLBACKS_REFUSE   2
g4s_status g4s_set_host_callback_policy(int32_t policy);
/* The same for the calling thread only (-1: back to the process-wide policy); *previous (may be NULL) receives what was set before, so that scopes nest
 * (g4s::ScopedRaceFree, include/g4s/graph.hpp: a call site declares ITS gathers race-free without changing what other threads' callbacks get). */
g4s_status g4s_set_host_callback_policy_thread(int32_t policy, int32_t *previous);

/* The reference symbol, exactly (citcoms/lib/global_defs.h:854-857; bound at citcoms/bin/Citcom.c:93).
 * Registered pairs run as HIP kernels; any other pair runs the reference's host loop (policy above). spmm_dense returns
 * void as the reference's does, so a failure aborts with a message — g4s_spmm_dense is the status-returning form. */
void spmm_dense(uint32_t numNodes, uint32_t degree, const double **edgeWeight, const double *vertexStates,
                double *temp, double *result, fun_gather gather, fun_apply apply, double *time, int threadNum);
g4s_status g4s_spmm_dense(uint32_t numNodes, uint32_t degree, const double **edgeWeight, const double *vertexStates,
                          double *temp, double *result, fun_gather gather, fun_apply apply, double *time, int threadNum);

/* Device-resident forms of the three patterns (what spmm_dense dispatches to; solvers call these directly
 * to keep vectors on the device between iterations). */
typedef struct g4s_elem_op_s *g4s_elem_op_t;
typedef struct g4s_node_op_s *g4s_node_op_t;
typedef struct g4s_cg_ws_s *g4s_cg_ws_t;
/* elt_k_dev: numElems × (npe·dof)² doubles, contiguous, device memory (borrowed). ien/id host arrays as in the descriptor. */
g4s_status g4s_elem_op_create(g4s_elem_op_t *out, int32_t numElems, int32_t nodes_per_elem, int32_t dof,
                              const int32_t *ien_host, const int32_t *id_host, int32_t nno, int32_t neq,
                              const double *elt_k_dev);
g4s_status g4s_elem_op_destroy(g4s_elem_op_t op);
/* Au_dev[0..neq) = Σ_e scatter(K_e · gather(u_dev))  — overwrites Au (the caller's zeroing at
 * Element_calculations.c:495-496 is folded in). Deterministic (no atomics). */
g4s_status g4s_elem_op_apply(g4s_elem_op_t op, const double *u_dev, double *Au_dev, void *stream);

/* BI_dev[eq] = 1 / Σ_e K_e[p·n+p] over the (element, local dof p) pairs that map to eq — build_diagonal_of_K
 * (citcoms/lib/Element_calculations.c:580-611) followed by the inversion at Construct_arrays.c:469. Equations with a zero
 * diagonal get 0 (the reference asserts instead). */
g4s_status g4s_elem_op_inverse_diagonal(g4s_elem_op_t op, double *BI_dev, void *stream);

/* Device-resident Jacobi-preconditioned conjugate gradient with the update order of conj_grad
 * (citcoms/lib/General_matrix_functions.c:307-424): d0 = 0, r = F; loop while (residual > acc && count < *cycles) || count == 0;
 * the mat-vec is g4s_elem_op_apply followed by zeroing the boundary rows (assemble_del2_u(..., strip_bcs = 1), the list of
 * citcoms/lib/BC_util.c:89-102). All vectors stay in HBM and the loop test runs on the device: the host enqueues iterations in batches and
 * reads 40 bytes of state per batch.
 * *cycles: in = iteration cap (vlowstep), out = iterations done. zero_resid_dev may be NULL when n_zero == 0.
 * Exactly one of op / A selects the operator (element-by-element or assembled CSR). */
g4s_status g4s_conj_grad(g4s_elem_op_t op, g4s_csr_t A, int32_t neq, const double *BI_dev, const int32_t *zero_resid_dev, int32_t n_zero,
                         const double *F_dev, double *d0_dev, double acc, int32_t *cycles, double *residual, void *stream);

/* ---- CitcomS's node-assembled stiffness operator (the other mat-vec format of assemble_del2_u) — SURVEY.md §8 f1.
 * node_map[nno·max_eqn] = E->Node_map[lev][m] (slot group 0: the node's own three equations, groups 1..13: lower-numbered
 * neighbours, unused slots = neq; citcoms/lib/Construct_arrays.c:254-328), eqn_k1..3[nno·max_eqn] = E->Eqn_k1..3[lev][m]
 * (construct_node_ks :335-470), id[nno·3] = E->ID .doff[1..3]; all host pointers, 0-based nodes, copied. The stored symmetric half
 * is expanded once into per-node 3×3 neighbour blocks so that the mat-vec is a gather. */
g4s_status g4s_node_op_create(g4s_node_op_t *out, int32_t nno, int32_t neq, int32_t max_eqn, const int32_t *node_map,
                              const int32_t *id, const double *eqn_k1, const double *eqn_k2, const double *eqn_k3);
g4s_status g4s_node_op_destroy(g4s_node_op_t op);
/* Au = K·u, then the listed rows zeroed (strip_bcs) — n_assemble_del2_u, citcoms/lib/Element_calculations.c:516-577.
 * u_dev / Au_dev hold neq doubles (the reference's dummy entry [neq] is not needed: unused slots are dropped at create). */
g4s_status g4s_node_op_apply(g4s_node_op_t op, const double *u_dev, double *Au_dev, const int32_t *zero_resid_dev, int32_t n_zero,
                             void *stream);
/* g4s_conj_grad (below) on the node-assembled operator. */
g4s_status g4s_conj_grad_node(g4s_node_op_t op, int32_t neq, const double *BI_dev, const int32_t *zero_resid_dev, int32_t n_zero,
                              const double *F_dev, double *d0_dev, double acc, int32_t *cycles, double *residual, void *stream);

/* ---- The incompressibility (Uzawa) iteration of CitcomS around the velocity solve — SURVEY.md §8 f1.
 * g_dev[e·npe·dof + p] = elt_del[e].g[p][0], the per-element divergence / gradient vector; pressure unknowns are elements. */

/* divU[e] = Σ_a (g[3a]·U[eq1] + g[3a+1]·U[eq2] + g[3a+2]·U[eq3]) — assemble_div_u, citcoms/lib/Element_calculations.c:701-729. */
g4s_status g4s_elem_op_div_u(g4s_elem_op_t op, const double *g_dev, const double *U_dev, double *divU_dev, void *stream);
/* gradP = Σ_e g·P[e] scattered to the equations (here: gathered per node, no atomics), then the boundary rows zeroed —
 * assemble_grad_p, Element_calculations.c:737-779 (strip_bcs_from_residual, BC_util.c:89-102). */
g4s_status g4s_elem_op_grad_p(g4s_elem_op_t op, const double *g_dev, const double *P_dev, double *gradP_dev,
                              const int32_t *zero_resid_dev, int32_t n_zero, void *stream);
/* BPI[e] = 1 / Σ_p g[e][p]·BI[eq(e,p)]·g[e][p] (1 where that is 0) — build_diagonal_of_Ahat / assemble_dAhatp_entry,
 * Element_calculations.c:613-644, 785-830. */
g4s_status g4s_elem_op_pressure_preconditioner(g4s_elem_op_t op, const double *g_dev, const double *BI_dev, double *BPI_dev, void *stream);

typedef struct g4s_stokes_params {
    double imp;                            /* accuracy of the outer iteration (control.accuracy) */
    double inner_accuracy_scale;           /* control.inner_accuracy_scale */
    double v_res;                          /* monitor.fdotf: the inner solves run to imp·inner_accuracy_scale·v_res */
    int32_t v_steps_low;                   /* iteration cap of one velocity solve (control.v_steps_low) */
    int32_t steps_max;                     /* cap of the outer iteration */
    int32_t check_continuity_convergence;  /* keep_iterating: || instead of && (Stokes_flow_Incomp.c:150-162) */
    int32_t check_pressure_convergence;    /* "converging" also needs dpressure < imp */
} g4s_stokes_params;

typedef struct g4s_stokes_result {
    int32_t outer_iterations;              /* *steps_max on return */
    int32_t last_solve_valid;              /* the last velocity solve reached its accuracy */
    int64_t inner_iterations;              /* CG iterations of all velocity solves */
    double incompressibility, v_norm, p_norm, dvelocity, dpressure;   /* the quantities of print_convergence_progress */
} g4s_stokes_result;

/* solve_Ahat_p_fhat_CG, citcoms/lib/Stokes_flow_Incomp.c:188-452, incompressible case (initial_vel_residual :839-881 included),
 * velocity solves by g4s_conj_grad (solve_del2_u's CG branch, General_matrix_functions.c:89-94) on the element-by-element
 * operator of `op`, or — K_csr != NULL — on the assembled stiffness matrix through g4s_spmv (BASELINE config 5: "assembled stiffness
 * matrix driving G4S SpMV inside the CG/Uzawa solver loop"; op then only supplies the mesh maps of div/grad; the boundary rows are
 * zeroed after every product either way, so K_csr is the plain assembly of the element matrices).
 * V_dev[neq] and P_dev[nel] are updated in place; F_dev is not modified. nmass_dev[nno] = NMass, area_dev[nel] = eco[].area,
 * volume = mesh.volume (the weights of global_v_norm2 / global_p_norm2 / global_div_norm2, Global_operations.c:591-656).
 * hist (host, may be NULL): 5 doubles per printed line — v_norm, p_norm, dvelocity, dpressure, incompressibility — line 0 before
 * the loop, at most hist_lines lines. Every vector stays on the device; a few scalars per outer iteration cross PCIe. */
g4s_status g4s_stokes_uzawa_cg(g4s_elem_op_t op, g4s_csr_t K_csr, const double *g_dev, const double *BI_dev, const double *BPI_dev, const double *nmass_dev,
                               const double *area_dev, double volume, const int32_t *zero_resid_dev, int32_t n_zero, const double *F_dev,
                               double *V_dev, double *P_dev, const g4s_stokes_params *params, g4s_stokes_result *result,
                               double *hist, int32_t hist_lines, void *stream);

/* ---- g4s_conj_grad with the loop opened up, for a row-partitioned operator on several GPUs (1-D row partition,
 * all-gather / halo exchange of the direction vector, all-reduce of the dot products). Every rank holds its slab of F, BI, d0; the
 * caller owns the mat-vec (exchange p, local g4s_spmv into Ap) and, between the steps, all-reduces (sum) the partial sums
 * element-wise: partials[0..256) = r·z, [256..512) = p·Ap, [512..768) = r·r. Sequence:
 *   g4s_cg_begin → all-reduce [512..768) and [0..256) → g4s_cg_direction → g4s_cg_state (done?) → g4s_cg_buffers: p → Ap = A·p →
 *   g4s_cg_reduce_pAp → all-reduce [256..512) → g4s_cg_update → all-reduce [512..768), [0..256) → g4s_cg_direction → … → g4s_cg_end.
 * With one rank and no all-reduce this is g4s_conj_grad step by step. zero_resid indices are local to the slab. */
g4s_status g4s_cg_ws_create(g4s_cg_ws_t *out, int32_t n_local);
g4s_status g4s_cg_ws_destroy(g4s_cg_ws_t ws);
g4s_status g4s_cg_begin(g4s_cg_ws_t ws, const double *F_dev, const double *BI_dev, double *d0_dev, const int32_t *zero_resid_dev, int32_t n_zero,
                        void *stream);
g4s_status g4s_cg_direction(g4s_cg_ws_t ws, int32_t steps, double acc, void *stream);   /* loop test + β + p (conj_grad :364-379) */
g4s_status g4s_cg_state(g4s_cg_ws_t ws, int32_t *count, int32_t *done, double *residual, void *stream);   /* synchronises */
g4s_status g4s_cg_buffers(g4s_cg_ws_t ws, double **p_dev, double **Ap_dev, double **partials_dev);        /* valid until the next g4s_cg_update */
g4s_status g4s_cg_reduce_pAp(g4s_cg_ws_t ws, void *stream);                              /* boundary rows of Ap := 0, partial p·Ap */
g4s_status g4s_cg_update(g4s_cg_ws_t ws, const double *BI_dev, double *d0_dev, void *stream);   /* α, d0, r, z (:383-402) */
g4s_status g4s_cg_end(g4s_cg_ws_t ws, double *d0_dev, const int32_t *zero_resid_dev, int32_t n_zero, void *stream);   /* d0 boundary rows := 0 (:409) */

/* The same loop closed in C for a row-partitioned operator: conj_grad (General_matrix_functions.c:307-424) with the product
 * g4s_spmv_dist_apply(A) and the dot products' partial sums all-reduced by g4s_comm_allreduce_sum_f64(comm) — the neighbour exchange of
 * Regional_parallel_related.c:744-789 and the MPI_Allreduce of Global_operations.c:534-562 on RCCL. Every rank calls it with its slab
 * (n_local rows; BI, F, d0 device arrays of that length; zero_resid: LOCAL indices of the boundary equations) and gets the same cycles
 * and residual. A must be connected to comm (g4s_spmv_dist_connect_rccl). */
g4s_status g4s_conj_grad_dist(g4s_spmv_dist_t A, void *comm, int32_t n_local, const double *BI_dev, const int32_t *zero_resid_dev, int32_t n_zero,
                              const double *F_dev, double *d0_dev, double acc, int32_t steps, int32_t *cycles, double *residual, void *stream);

/* The two collectives a partitioned Krylov solver needs, as a pair of callbacks, so that ONE loop in C serves RCCL and any transport the
 * host already has (MPI in CitcomS; gloo in the tests): the sum all-reduce of the dot products (Global_operations.c:534-562) and the
 * exchange of the x entries of one distributed product (Regional_parallel_related.c:744-789).
 *   allreduce_sum_f64(ctx, buf_dev, count, stream): element-wise sum over the ranks, in place, device buffer, ordered on `stream`.
 *   exchange(ctx, h, stream): called between g4s_spmv_dist_begin(h) and g4s_spmv_dist_finish(h): carry h's send buffer to the peers and fill
 *   its receive buffer (g4s_spmv_dist_buffers). NULL: the handle's own RCCL wiring does it (g4s_spmv_dist_apply).
 * g4s_transport_rccl fills the pair for an RCCL communicator the handles are connected to. */
typedef struct g4s_transport {
    void *ctx;
    g4s_status (*allreduce_sum_f64)(void *ctx, double *buf_dev, int64_t count, void *stream);
    g4s_status (*exchange)(void *ctx, g4s_spmv_dist_t h, void *stream);
} g4s_transport;
g4s_status g4s_transport_rccl(void *comm, g4s_transport *out);
/* g4s_conj_grad_dist over a transport. */
g4s_status g4s_conj_grad_dist_tr(g4s_spmv_dist_t A, const g4s_transport *tr, int32_t n_local, const double *BI_dev, const int32_t *zero_resid_dev,
                                 int32_t n_zero, const double *F_dev, double *d0_dev, double acc, int32_t steps, int32_t *cycles, double *residual,
                                 void *stream);

/* The Uzawa / Schur-complement CG iteration of g4s_stokes_uzawa_cg on a PARTITIONED operator (BASELINE configs[4] "1 vs 8 GPUs";
 * solve_Ahat_p_fhat_CG, citcoms/lib/Stokes_flow_Incomp.c:188-452, with the reductions of Global_operations.c:591-656 over the ranks).
 * The velocity unknowns (equations) and the pressure unknowns (elements) each have a 1-D partition; every rank holds its slabs of all
 * vectors and three distributed operators over those partitions:
 *   K   equations × equations   the assembled stiffness matrix (square; the inner solves are g4s_conj_grad_dist_tr on it);
 *   D   elements × equations    assemble_div_u:  divU[e] = Σ_p g[e][p]·U[eq(e,p)]      (Element_calculations.c:744-779), as a CSR matrix;
 *   Dt  equations × elements    assemble_grad_p: its transpose                           (:701-741)            (g4s_spmv_dist_create_rect).
 * On one rank the element-ordered sums of g4s_stokes_uzawa_cg become CSR row sums: same terms, same order within a part, the own-column
 * and remote-column parts added separately — results agree to rounding, iteration counts normally exactly.
 * vmass_dev[neq_local] = NMass of the node that owns the equation (the weight of global_v_norm2), area_dev[nel_local], volume = mesh volume,
 * zero_resid: LOCAL equation indices; BI / BPI: the two preconditioner diagonals, local slabs. V / P updated in place.
 * The host waits once per outer iteration: a velocity solve's first batch of iterations is enqueued with what follows it, and the rest of the iteration is
 * enqueued again if that batch turns out not to have met the solve's test (all ranks read the same all-reduced sums and take the same turn);
 * G4S_STOKES_SYNC=1 waits for every solve instead. */
g4s_status g4s_stokes_uzawa_cg_dist(g4s_spmv_dist_t K, g4s_spmv_dist_t D, g4s_spmv_dist_t Dt, const g4s_transport *tr, int32_t neq_local, int32_t nel_local,
                                    const double *BI_dev, const double *BPI_dev, const double *vmass_dev, const double *area_dev, double volume,
                                    const int32_t *zero_resid_dev, int32_t n_zero, const double *F_dev, double *V_dev, double *P_dev,
                                    const g4s_stokes_params *params, g4s_stokes_result *result, double *hist, int32_t hist_lines, void *stream);

/* result[M×K] = xx[M×N] · w[N×K], row-major fp64, device pointers (opt_matmul.cc:24-62). */
g4s_status g4s_dense_rows_times_matrix(int32_t M, int32_t N, int32_t K, const double *xx_dev, const double *w_dev,
                                       double *result_dev, void *stream);

/* Gradient of the op above — _opt_matmul_grad (deepmd/source/op/_opt_matmul_grad.py:6-12):
 *   dxx[M×N] = grad[M×K] · wᵀ      (tf.matmul(grad, w, False, True))
 *   dw[N×K]  = xxᵀ · grad[M×K]     (tf.matmul(xx, grad, True, False))
 * Row-major fp64 device pointers. dxx_dev or dw_dev may be NULL to skip that product. dw is reduced over the M rows in a fixed
 * slab order (no atomics): the same inputs give the same bits. */
g4s_status g4s_dense_rows_times_matrix_grad(int32_t M, int32_t N, int32_t K, const double *xx_dev, const double *w_dev,
                                            const double *grad_dev, double *dxx_dev, double *dw_dev, void *stream);

/* ---- The reference's dense comparison drivers: what it times next to the sparse kernels, not the hot path.
 * Column-major dim×dim fp64, alpha = 1, beta = 0, as the reference calls MKL. Host pointers, or device pointers with
 * G4S_DEVICE_POINTERS; synchronous.
 *   g4s_dense_mm — mm/src/cblas_dxxmm.c:57-111:  DGEMM  C = A·B          (cblas_dgemm ColMajor NoTrans NoTrans, :96-111)
 *                                                DSYMM  C = sym(A)·B     (cblas_dsymm Left Upper: only A's upper triangle is read, :57-76)
 *                                                DTRMM  B := B·triu(A)   (cblas_dtrmm Right Upper NoTrans NonUnit, in place; C unused, :78-95)
 *   g4s_dense_mv — mv/mv.c:6-27:                 DGEMV  y = A·x (:23-27)   DSYMV  y = sym(A)·x (Upper, :6-10)
 *                                                DTRMV  x := triu(A)ᵀ·x (Upper Trans NonUnit, in place; y unused, :12-15)
 *                                                DSPMV  y = sym(AP)·x, AP the packed upper triangle, dim(dim+1)/2 doubles (:17-21)
 * Level 3 runs on the fp64 MFMA GEMM of g4s_dense_rows_times_matrix; level 2 is one HBM pass over the matrix. */
#define G4S_DENSE_DGEMM 1
#define G4S_DENSE_DSYMM 2
#define G4S_DENSE_DTRMM 3
#define G4S_DENSE_DGEMV 4
#define G4S_DENSE_DSYMV 5
#define G4S_DENSE_DTRMV 6
#define G4S_DENSE_DSPMV 7
g4s_status g4s_dense_mm(int32_t kind, int32_t dim, const double *A, double *B, double *C, unsigned flags);
g4s_status g4s_dense_mv(int32_t kind, int32_t dim, const double *A, double *x, double *y, unsigned flags);

/* result[0] += Σ_i Σ_{j<i} x_i x_j (a[num·(i+m·j)] + a[num·(j+m·i)]) + Σ_i x_i² a[num·(i+m·i)];
 * numbers == 1: result[1] += Σ_i x_i·b_i (apply1); numbers > 1: result[1] likewise on a[…+1] (gather2/apply2).
 * Host pointers (the operands are ~100×100); result is a host double[2] that is accumulated into. */
g4s_status g4s_sym_quadratic_form(int32_t m, int32_t numbers, const double *a, const double *x, const double *b,
                                  double *result);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* G4S_H */
