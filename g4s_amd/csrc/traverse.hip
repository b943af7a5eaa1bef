// traverse.hip — g4s_sssp and g4s_bfs (include/g4s.h): single-source / multi-source shortest paths and BFS levels on a CSR handle stored by
// out-edges, with a per-step choice between a push from the frontier and the dense pull d := d ⊕ (Aᵀ ⊗ d).
//
// State lives on the device (traverse.hpp, TravState): two frontier queues, the length and out-edge count of the current one, the step counter
// and a `stop` word. Every step is ONE kernel; the workgroup that finishes last (a ticket counter, no waiting) swaps the queues, counts the
// step and sets `stop`: 1 frontier empty, 2 iteration cap, 3 the next step wants to pull, 4 the frontier outgrew the launch grid. A kernel
// that finds stop != 0 returns at once, so the host enqueues kBatch (doubling to kBatchMax) push launches blind and reads the 80-byte state once per batch, as
// g4s_conj_grad does. Kernel boundaries are the only ordering between workgroups; nothing spins and every loop is bounded by
// the queue length (<= rows) or a row length.
//
//   push    the frontier walk of frontier.hpp over the queue: rows at most kHubCut long from the front, hubs from the BACK of the same array.
//           SSSP: cand = d[u] + w; plain load of d[v]; global_atomic_min_f64 only when cand < d[v]; the vertex is
//           appended when the atomic returned a larger value and its step stamp (atomicMax on mark[v]) shows it is not queued yet.
//           BFS: compare-and-swap of level[v] from −1. Appends are one atomicAdd per wave.
//   pull    SSSP: y := Aᵀ ⊗ d by the inner handle's semiring kernels (any path), then sssp_combine_kernel: d := min(d, y), the changed vertices
//           are the next queue. BFS: bfs_pull_kernel over the arrays of Aᵀ, LPR lanes per unvisited vertex, stopping at the first in-edge
//           whose tail has level == step (the level array IS the frontier set; a vertex is written by its own group only).
// Where it loses (profiles/traverse.txt): a traversal of a few dense steps — configs[1] from its hub, 8 steps — is faster as the host loop over
// g4s_spmv_semiring_transpose (3.8 ms against 8.4 for SSSP, 4.0 against 14.0 for BFS): every changed vertex goes through append()'s one tail counter,
// which holds a step to about 7 G edges/s, in push and pull alike. It wins where steps are many and frontiers small (1000 x 1000 grid: 1.4x / 3.7x).
// min is order-independent and IEEE addition is monotone, so every schedule ends at the same bits (g4s.h has the argument).
#include "common.hpp"
#include "csr_handle.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "traverse.hpp"
#include <algorithm>
#include <climits>
#include <new>
#include <vector>

namespace {

using g4s::TravState;

constexpr int kBatch = G4S_TRAVERSE_BATCH;   // push launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)

enum { KIND_INIT = 0, KIND_PUSH = 1, KIND_PULL = 2 };

struct StepArgs {
    long long nnz;
    long long threshold;   // a frontier with more out-edges wants a pull (auto); −1: always pull; LLONG_MAX: never
    long long grid_cap;    // push only: more out-edges than this ask for a larger grid
    int max_iter;
    int resume;            // push only: the first launch of a batch goes on from stop == 4
};

// A vertex for the next queue: at most kHubCut out-edges to the front (one atomicAdd per wave), more to the hub end. Called by every lane that is
// active at the call site.
__device__ __forceinline__ void append(bool want, int v, int deg, int rows, int *__restrict__ q, TravState *st, long long &deg_sum)
{
    const bool hub = want && deg > kHubCut;
    const int idx = wave_append(want && !hub, &st->n_next);
    if ((unsigned)idx < (unsigned)rows) q[idx] = v;                // a vertex is appended once per step: idx < rows by construction
    if (hub) {
        const int h = atomicAdd(&st->n_hub_next, 1);
        if ((unsigned)h < (unsigned)rows) q[rows - 1 - h] = v;
    }
    if (want) deg_sum += deg;
}

// The end of a step kernel: the block's share of the next frontier's out-edges, then the ticket; the last block to arrive turns the page (turn_page).
__device__ __forceinline__ void finish(TravState *st, long long deg_sum, int kind, const StepArgs a)
{
    __shared__ long long s_red[WG / 64];
    deg_sum = wave_sum(deg_sum);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = deg_sum;
    if (!turn_page(&st->tickets, [&] {
        long long sum = 0;
        for (int w = 0; w < (int)blockDim.x / 64; ++w) sum += s_red[w];
        if (sum) atomicAdd((unsigned long long *)&st->edges_next, (unsigned long long)sum);
    })) return;
    const int n = atomicAdd(&st->n_next, 0), nh = atomicAdd(&st->n_hub_next, 0);
    const long long e = (long long)atomicAdd((unsigned long long *)&st->edges_next, 0ull);
    if (kind == KIND_PUSH) { st->edges_relaxed += st->edges_cur; st->push_steps += 1; st->iter += 1; }
    if (kind == KIND_PULL) { st->edges_relaxed += a.nnz; st->pull_steps += 1; st->iter += 1; }
    st->n_cur = n; st->n_hub_cur = nh; st->edges_cur = e;
    st->n_next = 0; st->n_hub_next = 0; st->edges_next = 0;
    st->cur ^= 1;
    st->tickets = 0;
    st->stop = (n + nh == 0) ? 1 : (st->iter >= a.max_iter ? 2 : (e > a.threshold ? 3 : (e > a.grid_cap ? 4 : 0)));
}

template <bool BFS>
__global__ __launch_bounds__(WG) void init_fill_kernel(int rows, double *__restrict__ dist, int *__restrict__ level, int *__restrict__ mark)
{
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < rows; i += (long long)gridDim.x * WG) {
        if constexpr (BFS) level[i] = -1;
        else { dist[i] = __builtin_inf(); mark[i] = 0; }
    }
}

// One workgroup: the state from zero, the (distinct) sources at 0 and in queue 0. `src` is queue 1, where the host staged them.
template <bool BFS>
__global__ __launch_bounds__(WG) void init_sources_kernel(int rows, int n_src, const int *__restrict__ src, const int *__restrict__ rowptr, double *__restrict__ dist,
                                                          int *__restrict__ level, int *__restrict__ q0, TravState *st, const StepArgs a)
{
    if (threadIdx.x == 0) {
        const int zero_values = st->zero_values;
        *st = TravState{};
        st->zero_values = zero_values;
        st->cur = 1;                                               // finish() flips it: queue 0 is the first frontier
    }
    __syncthreads();
    long long deg_sum = 0;
    for (int i0 = 0; i0 < n_src; i0 += WG) {
        const int i = i0 + (int)threadIdx.x;
        const bool valid = i < n_src;
        int v = 0, deg = 0;
        if (valid) {
            v = src[i];
            deg = rowptr[v + 1] - rowptr[v];
            if constexpr (BFS) level[v] = 0;
            else dist[v] = 0.0;
        }
        append(valid, v, deg, rows, q0, st, deg_sum);
    }
    finish(st, deg_sum, KIND_INIT, a);
}

// One relaxation of the edge u → v (entry k); true when v has to join the next frontier.
template <bool BFS, bool VALUES>
__device__ __forceinline__ bool relax(int k, int v, double du, int stamp, const double *__restrict__ values, double *dist, int *level, int *mark)
{
    if constexpr (BFS) {
        if constexpr (VALUES) {
            if (!(values[k] != 0.0)) return false;                 // or-and: a stored 0.0 is no edge (NaN counts as one)
        }
        if (level[v] != -1) return false;
        return atomicCAS(level + v, -1, stamp) == -1;
    } else {
        const double cand = du + values[k];
        if (!(cand < dist[v])) return false;                       // a stale read is only ever too large: the atomic below decides
        const double old = __hip_atomic_fetch_min(dist + v, cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(cand < old)) return false;
        return atomicMax(mark + v, stamp) < stamp;                 // first improvement of v in this step
    }
}

template <bool BFS, bool VALUES>
__global__ __launch_bounds__(WG) void push_kernel(int rows, const int *__restrict__ rowptr, const int *__restrict__ colids, const double *__restrict__ values,
                                                  double *dist, int *level, int *mark, int *q0, int *q1, TravState *st, const StepArgs a)
{
    if (!step_runs(st->stop, a.resume)) return;
    const int cur = st->cur, stamp = st->iter + 1;
    const int *q = cur ? q1 : q0;
    int *qn = cur ? q0 : q1;
    long long deg_sum = 0;
    auto vertex = [&](int u, int &start, int &deg, double &du) {
        start = rowptr[u];
        deg = rowptr[u + 1] - start;
        if constexpr (!BFS) du = dist[u];                          // BFS carries nothing: its payload is never read and takes no LDS
    };
    auto entry = [&](bool valid, int k, double du) {
        bool want = false;
        int v = 0, vdeg = 0;
        if (valid) {
            v = colids[k];
            want = relax<BFS, VALUES>(k, v, du, stamp, values, dist, level, mark);
            if (want) vdeg = rowptr[v + 1] - rowptr[v];
        }
        append(want, v, vdeg, rows, qn, st, deg_sum);
    };
    walk_tiles<double>(st->n_cur, [&](int i, int &start, int &deg, double &du) { vertex(q[i], start, deg, du); }, entry);
    walk_hubs<double>(st->n_hub_cur, [&](int h, int &start, int &deg, double &du) { vertex(q[rows - 1 - h], start, deg, du); }, entry);
    finish(st, deg_sum, KIND_PUSH, a);
}

// The second half of an SSSP pull step: y = Aᵀ ⊗ d has been computed; d := min(d, y), and the vertices that changed are the next frontier.
__global__ __launch_bounds__(WG) void sssp_combine_kernel(int rows, const int *__restrict__ rowptr, double *__restrict__ dist, const double *__restrict__ y, int *q0, int *q1,
                                                          TravState *st, const StepArgs a)
{
    int *qn = st->cur ? q0 : q1;
    long long deg_sum = 0;
    for (long long i0 = (long long)blockIdx.x * WG; i0 < rows; i0 += (long long)gridDim.x * WG) {
        const long long i = i0 + threadIdx.x;
        bool want = false;
        int deg = 0;
        if (i < rows) {
            const double yv = y[i];
            if (yv < dist[i]) {
                dist[i] = yv;
                want = true;
                deg = rowptr[i + 1] - rowptr[i];
            }
        }
        append(want, (int)i, deg, rows, qn, st, deg_sum);
    }
    finish(st, deg_sum, KIND_PULL, a);
}

// Bottom-up BFS step on Aᵀ (row v: the tails u of the edges u → v): LPR lanes per unvisited vertex, done at the first tail in the frontier.
template <int LPR, bool VALUES>
__global__ __launch_bounds__(WG) void bfs_pull_kernel(int rows, const int *__restrict__ rowptr, const int *__restrict__ trowptr, const int *__restrict__ tcolids,
                                                      const double *__restrict__ tvalues, int *level, int *q0, int *q1, TravState *st, const StepArgs a)
{
    constexpr int GPB = WG / LPR;
    int *qn = st->cur ? q0 : q1;
    const int depth = st->iter, stamp = depth + 1;
    const int t = (int)threadIdx.x, lig = t % LPR, lane = t & 63;
    const unsigned long long gmask = LPR == 64 ? ~0ull : (((1ull << (LPR % 64)) - 1ull) << (lane - lig));
    long long deg_sum = 0;
    for (long long r0 = (long long)blockIdx.x * GPB; r0 < rows; r0 += (long long)gridDim.x * GPB) {
        const long long v = r0 + t / LPR;
        bool found = false;
        if (v < rows && level[v] == -1) {
            const int end = trowptr[v + 1];
            for (int k0 = trowptr[v]; k0 < end; k0 += LPR) {       // the same trip count for the lanes of a group
                const int k = k0 + lig;
                bool hit = false;
                if (k < end) {
                    hit = level[tcolids[k]] == depth;
                    if constexpr (VALUES) hit = hit && (tvalues[k] != 0.0);
                }
                if constexpr (LPR > 1) hit = (__ballot(hit) & gmask) != 0ull;
                if (hit) { found = true; break; }
            }
        }
        const bool want = found && lig == 0;
        int deg = 0;
        if (want) {
            level[v] = stamp;                                      // written by v's own group only; readers compare with `depth`, never with stamp
            deg = rowptr[v + 1] - rowptr[v];
        }
        append(want, (int)v, deg, rows, qn, st, deg_sum);
    }
    finish(st, deg_sum, KIND_PULL, a);
}

// reached := vertices with a finite distance / a level >= 0, once the traversal has ended (stop 1 or 2); a no-op before.
template <bool BFS>
__global__ __launch_bounds__(WG) void count_kernel(int rows, const double *__restrict__ dist, const int *__restrict__ level, TravState *st)
{
    __shared__ int s_red[WG / 64];
    if (st->stop != 1 && st->stop != 2) return;
    int c = 0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < rows; i += (long long)gridDim.x * WG) c += BFS ? (level[i] >= 0) : (dist[i] < __builtin_inf());
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_red[w];
        if (sum) atomicAdd((unsigned long long *)&st->reached, (unsigned long long)sum);
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------ the handle's workspace
namespace g4s {

struct TraverseWork {
    int32_t *queue[2] = {nullptr, nullptr};   // rows ints each: frontier vertices from the front, hubs from the back
    int32_t *mark = nullptr;                  // rows ints: the step in which a vertex last joined a queue (SSSP)
    double *dist2 = nullptr;                  // rows doubles: y of the pull step
    TravState *state = nullptr;
    ZeroScan zeros;                           // is a stored value 0.0? BFS then has to read the values
    DevicePieces mem;                         // owns the arrays above
};

void traverse_work_destroy(TraverseWork *w) { delete w; }
long long traverse_work_bytes(const TraverseWork *w) { return w ? w->mem.bytes : 0; }
void traverse_values_changed(TraverseWork *w) { if (w) w->zeros.changed(); }

} // namespace g4s

namespace {

constexpr unsigned kDirFlags = G4S_TRAVERSE_PUSH | G4S_TRAVERSE_PULL;
constexpr unsigned kAllFlags = kDirFlags | G4S_TRAVERSE_SYMMETRIC;

// Does any stored value equal 0.0? One pass and one read, at reserve and after g4s_csr_update_values. Synchronises `s`.
int scan_values(g4s_csr_s *A, hipStream_t s, int *waits)
{
    g4s::TraverseWork *w = A->trv;
    return w->zeros.scan(A->nnz, A->d_values, w->mem.cus, &w->state->zero_values, s, waits);
}

// The workspace (once) and, unless the flags rule a pull out or declare A symmetric, the handle's transpose. NULL stream, synchronous.
int reserve(g4s_csr_s *A, unsigned flags)
{
    if (!A->trv) {
        std::unique_ptr<g4s::TraverseWork> w(new (std::nothrow) g4s::TraverseWork());
        if (!w) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
        const size_t n = (size_t)std::max(A->rows, 1);
        w->mem.take(&w->queue[0], sizeof(int32_t) * n);
        w->mem.take(&w->queue[1], sizeof(int32_t) * n);
        w->mem.take(&w->mark, sizeof(int32_t) * n);
        w->mem.take(&w->dist2, sizeof(double) * n);
        w->mem.take(&w->state, sizeof(TravState));
        if (w->mem.ok()) w->mem.note(hipMemset(w->state, 0, sizeof(TravState)));
        if (!w->mem.ok()) return w->mem.report("g4s_csr_traverse_reserve");
        A->trv = w.release();
    }
    G4S_TRY(scan_values(A, nullptr, nullptr));
    if (!(flags & (G4S_TRAVERSE_SYMMETRIC | G4S_TRAVERSE_PUSH)) && !A->tr) G4S_TRY(g4s_csr_transpose_reserve(A));
    return G4S_OK;
}

// push while the frontier has at most nnz / alpha out-edges. Defaults from the sweep in profiles/traverse.txt: SSSP 8 (configs[1]: 8.4 ms
// against 8.9 at 16, 8.5 at 4, 16.1 at 2); BFS 1, i.e. never pull — on configs[1] the bottom-up step loses to the push at every switch point measured
// (14.0 ms at 1, 16.5 at 2, 24.5 at 4..64). The grid of configs[0] never reaches either threshold.
double switch_alpha(bool bfs)
{
    if (const char *e = getenv("G4S_TRAVERSE_ALPHA")) {
        const double a = atof(e);
        if (a > 0.0) return a;
    }
    return bfs ? 1.0 : 8.0;
}

template <bool BFS>
int traverse(g4s_csr_s *A, const int32_t *sources, int32_t n_sources, double *dist, int32_t *level, int32_t cap, unsigned flags, g4s_traverse_info *info, hipStream_t s)
{
    const char *fn = BFS ? "g4s_bfs" : "g4s_sssp";
    if (A->rows != A->cols) return g4s::set_error(G4S_ERR_INVALID, "%s: the handle is %d x %d, a traversal needs a square matrix", fn, A->rows, A->cols);
    std::vector<int32_t> src(sources, sources + n_sources);
    for (int32_t v : src)
        if (v < 0 || v >= A->rows) return g4s::set_error(G4S_ERR_INVALID, "%s: source %d is outside [0, %d)", fn, v, A->rows);
    std::sort(src.begin(), src.end());
    src.erase(std::unique(src.begin(), src.end()), src.end());
    G4S_TRY(not_capturing(fn, s, "its state"));

    const bool symmetric = (flags & G4S_TRAVERSE_SYMMETRIC) != 0;
    const int mode = (flags & G4S_TRAVERSE_PUSH) ? KIND_PUSH : (flags & G4S_TRAVERSE_PULL) ? KIND_PULL : 0;
    if (!A->trv || (mode != KIND_PUSH && !symmetric && !A->tr)) G4S_TRY(reserve(A, flags));
    g4s::TraverseWork *w = A->trv;
    int waits = 0;
    if (BFS) G4S_TRY(scan_values(A, s, &waits));
    const bool values = w->zeros.state == 2;

    // the pull side: Aᵀ (its inner handle and arrays), or A itself when the caller declares it symmetric
    g4s_csr_t pull_handle = A;
    const int32_t *trowptr = A->d_rowptr, *tcolids = A->d_colids;
    const double *tvalues = A->d_values;
    if (mode != KIND_PUSH && !symmetric) g4s::transpose_work_view(A->tr, &trowptr, &tcolids, &tvalues, &pull_handle);

    const int rows = A->rows;
    StepArgs a;
    a.nnz = A->nnz;
    a.max_iter = cap > 0 ? cap : (BFS ? INT_MAX : rows);
    a.threshold = mode == KIND_PUSH ? LLONG_MAX : mode == KIND_PULL ? -1 : (long long)((double)A->nnz / switch_alpha(BFS));
    a.grid_cap = LLONG_MAX;
    a.resume = 0;
    const g4s::StepGrid sized(g4s::kMinGrid, 2 * w->mem.cus);  // the push grid of a batch: between 8 workgroups and two per CU
    TravState *st = w->state;
    int *q0 = w->queue[0], *q1 = w->queue[1];

    G4S_HIP_TRY(hipMemcpyAsync(q1, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(init_fill_kernel<BFS>, dim3(grid_rows(rows, w->mem.cus)), dim3(WG), 0, s, rows, dist, level, w->mark);
    hipLaunchKernelGGL(init_sources_kernel<BFS>, dim3(1), dim3(WG), 0, s, rows, (int)src.size(), q1, A->d_rowptr, dist, level, q0, st, a);
    G4S_HIP_TRY(hipGetLastError());

    g4s::ReadScope reads(s);
    TravState h{};
    h.stop = mode == KIND_PULL ? 3 : 0;                            // what the init kernel is bound to decide when the direction is forced
    bool know = false;                                             // h is the device's state
    int batch = kBatch;
    for (;;) {
        if (h.stop == 3) {                                         // one pull step
            if constexpr (BFS) {
                const long long avg = rows ? A->nnz / rows : 0;
                const int g = grid_rows((long long)rows * (avg <= 4 ? 4 : avg <= 16 ? 16 : 64), w->mem.cus);
#define TV_PULL(LPR) do { if (values) hipLaunchKernelGGL((bfs_pull_kernel<LPR, true>), dim3(g), dim3(WG), 0, s, rows, A->d_rowptr, trowptr, tcolids, tvalues, level, q0, q1, st, a); \
                          else hipLaunchKernelGGL((bfs_pull_kernel<LPR, false>), dim3(g), dim3(WG), 0, s, rows, A->d_rowptr, trowptr, tcolids, tvalues, level, q0, q1, st, a); } while (0)
                if (avg <= 4) TV_PULL(4);
                else if (avg <= 16) TV_PULL(16);
                else TV_PULL(64);
#undef TV_PULL
            } else {
                G4S_TRY(g4s_spmv_semiring(pull_handle, dist, w->dist2, G4S_SEMIRING_MIN_PLUS, s));
                hipLaunchKernelGGL(sssp_combine_kernel, dim3(grid_rows(rows, w->mem.cus)), dim3(WG), 0, s, rows, A->d_rowptr, dist, w->dist2, q0, q1, st, a);
            }
            G4S_HIP_TRY(hipGetLastError());
        }
        if (mode != KIND_PULL) {                                   // a batch of push steps: no-ops from the first stop on
            const int grid = know && h.stop != 3 ? sized.grid(h.edges_cur + h.n_cur + h.n_hub_cur) : sized.max_grid;
            a.grid_cap = sized.cap(grid);
            for (int b = 0; b < batch; ++b) {
                a.resume = b == 0;
                if (values || !BFS) hipLaunchKernelGGL((push_kernel<BFS, true>), dim3(grid), dim3(WG), 0, s, rows, A->d_rowptr, A->d_colids, A->d_values, dist, level, w->mark, q0, q1, st, a);
                else hipLaunchKernelGGL((push_kernel<BFS, false>), dim3(grid), dim3(WG), 0, s, rows, A->d_rowptr, A->d_colids, A->d_values, dist, level, w->mark, q0, q1, st, a);
            }
            G4S_HIP_TRY(hipGetLastError());
            a.grid_cap = LLONG_MAX;
            a.resume = 0;
            if (know) batch = sized.next_batch(batch);
        }
        hipLaunchKernelGGL(count_kernel<BFS>, dim3(grid_rows(rows, w->mem.cus)), dim3(WG), 0, s, rows, dist, level, st);
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(reads.fetch(h, st));
        ++waits;
        know = true;
        if (h.stop == 1 || h.stop == 2) break;
    }
    if (info) {
        info->iterations = h.iter;
        info->converged = h.stop == 1;
        info->push_steps = h.push_steps;
        info->pull_steps = h.pull_steps;
        info->host_waits = waits;
        info->reserved = 0;
        info->reached = h.reached;
        info->edges_relaxed = h.edges_relaxed;
    }
    return G4S_OK;
}

int check_args(const char *fn, g4s_csr_t A, const int32_t *sources, int32_t n_sources, const void *out, int32_t cap, unsigned flags)
{
    const char *what = (flags & ~kAllFlags) ? "flags other than G4S_TRAVERSE_PUSH / _PULL / _SYMMETRIC"
                       : (flags & kDirFlags) == kDirFlags ? "G4S_TRAVERSE_PUSH and G4S_TRAVERSE_PULL together"
                       : !A ? "NULL handle" : !sources ? "sources is NULL" : !out ? "the output array is NULL"
                       : n_sources < 1 ? "n_sources < 1" : cap < 0 ? "negative iteration cap" : nullptr;
    return what ? g4s::set_error(G4S_ERR_INVALID, "%s: %s", fn, what) : (int)G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_traverse_reserve(g4s_csr_t A, unsigned flags)
{
    G4S_REQUIRE((flags & ~kAllFlags) == 0u, "flags other than G4S_TRAVERSE_PUSH / _PULL / _SYMMETRIC");
    G4S_REQUIRE((flags & kDirFlags) != kDirFlags, "G4S_TRAVERSE_PUSH and G4S_TRAVERSE_PULL together");
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(A->rows == A->cols, "a traversal needs a square matrix");
    G4S_HIP_TRY(hipDeviceSynchronize());
    return reserve(A, flags);
}

G4S_API g4s_status g4s_sssp(g4s_csr_t A, const int32_t *sources, int32_t n_sources, double *dist_dev, int32_t max_iterations, unsigned flags,
                            g4s_traverse_info *info, void *stream)
{
    G4S_TRY(check_args(__func__, A, sources, n_sources, dist_dev, max_iterations, flags));
    return traverse<false>(A, sources, n_sources, dist_dev, nullptr, max_iterations, flags, info, g4s::as_stream(stream));
}

G4S_API g4s_status g4s_bfs(g4s_csr_t A, const int32_t *sources, int32_t n_sources, int32_t *level_dev, int32_t max_depth, unsigned flags,
                           g4s_traverse_info *info, void *stream)
{
    G4S_TRY(check_args(__func__, A, sources, n_sources, level_dev, max_depth, flags));
    return traverse<true>(A, sources, n_sources, nullptr, level_dev, max_depth, flags, info, g4s::as_stream(stream));
}
