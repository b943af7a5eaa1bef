// betweenness.hip — g4s_betweenness (include/g4s.h): Brandes' betweenness centrality on a CSR handle stored by out-edges, one source after the other,
// both halves of every traversal on the device.
//
// Forward half: a BFS that counts shortest paths, ONE kernel per level, on the frontier walk of frontier.hpp. `order` holds every frontier of the
// traversal one behind the other (a vertex joins once, so rows entries suffice); level d is order[level_start[d] .. level_start[d + 1]). A vertex
// above kHubCut edges is also kept in a hub list of its own (two of them, ping-pong: `order` has no free back end). Per edge
// u → v: compare-and-swap of level[v] from −1 to d + 1 — the winner appends v, one atomicAdd per wave — then, if level[v] == d + 1, σ[v] += σ[u] by
// an fp64 global atomic. σ[u] is final: level d was completed behind the previous kernel boundary, and nobody reads σ[v] before the next one.
// The workgroup that finishes last (a ticket, no waiting) records level_start[d + 2], the lane count of the new level for the way back, the
// counters and `stop`: 1 nothing new was found, 4 the frontier outgrew the launch grid. A kernel that finds stop != 0 returns at once, so the host
// enqueues kBatch (doubling to kBatchMax) launches blind and reads the 104-byte state once per batch. Each frontier vertex's σ goes into one max
// per source (sigma_max_bits): a non-finite one is G4S_ERR_OVERFLOW, one above 2^53 clears sigma_exact.
//
// Backward half: D known from that read, one kernel per level d = D − 1 … 1 without further reads (level 0 is the source, whose δ is 0 by
// definition). Vertex u of level d is OWNED by a group of LPR ∈ {1, 4, 16, 64} lanes — chosen per level from its mean degree by the forward step
// that built it — which walks row u of A (no transpose: the successors of u are among its out-edges) and sums σ[u] / σ[v] · (1 + δ[v]) over the
// edges into level d + 1: lane j takes entries j, j + LPR, … in order, then a butterfly over the group. The owner writes δ[u] and acc[u] += δ[u].
// Rows above kHubCut are skipped there and summed by a whole workgroup each (back_long_kernel: 256 strided partial sums, a shuffle tree per
// wave, the waves in index order); that kernel is launched only when the handle has such a row. No atomics on this side, so δ and acc are the
// same bits whatever the grid. An epilogue writes bc = (old bc) + scale · acc.
//
// Determinism: while every σ <= 2^53 the forward atomics add integers exactly, in any order; everything else is summed in an order fixed by the
// graph and the source list. Where it loses: one level is one launch in each direction — a deep graph is launch-bound.
#include "common.hpp"
#include "csr_handle.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "betweenness.hpp"
#include <algorithm>
#include <climits>
#include <cmath>
#include <new>

namespace {

using g4s::BcState;

constexpr int kBatch = G4S_BC_BATCH;      // forward launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)

static_assert(sizeof(BcState) == 104, "the host reads BcState as one small block");

struct StepArgs {
    long long grid_cap;   // more out-edges than this ask for a larger grid
    int resume;           // the first launch of a batch goes on from stop == 4
};

struct Arrays {           // the workspace and the matrix, as the kernels see them
    int rows, hub_cap;
    const int *rowptr, *colids;
    const double *values;
    int *level, *order, *level_start, *hub0, *hub1;
    unsigned char *lpr;
    double *sigma, *delta, *acc;
    BcState *st;
};

__device__ __forceinline__ int lanes_for(long long edges, int n) { return edges <= 2ll * n ? 1 : edges <= 8ll * n ? 4 : edges <= 32ll * n ? 16 : 64; }

// The fills of one traversal, fused: level = −1, σ = δ = 0 (acc too for the first source of a call), the source at level 0 with σ = 1, the state.
__global__ __launch_bounds__(WG) void init_kernel(const Arrays w, int src, int first)
{
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < w.rows; i += (long long)gridDim.x * WG) {
        const bool is = i == src;
        w.level[i] = is ? 0 : -1;
        w.sigma[i] = is ? 1.0 : 0.0;
        w.delta[i] = 0.0;
        if (first) w.acc[i] = 0.0;
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    BcState *st = w.st;
    const int deg = w.rowptr[src + 1] - w.rowptr[src], hub = deg > kHubCut;
    w.order[0] = src;
    w.level_start[0] = 0;
    w.level_start[1] = 1;
    if (hub) w.hub0[0] = src;
    st->edges_cur = deg; st->edges_next = 0; st->edges_level_max = deg;
    st->n_cur = 1; st->width_max = 1; st->n_hub_cur = hub; st->n_hub_next = 0;
    st->tail = 1; st->depth = 0; st->stop = 0; st->cur = 0; st->tickets = 0;
    if (first) { st->max_depth = 0; st->levels = 0; st->reached = 0; st->edges_walked = 0; st->sigma_max_bits = 0ull; }
    st->reached += 1;
}

// One atomicAdd per wave for the vertices its lanes discovered; a hub goes to the next hub list as well.
__device__ __forceinline__ void append(bool want, int v, int deg, const Arrays &w, int *hubs_next, long long &deg_sum)
{
    const int idx = wave_append(want, &w.st->tail);
    if (!want) return;
    if ((unsigned)idx < (unsigned)w.rows) w.order[idx] = v;            // a vertex is appended once per traversal: idx < rows by construction
    if (deg > kHubCut) {
        const int h = atomicAdd(&w.st->n_hub_next, 1);
        if ((unsigned)h < (unsigned)w.hub_cap) hubs_next[h] = v;       // at most nnz / (kHubCut + 1) such rows exist
    }
    deg_sum += deg;
}

// The edge u → v (entry k) seen from level d: claim v for level d + 1 if nobody has, then hand σ[u] on if v is in level d + 1.
template <bool VALUES>
__device__ __forceinline__ bool relax(int k, int v, double su, int d, const Arrays &w)
{
    if constexpr (VALUES) {
        if (!(w.values[k] != 0.0)) return false;                      // or-and: a stored 0.0 is no edge (NaN counts as one)
    }
    int lv = w.level[v];                                               // a stale read is −1: the compare-and-swap below decides
    bool won = false;
    if (lv == -1) {
        const int old = atomicCAS(w.level + v, -1, d + 1);
        won = old == -1;
        lv = won ? d + 1 : old;
    }
    if (lv == d + 1) atomicAdd(w.sigma + v, su);
    return won;
}

// The end of a forward step: the block's share of the next frontier's out-edges and of the σ maximum, then the ticket; the last block turns the page (turn_page).
__device__ __forceinline__ void finish(const Arrays &w, long long deg_sum, double smax, int d, int end, const StepArgs a)
{
    __shared__ long long s_red[WG / 64];
    __shared__ double s_max[WG / 64];
    BcState *st = w.st;
    deg_sum = wave_sum(deg_sum);
    smax = wave_max(smax);
    if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6] = deg_sum; s_max[threadIdx.x >> 6] = smax; }
    if (!turn_page(&st->tickets, [&] {
        long long sum = 0;
        double mx = 0.0;
        for (int i = 0; i < WG / 64; ++i) { sum += s_red[i]; mx = fmax(mx, s_max[i]); }
        if (sum) atomicAdd((unsigned long long *)&st->edges_next, (unsigned long long)sum);
        if (mx > 0.0) atomicMax(&st->sigma_max_bits, (unsigned long long)__double_as_longlong(mx));   // non-negative doubles order as their bits
    })) return;
    const int tail = atomicAdd(&st->tail, 0), nh = atomicAdd(&st->n_hub_next, 0);
    const long long e = (long long)atomicAdd((unsigned long long *)&st->edges_next, 0ull);
    const int n_new = tail - end;
    st->levels += 1;
    st->edges_walked += st->edges_cur * (n_new > 0 ? 2 : 1);           // level d is walked again on the way back unless it is the deepest
    w.level_start[d + 2] = tail;                                       // d <= rows − 1 and level_start has rows + 2 entries
    if (n_new > 0) {
        w.lpr[d + 1] = (unsigned char)lanes_for(e, n_new);
        st->depth = d + 1;
        st->reached += n_new;
        if (d + 1 > st->max_depth) st->max_depth = d + 1;
        if (n_new > st->width_max) st->width_max = n_new;
        if (e > st->edges_level_max) st->edges_level_max = e;
    }
    st->n_cur = n_new; st->n_hub_cur = nh; st->edges_cur = e;
    st->n_hub_next = 0; st->edges_next = 0;
    st->cur ^= 1;
    st->tickets = 0;
    st->stop = n_new == 0 ? 1 : (e > a.grid_cap ? 4 : 0);
}

template <bool VALUES>
__global__ __launch_bounds__(WG) void forward_kernel(const Arrays w, const StepArgs a)
{
    BcState *st = w.st;
    if (!step_runs(st->stop, a.resume)) return;
    const int d = st->depth, cur = st->cur;
    const int begin = w.level_start[d], end = w.level_start[d + 1];
    const int *hubs = cur ? w.hub1 : w.hub0;
    int *hubs_next = cur ? w.hub0 : w.hub1;
    long long deg_sum = 0;
    double smax = 0.0;
    auto vertex = [&](int u, int &start, int &deg, double &su) {
        start = w.rowptr[u];
        deg = w.rowptr[u + 1] - start;
        su = w.sigma[u];
    };
    auto entry = [&](bool valid, int k, double su) {
        bool want = false;
        int v = 0, vdeg = 0;
        if (valid) {
            v = w.colids[k];
            want = relax<VALUES>(k, v, su, d, w);
            if (want) vdeg = w.rowptr[v + 1] - w.rowptr[v];
        }
        append(want, v, vdeg, w, hubs_next, deg_sum);
    };
    walk_tiles<double>(end - begin, [&](int i, int &start, int &deg, double &su) {
        vertex(w.order[begin + i], start, deg, su);
        if (deg > kHubCut) deg = 0;                                    // a hub: walked below, out of the hub list
        smax = fmax(smax, su);                                         // fmax drops a NaN; +inf is what an overflow leaves
    }, entry);
    walk_hubs<double>(st->n_hub_cur, [&](int h, int &start, int &deg, double &su) { vertex(hubs[h], start, deg, su); }, entry);
    finish(w, deg_sum, smax, d, end, a);
}

// The term of the edge u → v (entry k) in δ[u], for u in level d.
template <bool VALUES>
__device__ __forceinline__ double term(int k, double su, int d, const Arrays &w)
{
    if constexpr (VALUES) {
        if (!(w.values[k] != 0.0)) return 0.0;
    }
    const int v = w.colids[k];
    if (w.level[v] != d + 1) return 0.0;
    return su / w.sigma[v] * (1.0 + w.delta[v]);
}

// Level [begin, end) of `order`, LPR lanes per vertex: lane j sums entries j, j + LPR, … of the row in order, then a butterfly over the group.
template <int LPR, bool VALUES>
__device__ __forceinline__ void back_rows(const Arrays &w, int begin, int end, int d, int src)
{
    constexpr int GPB = WG / LPR;
    const int t = (int)threadIdx.x, lig = t % LPR;
    for (long long r0 = (long long)begin + (long long)blockIdx.x * GPB; r0 < end; r0 += (long long)gridDim.x * GPB) {
        const long long i = r0 + t / LPR;
        double sum = 0.0;
        bool mine = false;
        int u = 0;
        if (i < end) {
            u = w.order[i];
            const int b = w.rowptr[u], e = w.rowptr[u + 1];
            if (e - b <= kHubCut) {
                mine = true;
                const double su = w.sigma[u];
                for (int k = b + lig; k < e; k += LPR) sum += term<VALUES>(k, su, d, w);
            }
        }
        if constexpr (LPR > 1) {
            for (int o = LPR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        }
        if (mine && lig == 0) {
            w.delta[u] = sum;
            if (u != src) w.acc[u] += sum;
        }
    }
}

template <bool VALUES>
__global__ __launch_bounds__(WG) void backward_kernel(const Arrays w, int d, int src)
{
    const int begin = w.level_start[d], end = w.level_start[d + 1];
    switch (w.lpr[d]) {                                                // written by the forward step that built level d: the same for every block
    case 1: back_rows<1, VALUES>(w, begin, end, d, src); break;
    case 4: back_rows<4, VALUES>(w, begin, end, d, src); break;
    case 16: back_rows<16, VALUES>(w, begin, end, d, src); break;
    default: back_rows<64, VALUES>(w, begin, end, d, src); break;
    }
}

// The hubs of level d: a workgroup looks at 256 entries of the level and sums each long row among them with all its threads, in a fixed tree.
template <bool VALUES>
__global__ __launch_bounds__(WG) void back_long_kernel(const Arrays w, int d, int src)
{
    __shared__ unsigned long long s_mask[WG / 64];
    __shared__ double s_red[WG / 64];
    const int begin = w.level_start[d], end = w.level_start[d + 1];
    const int t = (int)threadIdx.x;
    for (long long base = (long long)begin + (long long)blockIdx.x * WG; base < end; base += (long long)gridDim.x * WG) {
        const long long i = base + t;
        bool is_long = false;
        if (i < end) {
            const int u = w.order[i];
            is_long = w.rowptr[u + 1] - w.rowptr[u] > kHubCut;
        }
        const unsigned long long m = __ballot(is_long);
        if ((t & 63) == 0) s_mask[t >> 6] = m;
        __syncthreads();
        for (int wv = 0; wv < WG / 64; ++wv) {
            unsigned long long mm = s_mask[wv];                        // the same word for every thread: the loop below is uniform
            while (mm) {
                const int u = w.order[base + wv * 64 + (__ffsll((long long)mm) - 1)];
                mm &= mm - 1;
                const int b = w.rowptr[u], e = w.rowptr[u + 1];
                const double su = w.sigma[u];
                double s = 0.0;
                for (int k = b + t; k < e; k += WG) s += term<VALUES>(k, su, d, w);
                s = wave_sum(s);
                if ((t & 63) == 0) s_red[t >> 6] = s;
                __syncthreads();
                if (t == 0) {
                    double sum = 0.0;
                    for (int i2 = 0; i2 < WG / 64; ++i2) sum += s_red[i2];
                    w.delta[u] = sum;
                    if (u != src) w.acc[u] += sum;
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(WG) void epilogue_kernel(int rows, double scale, int accumulate, const double *__restrict__ acc, double *__restrict__ bc)
{
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < rows; i += (long long)gridDim.x * WG) bc[i] = (accumulate ? bc[i] : 0.0) + scale * acc[i];
}

__global__ __launch_bounds__(WG) void max_degree_kernel(int rows, const int *__restrict__ rowptr, BcState *st)
{
    int m = 0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < rows; i += (long long)gridDim.x * WG) m = max(m, rowptr[i + 1] - rowptr[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&st->max_degree, m);
}

} // namespace

// ------------------------------------------------------------------------------------------------ the handle's workspace
namespace g4s {

struct BcWork {
    int32_t *ints = nullptr;      // level (n) | order (n) | level_start (n + 2) | hub list 0 | hub list 1 (hub_cap each)
    unsigned char *lpr = nullptr; // lanes per vertex of every level's backward step (n + 2 bytes)
    double *vec = nullptr;        // sigma | delta | acc, n doubles each
    BcState *state = nullptr;
    int hub_cap = 1;
    int max_degree = 0;
    ZeroScan zeros;               // is a stored value 0.0? the kernels then have to read the values
    int64_t n = 0;
    DevicePieces mem;             // owns the arrays above
};

void betweenness_work_destroy(BcWork *w) { delete w; }
long long betweenness_work_bytes(const BcWork *w) { return w ? w->mem.bytes : 0; }
void betweenness_values_changed(BcWork *w) { if (w) w->zeros.changed(); }

} // namespace g4s

namespace {

// The workspace (once), the longest row and whether a stored value is zero. NULL stream, synchronous.
int reserve(g4s_csr_s *A)
{
    if (!A->bc) {
        std::unique_ptr<g4s::BcWork> w(new (std::nothrow) g4s::BcWork());
        if (!w) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
        const size_t n = (size_t)std::max(A->rows, 1);
        w->n = (int64_t)n;
        w->hub_cap = (int)std::min<int64_t>((int64_t)n, A->nnz / (kHubCut + 1)) + 1;
        const size_t n_ints = 3 * n + 2 + 2 * (size_t)w->hub_cap;
        w->mem.take(&w->ints, sizeof(int32_t) * n_ints);
        w->mem.take(&w->lpr, n + 2);
        w->mem.take(&w->vec, sizeof(double) * 3 * n);
        w->mem.take(&w->state, sizeof(BcState));
        if (w->mem.ok()) w->mem.note(hipMemset(w->state, 0, sizeof(BcState)));
        if (w->mem.ok() && A->rows > 0) {
            hipLaunchKernelGGL(max_degree_kernel, dim3(grid_rows(A->rows, w->mem.cus)), dim3(WG), 0, nullptr, A->rows, A->d_rowptr, w->state);
            w->mem.note(hipGetLastError());
            if (w->mem.ok()) w->mem.note(hipMemcpy(&w->max_degree, &w->state->max_degree, sizeof(int), hipMemcpyDeviceToHost));
        }
        if (!w->mem.ok()) return w->mem.report("g4s_csr_betweenness_reserve");
        A->bc = w.release();
    }
    g4s::BcWork *w = A->bc;
    return w->zeros.scan(A->nnz, A->d_values, w->mem.cus, &w->state->zero_values, nullptr, nullptr);
}

int betweenness(g4s_csr_s *A, const int32_t *sources, int32_t n_sources, double scale, double *bc, unsigned flags, g4s_bc_info *info, hipStream_t s)
{
    const char *fn = "g4s_betweenness";
    if (A->rows != A->cols) return g4s::set_error(G4S_ERR_INVALID, "%s: the handle is %d x %d, betweenness needs a square matrix", fn, A->rows, A->cols);
    for (int32_t i = 0; i < n_sources; ++i)
        if (sources[i] < 0 || sources[i] >= A->rows) return g4s::set_error(G4S_ERR_INVALID, "%s: sources[%d] = %d is outside [0, %d)", fn, i, sources[i], A->rows);
    G4S_TRY(not_capturing(fn, s, "its state"));
    if (info) *info = g4s_bc_info{};
    if (!A->bc) G4S_TRY(reserve(A));
    g4s::BcWork *wk = A->bc;

    const int rows = A->rows;
    const size_t n = (size_t)wk->n;
    Arrays w;
    w.rows = rows; w.hub_cap = wk->hub_cap;
    w.rowptr = A->d_rowptr; w.colids = A->d_colids; w.values = A->d_values;
    w.level = wk->ints; w.order = wk->ints + n; w.level_start = wk->ints + 2 * n; w.hub0 = wk->ints + 3 * n + 2; w.hub1 = w.hub0 + wk->hub_cap;
    w.lpr = wk->lpr;
    w.sigma = wk->vec; w.delta = wk->vec + n; w.acc = wk->vec + 2 * n;
    w.st = wk->state;
    BcState *st = wk->state;

    // New values since the last verdict: the scan runs in front of the first traversal, which reads the values whatever it will say; the verdict
    // comes back with the first state read, so it costs no wait of its own.
    const bool rescan = wk->zeros.state == 0;
    if (rescan && A->nnz > 0) G4S_HIP_TRY(wk->zeros.enqueue(A->nnz, A->d_values, wk->mem.cus, &st->zero_values, s));
    const bool values = wk->zeros.state != 1;
    const bool has_hubs = wk->max_degree > kHubCut;
    using g4s::kEdgesPerWg;                                                // the forward grid: 8 workgroups to two per CU, and no more than the graph is work for
    const g4s::StepGrid sized(g4s::kMinGrid, (int)std::min<long long>(2LL * wk->mem.cus, (A->nnz + rows + kEdgesPerWg - 1) / kEdgesPerWg));

    g4s::ReadScope reads(s);
    BcState h{};
    int waits = 0;
    for (int32_t i = 0; i < n_sources; ++i) {
        const int src = sources[i];
        hipLaunchKernelGGL(init_kernel, dim3(grid_rows(rows, wk->mem.cus)), dim3(WG), 0, s, w, src, (int)(i == 0));
        G4S_HIP_TRY(hipGetLastError());
        bool know = false, outgrown = false;                               // h is this traversal's state; a frontier outgrew a sized grid once
        int batch = kBatch;
        for (;;) {
            const int grid = know && !outgrown ? sized.grid(h.edges_cur + h.n_cur) : sized.max_grid;
            StepArgs a;
            a.grid_cap = sized.cap(grid);
            for (int b = 0; b < batch; ++b) {
                a.resume = b == 0;
                if (values) hipLaunchKernelGGL(forward_kernel<true>, dim3(grid), dim3(WG), 0, s, w, a);
                else hipLaunchKernelGGL(forward_kernel<false>, dim3(grid), dim3(WG), 0, s, w, a);
            }
            G4S_HIP_TRY(hipGetLastError());
            G4S_HIP_TRY(reads.fetch(h, st));
            ++waits;
            if (rescan) wk->zeros.state = h.zero_values ? 2 : 1;
            if (h.stop == 1) break;
            if (h.stop == 4) outgrown = true;                              // the rest of this traversal runs on the full grid: one resume per source
            if (know) batch = sized.next_batch(batch);
            know = true;
        }
        double smax;
        memcpy(&smax, &h.sigma_max_bits, sizeof smax);
        if (!(smax < (double)INFINITY))
            return g4s::set_error(G4S_ERR_OVERFLOW, "%s: the number of shortest paths from sources[%d] = %d exceeds the range of a double", fn, i, src);
        const int D = h.depth;
        const int gb = (int)std::max(1LL, std::min(4LL * wk->mem.cus, (h.edges_level_max + h.width_max + kEdgesPerWg - 1) / kEdgesPerWg));
        const int gl = (int)std::max(1LL, std::min(4LL * wk->mem.cus, ((long long)h.width_max + WG - 1) / WG));
        for (int d = D - 1; d >= 1; --d) {
            if (values) hipLaunchKernelGGL(backward_kernel<true>, dim3(gb), dim3(WG), 0, s, w, d, src);
            else hipLaunchKernelGGL(backward_kernel<false>, dim3(gb), dim3(WG), 0, s, w, d, src);
            if (has_hubs) {
                if (values) hipLaunchKernelGGL(back_long_kernel<true>, dim3(gl), dim3(WG), 0, s, w, d, src);
                else hipLaunchKernelGGL(back_long_kernel<false>, dim3(gl), dim3(WG), 0, s, w, d, src);
            }
        }
        G4S_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(epilogue_kernel, dim3(grid_rows(rows, wk->mem.cus)), dim3(WG), 0, s, rows, scale, (int)((flags & G4S_BC_ACCUMULATE) != 0), (const double *)w.acc, bc);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(reads.wait());
    ++waits;
    if (info) {
        double smax;
        memcpy(&smax, &h.sigma_max_bits, sizeof smax);
        info->sources = n_sources;
        info->max_depth = h.max_depth;
        info->host_waits = waits;
        info->sigma_exact = smax <= 9007199254740992.0;
        info->levels = h.levels;
        info->reached = h.reached;
        info->edges_walked = h.edges_walked;
        info->sigma_max = smax;
    }
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_betweenness_reserve(g4s_csr_t A, unsigned flags)
{
    G4S_REQUIRE(flags == 0u, "flags must be 0");
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(A->rows == A->cols, "betweenness needs a square matrix");
    G4S_HIP_TRY(hipDeviceSynchronize());
    return reserve(A);
}

G4S_API g4s_status g4s_betweenness(g4s_csr_t A, const int32_t *sources, int32_t n_sources, double scale, double *bc_dev, unsigned flags, g4s_bc_info *info,
                                   void *stream)
{
    G4S_REQUIRE((flags & ~G4S_BC_ACCUMULATE) == 0u, "flags other than G4S_BC_ACCUMULATE");
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(sources, "sources is NULL");
    G4S_REQUIRE(bc_dev, "bc_dev is NULL");
    G4S_REQUIRE(n_sources >= 1, "n_sources < 1 (sources is empty)");
    G4S_REQUIRE(std::isfinite(scale), "scale is not finite");
    return betweenness(A, sources, n_sources, scale, bc_dev, flags, info, g4s::as_stream(stream));
}
