// ktruss.hip — g4s_ktruss (include/g4s.h): the truss numbers of a simple undirected graph given as a symmetric CSR pattern, by synchronous peeling of
// edges by triangle support, and with them the peel order (round: which frontier removed the edge) and the supports in the input graph. DESIGN §4.17.
//
// State lives on the device (ktruss.hpp, KtState). Every undirected off-diagonal edge has a compact id c in [0, m): the rank of its stored entry right
// of the diagonal. All per-edge state (sup, rnd, tr) is indexed by c, so a decrement is one atomic and a scan runs over m words; eid[p] maps a stored
// entry to its edge (−1 for a diagonal entry), eu[c] < ev[c] are the endpoints. The graph is peeled level by level (j = the smallest remaining support,
// truss = j + 2) and inside a level frontier by frontier; every edge enters a frontier exactly once per call, so ONE queue of m ints holds all frontiers
// one behind the other (kcore.hip's layout): [head, end) is the current frontier, [end, tail) the one being built. Every step is one kernel; the workgroup
// that finishes last (a ticket counter, no waiting) turns the page. A step kernel that finds nothing to do returns at once, so the host enqueues scans
// and peels blind, kBatch (doubling to kBatchMax) launches behind one read of the state, as kcore.hip does.
//
//   open   kt_open_rows_kernel: rowptr[0] == 0, non-decreasing; nnz = rowptr[n]. With device pointers the host reads the state here (it sizes the work
//          block from nnz). kt_open_ids_kernel / kt_open_hubs_kernel (return at once when the rows were bad): ids in [0, n), rows strictly ascending,
//          up[p] = 1 for an entry right of the diagonal; rows above kHubCut go through a hub list. An exclusive scan of up (prims.hpp) is the rank:
//          m = rank[nnz]. kt_build_kernel: per entry, eid[p] — the rank itself right of the diagonal, where it also writes eu, ev, sup = 0, rnd = −1 and
//          sends the edge to the support pass's hub list when its shorter row is long; left of the diagonal the rank of the mirror entry, found by a
//          binary search (−1 when the declared symmetry does not hold: such an entry is left out, nothing is indexed through it).
//   walk   one body, two users: an item is an edge c, its row for walk_tiles / walk_hubs is the SHORTER of its endpoints' stored rows, the payload is
//          (c, u, v, the other row's bounds). Per entry w of that row: skip u and v, binary-search w in the other row; a hit at positions k, k2 is a
//          triangle whose other two edges are eid[k] and eid[k2]. A tile of walk_tiles is one workgroup's loop over 256 rows, which is too coarse
//          where the items' rows are long: item i is presented as row i << spread with empty rows between (intersect_walk), spread chosen per peel
//          from the frontier's average walk length, and the host weighs a walk entry as kEntryWeight plain ones when it sizes the grid.
//   support  the walk over all m edges (kt_support_kernel); a hit adds 1 to the item's own counter — one atomic per wave where the wave's hits belong
//          to one edge. kt_support_out_kernel then sums the supports (3 · triangles) and scatters them to the caller's array.
//   scan   runs when the frontier is empty: every remaining edge with sup <= j joins the frontier (tr = j + 2, rnd = the coming round); the others
//          contribute to a minimum. Page turn: nothing collected → j := that minimum, and stop = 2 when j + 2 >= max_k.
//   peel   runs when the frontier is not empty: the walk over queue[head, end), hubs out of the hub list. Per triangle (e; f, g) found from frontier
//          edge e in round r (an entry of the walked row whose own edge left before round r is turned down before the search): rnd[f], rnd[g] by
//          plain loads; a value in [0, r) — the triangle is dead; == r — that edge is in this frontier. Both in
//          the frontier: nothing. One of them, say f: g loses 1 only when c(e) < c(f), so the triangle dies ONCE. Neither: both lose 1. A decrement is
//          old = atomicSub(sup + g, 1); the one lane that sees old == j + 1 appends g and writes tr[g] = j + 2, rnd[g] = r + 1. Page turn as kcore.hip:
//          stop = 1 when the built frontier is empty and every edge has been removed, 4 when it has more walk entries than the batch's grid was sized for.
//   finish kt_finish_kernel, behind every batch, a no-op until stop is 1 or 2: tr / rnd go to the per-entry outputs through eid (an edge left by max_k
//          gets max_k and −1, a diagonal entry 0 and −1) and the edges of the top truss are counted.
// Memory model: kernel boundaries are the only ordering between workgroups. Inside a peel of round r the values of rnd below r and equal to r were
// written by earlier kernels and do not change; the only value that races is −1 against r + 1, and both read as "alive, not in this frontier". Supports
// only decrease; an edge appended in this kernel may take further decrements, which nobody reads again (it is in the next frontier, whose members are
// never decremented, and its tr and rnd are already written by the one appending lane). Nothing spins; every loop is bounded by a queue or a row length.
#include "common.hpp"
#include "level_peel.hpp"
#include "prims.hpp"
#include "ktruss.hpp"
#include <algorithm>
#include <climits>

namespace {

using g4s::KtState;

constexpr int kBatch = G4S_KTRUSS_BATCH;     // step launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr int kScanUnroll = 4;                // edges per thread and trip of a scan
constexpr long long kEntryWeight = 16;        // a walk entry is a binary search in the other row — a dozen dependent loads — where StepGrid counts plain entries
constexpr size_t kStateBytes = 256;
static_assert(sizeof(KtState) <= kStateBytes, "state block");

struct StepArgs {
    long long grid_cap;    // a frontier with more walk entries than this asks for a larger peel grid
    int max_k;
    int hub_cap;           // room in each hub list
    int resume;            // peel only: the first launch of a batch goes on from stop == 4
};

// the arrays of the work block; every one has room for nnz ints (m <= nnz), rank for nnz + 1
struct Graph {
    const int *rowptr, *colids;
    int *rank, *eid, *eu, *ev, *sup, *rnd, *tr, *queue;
    int *hubs0, *hubs1;
};

struct EdgeRef {
    int c, u, v;           // the edge and its endpoints
    int ob, oe;            // the other (longer) row
};

// the position of w in the ascending colids[lo, hi), −1 when it is not there
__device__ __forceinline__ int find(const int *__restrict__ colids, int lo, int hi, int w)
{
    const int end = hi;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (colids[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && colids[lo] == w ? lo : -1;
}

// Edge c as an item of the walk: its shorter row (u's on a tie) is walked, the other one searched.
__device__ __forceinline__ void edge_item(int c, const Graph &g, int &start, int &len, EdgeRef &r)
{
    const int u = g.eu[c], v = g.ev[c];
    const int ub = g.rowptr[u], ul = g.rowptr[u + 1] - ub, vb = g.rowptr[v], vl = g.rowptr[v + 1] - vb;
    r.c = c; r.u = u; r.v = v;
    if (ul <= vl) { start = ub; len = ul; r.ob = vb; r.oe = vb + vl; }
    else { start = vb; len = vl; r.ob = ub; r.oe = ub + ul; }
}

__device__ __forceinline__ int walk_len(int c, const Graph &g)
{
    const int u = g.eu[c], v = g.ev[c];
    const int ul = g.rowptr[u + 1] - g.rowptr[u], vl = g.rowptr[v + 1] - g.rowptr[v];
    return ul <= vl ? ul : vl;
}

// An edge for the frontier being built (append_frontier). An edge is appended once per call: its slot is below m, which the kernel reads once and hands
// down (a load of st->m per entry waits behind the atomics on its neighbours in the state block). Unlike rows, the edges whose walk row is long have no
// bound below kHubCap (kHubCap of them is the limit of the call): a full hub list refuses the pattern.
__device__ __forceinline__ void append(bool want, int c, int len, int m, const StepArgs &a, const Graph &g, int *__restrict__ hubs_next, KtState *st, long long &len_sum)
{
    if (!append_frontier(want, c, len, m, a.hub_cap, g.queue, hubs_next, &st->tail, &st->n_hub_next, len_sum)) atomicOr(&st->invalid, 8);
}

__global__ __launch_bounds__(WG) void kt_open_rows_kernel(int n, const int *__restrict__ rowptr, KtState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [](long long, int, int) {});
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->nnz = rowptr[n];
        st->min_left = INT_MAX;
    }
}

// The column ids (open_ids / open_hubs, strictly ascending rows): up[k] = 1 for an entry right of the diagonal, in rank's array; the rows above kHubCut
// entries stay in hubs1 for the building pass.
__global__ __launch_bounds__(WG) void kt_open_ids_kernel(int n, int nnz, int hub_cap, const Graph g, KtState *st)
{
    if (st->invalid || st->nnz != nnz) return;                     // rowptr is monotone from 0 to nnz beyond this line: [0, nnz) is the colids array
    if (blockIdx.x == 0 && threadIdx.x == 0) g.rank[nnz] = 0;      // the scan's total lands here
    open_ids<true>(n, hub_cap, g.rowptr, g.colids, g.hubs1, &st->n_hub_rows, &st->invalid, 2, [&](int k, int u, int v) { g.rank[k] = v > u; });
}

__global__ __launch_bounds__(WG) void kt_open_hubs_kernel(int n, int nnz, int hub_cap, const Graph g, KtState *st)
{
    if (st->invalid || st->nnz != nnz) return;
    open_hubs<true>(n, hub_cap, g.rowptr, g.colids, g.hubs1, &st->n_hub_rows, &st->invalid, 2, [&](int k, int u, int v) { g.rank[k] = v > u; });
}

// Behind the scan of up: m, and the two ends that need no step (no edge at all; max_k == 2, under which no level lies).
__global__ void kt_open_m_kernel(int nnz, int max_k, const int *__restrict__ rank, KtState *st)
{
    if (st->invalid || st->nnz != nnz) { if (!st->invalid) st->invalid = 1; return; }
    const int m = rank[nnz];
    st->m = m;
    if (m == 0) st->stop = 1;
    else if (max_k <= 2) st->stop = 2;
}

// One entry of row u in the building pass (see the head of the file).
__device__ __forceinline__ void build_entry(bool valid, int k, OpenRow r, int hub_cap, const Graph &g, KtState *st)
{
    if (!valid) return;
    const int v = g.colids[k], u = r.u;
    if (v > u) {
        const int c = g.rank[k];
        g.eid[k] = c;
        g.eu[c] = u; g.ev[c] = v;
        g.sup[c] = 0; g.rnd[c] = -1; g.tr[c] = 0;
        const int ul = g.rowptr[u + 1] - g.rowptr[u], vl = g.rowptr[v + 1] - g.rowptr[v];
        if ((ul <= vl ? ul : vl) > kHubCut) {
            const int h = atomicAdd(&st->n_hub_all, 1);
            if ((unsigned)h < (unsigned)hub_cap) g.hubs0[h] = c;
            else atomicOr(&st->invalid, 8);
        }
    } else if (v == u) {
        g.eid[k] = -1;
    } else {
        const int q = find(g.colids, g.rowptr[v], g.rowptr[v + 1], u);
        g.eid[k] = q >= 0 ? g.rank[q] : -1;
    }
}

__global__ __launch_bounds__(WG) void kt_build_kernel(int n, int hub_cap, const Graph g, KtState *st)
{
    if (st->invalid) return;
    auto entry = [&](bool valid, int k, OpenRow r) { build_entry(valid, k, r, hub_cap, g, st); };
    walk_tiles<OpenRow>(n, [&](int i, int &start, int &len, OpenRow &r) {
        const int rb = g.rowptr[i], l = g.rowptr[i + 1] - rb;
        r.u = i;
        r.start = rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        start = rb;
        len = l;
    }, entry);
    walk_hubs<OpenRow>(st->n_hub_rows < hub_cap ? st->n_hub_rows : hub_cap, [&](int h, int &start, int &len, OpenRow &r) {
        r.u = g.hubs1[h];
        r.start = start = g.rowptr[r.u];
        len = g.rowptr[r.u + 1] - start;
    }, entry);
}

// The intersect walk over `count` items (item(i) names the edge), hubs out of `hubs`: hit(valid, k, k2, e) by EVERY thread per entry; k2 >= 0 is a
// triangle through e whose other two edges are the stored entries k (in the walked row) and k2 (in the other row). live(k) may turn an entry of the
// walked row down before the search, which is the expensive part: a dozen dependent loads in a long row.
// spread (a shift): item i is presented to walk_tiles as row i << spread and the rows between are empty, so a tile — one workgroup's loop — holds
// 256 >> spread items: a frontier of few edges with long rows is dealt over many workgroups instead of one per 256 edges.
template <typename Item, typename Live, typename Hit>
__device__ __forceinline__ void intersect_walk(int count, int spread, Item item, const int *__restrict__ hubs, int n_hubs, const Graph &g, Live live, Hit hit)
{
    auto entry = [&](bool valid, int k, EdgeRef e) {
        int k2 = -1;
        if (valid) {
            const int w = g.colids[k];
            if (w != e.u && w != e.v && live(k)) k2 = find(g.colids, e.ob, e.oe, w);
        }
        hit(valid, k, k2, e);
    };
    walk_tiles<EdgeRef>(count << spread, [&](int i, int &start, int &len, EdgeRef &e) {
        if (i & ((1 << spread) - 1)) return;
        int s, l;
        edge_item(item(i >> spread), g, s, l, e);
        if (l > kHubCut) return;                                   // walked out of the hub list
        start = s;
        len = l;
    }, entry);
    walk_hubs<EdgeRef>(n_hubs, [&](int h, int &start, int &len, EdgeRef &e) { edge_item(hubs[h], g, start, len, e); }, entry);
}

__global__ __launch_bounds__(WG) void kt_support_kernel(int hub_cap, const Graph g, KtState *st)
{
    if (st->invalid || st->stop == 1) return;
    long long walked = 0;
    intersect_walk(st->m, 0, [](int i) { return i; }, g.hubs0, st->n_hub_all < hub_cap ? st->n_hub_all : hub_cap, g, [](int) { return true; },
                   [&](bool valid, int, int k2, EdgeRef e) {
        walked += valid;
        const bool hit = k2 >= 0;
        const unsigned long long hits = __ballot(hit);
        if (hits == 0) return;                                     // the same for the whole wave
        const int leader = __ffsll((long long)hits) - 1, c0 = __shfl(e.c, leader);
        if (__ballot(hit && e.c != c0) == 0) {                     // one edge's hits: one atomic
            if ((int)__lane_id() == leader) atomicAdd(g.sup + c0, __popcll(hits));
        } else if (hit) {
            atomicAdd(g.sup + e.c, 1);
        }
    });
    walked = wave_sum(walked);
    if ((threadIdx.x & 63) == 0 && walked) atomicAdd(&st->support_walked, (unsigned long long)walked);
}

// The supports of the input graph: their sum over the edges (3 · triangles), and the caller's per-entry array through eid.
__global__ __launch_bounds__(WG) void kt_support_out_kernel(int nnz, const Graph g, int *__restrict__ support, KtState *st)
{
    if (st->invalid) return;
    const int m = st->m;
    long long sum = 0;
    for (long long c = (long long)blockIdx.x * WG + threadIdx.x; c < m; c += (long long)gridDim.x * WG) sum += g.sup[c];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&st->support_sum, (unsigned long long)sum);
    if (!support) return;
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < nnz; p += (long long)gridDim.x * WG) {
        const int c = g.eid[p];
        support[p] = c >= 0 ? g.sup[c] : 0;
    }
}

__global__ __launch_bounds__(WG) void kt_scan_kernel(const Graph g, KtState *st, const StepArgs a)
{
    if (st->invalid || st->stop != 0 || st->end != st->head) return;   // the same words for every block: they change only after the last ticket
    const int jj = st->level, r = st->round, m = st->m;
    int *hubs_next = st->hub_cur ? g.hubs0 : g.hubs1;
    long long len_sum = 0;
    int mn = INT_MAX;
    for (long long i0 = (long long)blockIdx.x * (WG * kScanUnroll); i0 < m; i0 += (long long)gridDim.x * (WG * kScanUnroll)) {
        int x[kScanUnroll], d[kScanUnroll];
#pragma unroll
        for (int q = 0; q < kScanUnroll; ++q) {                    // the loads of a trip first: they do not depend on each other
            const long long i = i0 + q * WG + threadIdx.x;
            x[q] = i < m ? g.rnd[i] : 0;
        }
#pragma unroll
        for (int q = 0; q < kScanUnroll; ++q) {
            const long long i = i0 + q * WG + threadIdx.x;
            d[q] = x[q] == -1 ? g.sup[i] : 0;
        }
#pragma unroll
        for (int q = 0; q < kScanUnroll; ++q) {
            const long long i = i0 + q * WG + threadIdx.x;
            const bool want = x[q] == -1 && d[q] <= jj;
            int len = 0;
            if (want) {
                g.tr[i] = jj + 2;
                g.rnd[i] = r;
                len = walk_len((int)i, g);
            } else if (x[q] == -1) {
                mn = d[q] < mn ? d[q] : mn;
            }
            append(want, (int)i, len, m, a, g, hubs_next, st, len_sum);
        }
    }
    finish_step(st, len_sum, 0, mn, KIND_SCAN, a.grid_cap, a.max_k - 2, [&] { return st->m; });   // level j is truss j + 2: the levels end at max_k − 2
}

__global__ __launch_bounds__(WG) void kt_peel_kernel(const Graph g, KtState *st, const StepArgs a)
{
    if (st->invalid || st->end == st->head || !step_runs(st->stop, a.resume)) return;
    const int jj = st->level, r = st->round, head = st->head, m = st->m;
    const int *hubs_cur = st->hub_cur ? g.hubs1 : g.hubs0;
    int *hubs_next = st->hub_cur ? g.hubs0 : g.hubs1;
    long long len_sum = 0, walked = 0;
    // edge c loses one triangle; the lane that brings it to j joins it to the next frontier
    auto lose = [&](bool dec, int c) {
        bool want = false;
        int len = 0;
        if (dec) {
            want = atomicSub(g.sup + c, 1) == jj + 1;
            if (want) {
                g.tr[c] = jj + 2;
                g.rnd[c] = r + 1;
                len = walk_len(c, g);
            }
        }
        append(want, c, len, m, a, g, hubs_next, st, len_sum);
    };
    // an entry whose own edge left in an earlier round closes no live triangle: two loads instead of the search (late in a peel most of a long row is gone)
    auto live = [&](int k) {
        const int f = g.eid[k];
        return f >= 0 && !((unsigned)ld(g.rnd + f) < (unsigned)r);
    };
    // tiles of about 2048 walk entries: 256 edges a tile where the rows are short, down to 4 where they average 512 entries and more
    const int count = st->end - head;
    const long long avg = st->edges_cur / count;
    int spread = 0;
    while (spread < 6 && (avg >> (spread + 4)) > 0 && ((long long)count << (spread + 1)) < (1 << 30)) ++spread;
    intersect_walk(count, spread, [&](int i) { return g.queue[head + i]; }, hubs_cur, st->n_hub_cur < a.hub_cap ? st->n_hub_cur : a.hub_cap, g, live,
                   [&](bool valid, int k, int k2, EdgeRef e) {
        walked += valid;
        int f = -1, h = -1;
        bool df = false, dh = false;
        if (k2 >= 0) {
            f = g.eid[k];
            h = g.eid[k2];
            if (f >= 0 && h >= 0) {                                // −1: the declared symmetry does not hold here
                const int rf = ld(g.rnd + f), rh = ld(g.rnd + h);
                if (!((unsigned)rf < (unsigned)r || (unsigned)rh < (unsigned)r)) {   // else an edge left in an earlier round: the triangle is dead
                    const bool in_f = rf == r, in_h = rh == r;     // in this frontier; −1 and r + 1 are both "alive, outside it"
                    df = !in_f && (!in_h || e.c < h);
                    dh = !in_h && (!in_f || e.c < f);
                }
            }
        }
        lose(df, f);
        lose(dh, h);
    });
    finish_step(st, len_sum, walked, INT_MAX, KIND_PEEL, a.grid_cap, a.max_k - 2, [&] { return st->m; });
}

// Once the peeling has ended (stop 1 or 2; a no-op before): the edges left by max_k get truss = max_k, the edges of the top truss are counted, and
// the per-edge results go to the per-entry outputs.
__global__ __launch_bounds__(WG) void kt_finish_kernel(int nnz, int max_k, const Graph g, int *__restrict__ truss, int *__restrict__ round, KtState *st)
{
    __shared__ int s_red[WG / 64];
    if (st->invalid || (st->stop != 1 && st->stop != 2)) return;
    const int top = st->stop == 2 ? max_k : st->top_level + 2, m = st->m;
    int cnt = 0;
    for (long long c = (long long)blockIdx.x * WG + threadIdx.x; c < m; c += (long long)gridDim.x * WG) cnt += (g.rnd[c] == -1 ? max_k : g.tr[c]) == top;
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_red[w];
        if (sum) atomicAdd(&st->top_edges, (unsigned long long)sum);
    }
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < nnz; p += (long long)gridDim.x * WG) {
        const int c = g.eid[p];
        const int rc = c >= 0 ? g.rnd[c] : -1;
        truss[p] = c < 0 ? 0 : rc == -1 ? max_k : g.tr[c];
        if (round) round[p] = rc;
    }
}

// Everything behind the opening read on device arrays; returns behind a wait on `s` with *h the final state.
int run(int n, int nnz, int max_k, const Graph &g, int *truss, int *round, int *support, KtState *st, int hub_cap, int cus, KtState *h, Counts *cnt, hipStream_t s)
{
    // G4S_KTRUSS_SCAN_WGS and G4S_KTRUSS_MIN_GRID are A/B switches as kcore.hip's: the outputs do not depend on them.
    const g4s::StepGrid sized(env_int("G4S_KTRUSS_MIN_GRID", g4s::kMinGrid, 1, 2 * cus), 2 * cus);   // the peel grid of a batch: between 8 workgroups and two per CU
    const int g_rows = grid_rows(nnz, cus), g_scan = grid_for<WG * kScanUnroll>(nnz / 2 + 1, env_int("G4S_KTRUSS_SCAN_WGS", cus, 1, 8 * cus));
    StepArgs a;
    a.grid_cap = LLONG_MAX;
    a.max_k = max_k;
    a.hub_cap = hub_cap;
    a.resume = 0;
    hipLaunchKernelGGL(kt_open_ids_kernel, dim3(grid_for<WG>(n, 2048)), dim3(WG), 0, s, n, nnz, hub_cap, g, st);
    hipLaunchKernelGGL(kt_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, nnz, hub_cap, g, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(g.rank, g.rank, (long long)nnz + 1, s));
    hipLaunchKernelGGL(kt_open_m_kernel, dim3(1), dim3(1), 0, s, nnz, max_k, g.rank, st);
    hipLaunchKernelGGL(kt_build_kernel, dim3(grid_for<WG>(n, 2048)), dim3(WG), 0, s, n, hub_cap, g, st);
    hipLaunchKernelGGL(kt_support_kernel, dim3(grid_for<WG>(nnz / 2 + 1, 2048)), dim3(WG), 0, s, hub_cap, g, st);
    hipLaunchKernelGGL(kt_support_out_kernel, dim3(g_rows), dim3(WG), 0, s, nnz, g, support, st);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 9;                                            // the scan is three

    g4s::ReadScope reads(s);
    return run_level_peel(sized, kBatch, kEntryWeight, [&](long long grid_cap) {
        a.grid_cap = grid_cap;
        hipLaunchKernelGGL(kt_scan_kernel, dim3(g_scan), dim3(WG), 0, s, g, st, a);
    }, [&](int grid, long long grid_cap, int resume) {
        a.grid_cap = grid_cap;
        a.resume = resume;
        hipLaunchKernelGGL(kt_peel_kernel, dim3(grid), dim3(WG), 0, s, g, st, a);
        a.resume = 0;
    }, [&] { hipLaunchKernelGGL(kt_finish_kernel, dim3(g_rows), dim3(WG), 0, s, nnz, max_k, g, truss, round, st); }, reads, st, h, cnt);
}

} // namespace

G4S_API g4s_status g4s_ktruss(int32_t n, const int32_t *rowptr, const int32_t *colids, int32_t max_k, int32_t *truss, int32_t *round, int32_t *support,
                              unsigned flags, g4s_ktruss_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(max_k >= 2, "max_k below 2");
    G4S_REQUIRE(rowptr && truss, "rowptr or truss is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        const size_t eb = sizeof(int32_t) * (size_t)nnz;
        const Span outs[] = {{truss, eb}, {round, eb}, {support, eb}}, ins[] = {{rowptr, sizeof(int32_t) * ((size_t)n + 1)}, {colids, eb}};
        G4S_REQUIRE(!any_overlap(outs, ins), "truss, round and support must not overlap the inputs or each other");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) *info = g4s_ktruss_info{};
    if (n == 0) return G4S_OK;

    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    KtState *st, h{};
    Carver head, work;
    head.tail(&st, kStateBytes);
    Staged stage(s);
    Counts cnt;
    Graph g{};
    int *tr_out = truss, *rnd_out = round, *sup_out = support;
    int hub_cap = 0;
    int status = head.alloc();
    if (status == G4S_OK && !device) {
        g.rowptr = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        g.colids = stage.in(colids, sizeof(int) * (size_t)nnz);
        status = stage.error();
    } else {
        g.rowptr = rowptr;
        g.colids = colids;
    }
    if (status == G4S_OK) {
        // the rows first: with device pointers nnz is theirs to tell, and nothing is sized from a rowptr that was not checked
        hipError_t e = hipMemsetAsync(st, 0, kStateBytes, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kt_open_rows_kernel, dim3(grid_rows(n, cus)), dim3(WG), 0, s, n, g.rowptr, st);
            e = hipGetLastError();
        }
        cnt.launches += 1;
        if (e == hipSuccess && (device || nnz == 0)) {
            e = g4s::ReadScope(s).fetch(h, st);
            cnt.waits += 1;
            if (e == hipSuccess && !h.invalid) nnz = h.nnz;
        }
        if (e != hipSuccess) status = g4s::set_error(G4S_ERR_HIP, "g4s_ktruss: %s", hipGetErrorString(e));
    }
    const bool steps = status == G4S_OK && !h.invalid && nnz > 0;  // else: refused by its rowptr, or no stored entry — nothing to write
    if (steps) {
        const size_t eb = sizeof(int) * (size_t)nnz;
        hub_cap = (int)std::min<long long>(nnz, kHubCap);
        work.piece(&g.rank, eb + sizeof(int));
        work.piece(&g.eid, eb);
        work.piece(&g.eu, eb);
        work.piece(&g.ev, eb);
        work.piece(&g.sup, eb);
        work.piece(&g.rnd, eb);
        work.piece(&g.tr, eb);
        work.piece(&g.queue, eb);
        work.piece(&g.hubs0, sizeof(int) * (size_t)hub_cap);
        work.tail(&g.hubs1, sizeof(int) * (size_t)hub_cap);
        status = work.alloc();
        if (status == G4S_OK && !device) {
            tr_out = stage.out<int>(eb);
            if (round) rnd_out = stage.out<int>(eb);
            if (support) sup_out = stage.out<int>(eb);
            status = stage.error();
        }
        if (status == G4S_OK) status = run(n, (int)nnz, max_k, g, tr_out, rnd_out, sup_out, st, hub_cap, cus, &h, &cnt, s);
        if (status == G4S_OK && !device && !h.invalid) {
            status = stage.to_host(truss, tr_out, eb);
            if (status == G4S_OK && round) status = stage.to_host(round, rnd_out, eb);
            if (status == G4S_OK && support) status = stage.to_host(support, sup_out, eb);
            if (status == G4S_OK) status = stage.wait();
            cnt.waits += 1;
        }
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    head.idle();
    work.idle();
    if (status == G4S_OK && h.invalid) {
        const char *text = csr_invalid_text(h.invalid);
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_ktruss: %s", text ? text : "more than 524288 edges join two rows above 4096 entries");
    }
    if (status == G4S_OK && info) {
        info->triangles = (int64_t)(h.support_sum / 3);
        info->edges_walked = (int64_t)h.edges_walked;
        info->support_walked = (int64_t)h.support_walked;
        info->top_truss_edges = (int64_t)h.top_edges;
        info->max_truss = h.stop == 2 ? max_k : h.m ? h.top_level + 2 : 0;
        info->levels = h.levels;
        info->rounds = h.round;
        info->scans = h.scans;
        info->launches = cnt.launches;
        info->resumes = cnt.resumes;
        info->host_waits = cnt.waits;
        info->capped = h.stop == 2;
    }
    return status;
}
