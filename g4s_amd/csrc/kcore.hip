// kcore.hip — g4s_kcore (include/g4s.h): the core numbers of a simple undirected graph given as a symmetric CSR pattern, by synchronous peeling, and
// with them the peel order (round[v]: which frontier removed v), which sorted by (round, id) is a degeneracy ordering. DESIGN §4.15.
//
// State lives on the device (kcore.hpp, KcState). The graph is peeled level by level (k = the smallest remaining degree) and inside a level frontier
// by frontier; every vertex enters a frontier exactly once per call, so ONE queue of n ints holds all frontiers one behind the other (the `order` layout
// of betweenness.hip): [head, end) is the current frontier, [end, tail) the one being built. Every step is one kernel; the workgroup that finishes last
// (a ticket counter, no waiting) turns the page. A step kernel that finds nothing to do returns at once, so the host enqueues scans and peels blind,
// kBatch (doubling to kBatchMax) launches behind one read of the 104-byte state, as traverse.hip does.
//
//   open   kc_open_rows_kernel: rowptr[0] == 0, non-decreasing; deg[v] = row length, core[v] = round[v] = −1. kc_open_ids_kernel (returns at once when
//          the rows were bad, so no entry outside [0, rowptr[n]) is read): ids in [0, n), rows strictly ascending, a stored diagonal entry takes one off
//          deg[v]; rows above kHubCut go to a hub list and through kc_open_hubs_kernel. Every later kernel begins with `if (st->invalid) return`.
//   scan   runs when the frontier is empty: every unremoved vertex with deg <= k joins the frontier (core = k, round = the coming round); the others
//          contribute to a minimum, at most one atomicMin per workgroup. Four vertices a thread and trip, at most one workgroup per CU. Page turn:
//          nothing collected → k := that minimum (the level jump; the next scan then collects at least one vertex), and stop = 2 when k >= max_k.
//   peel   runs when the frontier is not empty: the frontier walk of frontier.hpp over queue[head, end), hubs out of the hub list. Per entry u → v:
//          skip v == u; a plain load of deg[v], skip when it is <= k; old = atomicSub(deg + v, 1); the one lane that sees old == k + 1 appends v.
//          Page turn: the built frontier becomes the current one; stop = 1 when it is empty and every vertex has been removed, 4 when it has more
//          entries than the launch grid of the batch was sized for (the host resumes on a larger grid).
//   finish kc_finish_kernel, behind every batch, a no-op until stop is 1 or 2: the vertices left by max_k get core = max_k; counts the top core.
// Memory model: kernel boundaries are the only ordering between workgroups. Inside a peel the plain load of deg[v] may be stale; degrees only decrease,
// so a stale value is only ever too large, the lane then goes to the atomic, and the atomic alone decides who appends (the SSSP argument of DESIGN §4.6).
// A vertex whose degree has fallen to k or below is never appended again: later atomics on it return at most k. core[v] and round[v] are written by the
// one appending lane and read only behind a kernel boundary. Nothing spins; every loop is bounded by the queue or a row length.
#include "common.hpp"
#include "level_peel.hpp"
#include "kcore.hpp"
#include <algorithm>
#include <climits>

namespace {

using g4s::KcState;

constexpr int kBatch = G4S_KCORE_BATCH;      // step launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr int kScanUnroll = 4;                // vertices per thread and trip of a scan
constexpr size_t kStateBytes = 256;
static_assert(sizeof(KcState) <= kStateBytes, "state block");

struct StepArgs {
    long long grid_cap;    // a frontier with more entries than this asks for a larger peel grid
    int n;
    int max_k;
    int hub_cap;           // room in each hub list
    int resume;            // peel only: the first launch of a batch goes on from stop == 4
};

__global__ __launch_bounds__(WG) void kc_open_rows_kernel(int n, int max_k, const int *__restrict__ rowptr, int *__restrict__ deg, int *__restrict__ core,
                                                          int *__restrict__ round, KcState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [&](long long i, int rb, int re) {
        deg[i] = re - rb;
        core[i] = -1;
        if (round) round[i] = -1;
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->min_left = INT_MAX;
        if (max_k == 0) st->stop = 2;                              // no level is below the cap: every vertex is left
    }
}

// The column ids (open_ids / open_hubs, strictly ascending rows); the diagonal does not count in the degree.
__global__ __launch_bounds__(WG) void kc_open_ids_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *deg,
                                                         int *__restrict__ hubs, KcState *st)
{
    if (st->invalid) return;                                       // rowptr is monotone from 0 beyond this line: [0, rowptr[n]) is the colids array
    open_ids<true>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_cur, &st->invalid, 2, [&](int, int u, int v) { if (v == u) atomicSub(deg + u, 1); });
}

__global__ __launch_bounds__(WG) void kc_open_hubs_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *deg,
                                                          const int *__restrict__ hubs, KcState *st)
{
    if (st->invalid) return;
    open_hubs<true>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_cur, &st->invalid, 2, [&](int, int u, int v) { if (v == u) atomicSub(deg + u, 1); });
}

__global__ __launch_bounds__(WG) void kc_scan_kernel(const int *__restrict__ rowptr, const int *__restrict__ deg, int *__restrict__ core, int *__restrict__ round,
                                                     int *__restrict__ queue, int *hubs0, int *hubs1, KcState *st, const StepArgs a)
{
    if (st->invalid || st->stop != 0 || st->end != st->head) return;   // the same words for every block: they change only after the last ticket
    const int kk = st->level, r = st->round;
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0;
    int mn = INT_MAX;
    for (long long i0 = (long long)blockIdx.x * (WG * kScanUnroll); i0 < a.n; i0 += (long long)gridDim.x * (WG * kScanUnroll)) {
        int c[kScanUnroll], d[kScanUnroll];
#pragma unroll
        for (int j = 0; j < kScanUnroll; ++j) {                    // the loads of a trip first: they do not depend on each other
            const long long i = i0 + j * WG + threadIdx.x;
            c[j] = i < a.n ? core[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kScanUnroll; ++j) {
            const long long i = i0 + j * WG + threadIdx.x;
            d[j] = c[j] == -1 ? deg[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kScanUnroll; ++j) {
            const long long i = i0 + j * WG + threadIdx.x;
            const bool want = c[j] == -1 && d[j] <= kk;
            int len = 0;
            if (want) {
                core[i] = kk;
                if (round) round[i] = r;
                len = rowptr[i + 1] - rowptr[i];
            } else if (c[j] == -1) {
                mn = d[j] < mn ? d[j] : mn;
            }
            append_frontier(want, (int)i, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);   // appended once per call: the slot is below n
        }
    }
    finish_step(st, len_sum, 0, mn, KIND_SCAN, a.grid_cap, a.max_k, [&] { return a.n; });
}

__global__ __launch_bounds__(WG) void kc_peel_kernel(const int *__restrict__ rowptr, const int *__restrict__ colids, int *deg, int *core, int *round, int *queue,
                                                     int *hubs0, int *hubs1, KcState *st, const StepArgs a)
{
    if (st->invalid || st->end == st->head || !step_runs(st->stop, a.resume)) return;
    const int kk = st->level, r = st->round + 1, head = st->head;
    const int *hubs_cur = st->hub_cur ? hubs1 : hubs0;
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0, walked = 0;
    auto entry = [&](bool valid, int k, int u) {
        bool want = false;
        int v = 0, len = 0;
        if (valid) {
            v = colids[k];
            if (v != u) {
                walked += 1;
                if (ld(deg + v) > kk) {                            // a stale read is only ever too large: the atomic below decides
                    want = atomicSub(deg + v, 1) == kk + 1;
                    if (want) {
                        core[v] = kk;
                        if (round) round[v] = r;
                        len = rowptr[v + 1] - rowptr[v];
                    }
                }
            }
        }
        append_frontier(want, v, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);
    };
    walk_tiles<int>(st->end - head, [&](int i, int &start, int &len, int &u) {
        u = queue[head + i];
        const int rb = rowptr[u], l = rowptr[u + 1] - rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        start = rb;
        len = l;
    }, entry);
    walk_hubs<int>(st->n_hub_cur < a.hub_cap ? st->n_hub_cur : a.hub_cap, [&](int h, int &start, int &len, int &u) {
        u = hubs_cur[h];
        start = rowptr[u];
        len = rowptr[u + 1] - start;
    }, entry);
    finish_step(st, len_sum, walked, INT_MAX, KIND_PEEL, a.grid_cap, a.max_k, [&] { return a.n; });
}

// Once the peeling has ended (stop 1 or 2; a no-op before): what max_k left gets core = max_k, and the vertices of the top core are counted.
__global__ __launch_bounds__(WG) void kc_finish_kernel(int n, int max_k, int *__restrict__ core, KcState *st)
{
    __shared__ int s_red[WG / 64];
    if (st->invalid || (st->stop != 1 && st->stop != 2)) return;
    const int top = st->stop == 2 ? max_k : st->top_level;
    int c = 0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        int x = core[i];
        if (x == -1) core[i] = x = max_k;
        c += x == top;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_red[w];
        if (sum) atomicAdd(&st->top_core, (unsigned long long)sum);
    }
}

// The whole decomposition on device arrays; returns behind a wait on `s` with *h the final state. `st` has room for kStateBytes, `deg` and `queue` for
// n ints, hubs[0] and hubs[1] for hub_cap ints each.
int run(int n, const int *rowptr, const int *colids, int max_k, int *core, int *round, KcState *st, int *deg, int *queue, int *const hubs[2], int hub_cap, int cus,
        KcState *h, Counts *cnt, hipStream_t s)
{
    // a scan ends in one ticket per workgroup on one word, so its grid is kept small: kScanUnroll vertices a thread and trip, at most one workgroup
    // per CU (the sweep in profiles/kcore.txt). G4S_KCORE_SCAN_WGS and G4S_KCORE_MIN_GRID are A/B switches: the outputs do not depend on them.
    const g4s::StepGrid sized(env_int("G4S_KCORE_MIN_GRID", g4s::kMinGrid, 1, 2 * cus), 2 * cus);   // the peel grid of a batch: between 8 workgroups and two per CU
    const int g_rows = grid_rows(n, cus), g_scan = grid_for<WG * kScanUnroll>(n, env_int("G4S_KCORE_SCAN_WGS", cus, 1, 8 * cus));
    StepArgs a;
    a.grid_cap = LLONG_MAX;
    a.n = n;
    a.max_k = max_k;
    a.hub_cap = hub_cap;
    a.resume = 0;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, kStateBytes, s));
    hipLaunchKernelGGL(kc_open_rows_kernel, dim3(g_rows), dim3(WG), 0, s, n, max_k, rowptr, deg, core, round, st);
    hipLaunchKernelGGL(kc_open_ids_kernel, dim3(grid_for<WG>(n, 2048)), dim3(WG), 0, s, n, hub_cap, rowptr, colids, deg, hubs[0], st);
    hipLaunchKernelGGL(kc_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, hub_cap, rowptr, colids, deg, hubs[0], st);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 3;

    g4s::ReadScope reads(s);
    return run_level_peel(sized, kBatch, 1, [&](long long grid_cap) {
        a.grid_cap = grid_cap;
        hipLaunchKernelGGL(kc_scan_kernel, dim3(g_scan), dim3(WG), 0, s, rowptr, deg, core, round, queue, hubs[0], hubs[1], st, a);
    }, [&](int grid, long long grid_cap, int resume) {
        a.grid_cap = grid_cap;
        a.resume = resume;
        hipLaunchKernelGGL(kc_peel_kernel, dim3(grid), dim3(WG), 0, s, rowptr, colids, deg, core, round, queue, hubs[0], hubs[1], st, a);
        a.resume = 0;
    }, [&] { hipLaunchKernelGGL(kc_finish_kernel, dim3(g_rows), dim3(WG), 0, s, n, max_k, core, st); }, reads, st, h, cnt);
}

} // namespace

G4S_API g4s_status g4s_kcore(int32_t n, const int32_t *rowptr, const int32_t *colids, int32_t max_k, int32_t *core, int32_t *round, unsigned flags,
                             g4s_kcore_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(max_k >= 0, "negative max_k");
    G4S_REQUIRE(rowptr && core, "rowptr or core is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        const size_t nb = sizeof(int32_t) * (size_t)n;
        const Span outs[] = {{core, nb}, {round, nb}}, ins[] = {{rowptr, nb + sizeof(int32_t)}, {colids, sizeof(int32_t) * (size_t)nnz}};
        G4S_REQUIRE(!any_overlap(outs, ins), "core and round must not overlap the inputs or each other");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) *info = g4s_kcore_info{};
    if (n == 0) return G4S_OK;

    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const int hub_cap = std::min(n, kHubCap);
    KcState *st, h{};
    int *deg, *queue, *hubs[2];
    Carver work;
    work.piece(&st, kStateBytes);
    work.piece(&deg, sizeof(int) * (size_t)n);
    work.piece(&queue, sizeof(int) * (size_t)n);
    work.piece(&hubs[0], sizeof(int) * (size_t)hub_cap);
    work.tail(&hubs[1], sizeof(int) * (size_t)hub_cap);
    Staged stage(s);
    Counts cnt;
    int status = work.alloc();
    const int *rp = rowptr, *ci = colids;
    int *co = core, *ro = round;
    if (status == G4S_OK && !device) {
        rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        ci = stage.in(colids, sizeof(int) * (size_t)nnz);
        co = stage.out<int>(sizeof(int) * (size_t)n);
        if (round) ro = stage.out<int>(sizeof(int) * (size_t)n);
        status = stage.error();
    }
    if (status == G4S_OK) status = run(n, rp, ci, max_k, co, ro, st, deg, queue, hubs, hub_cap, cus, &h, &cnt, s);
    if (status == G4S_OK && !device && !h.invalid) {
        status = stage.to_host(core, co, sizeof(int) * (size_t)n);
        if (status == G4S_OK && round) status = stage.to_host(round, ro, sizeof(int) * (size_t)n);
        if (status == G4S_OK) status = stage.wait();
        cnt.waits += 1;
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    work.idle();
    if (status == G4S_OK && h.invalid)
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_kcore: %s", csr_invalid_text(h.invalid));
    if (status == G4S_OK && info) {
        info->edges_walked = (int64_t)h.edges_walked;
        info->top_core_size = (int64_t)h.top_core;
        info->degeneracy = h.stop == 2 ? max_k : h.top_level;
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
