// color.hip — g4s_color (include/g4s.h): the first-fit colouring of a simple undirected graph given as a symmetric CSR pattern, in decreasing priority
// (key[v], fmix32(v ^ seed)), by a Jones–Plassmann sweep over the priority DAG; with it round[v], the depth of v in that DAG. Colour class 0 is the
// greedy maximal independent set of the same order. DESIGN §4.16.
//
// State lives on the device (color.hpp, ClState). Per vertex: pred[v], the higher-priority neighbours not yet coloured, and mask[v], the colours below
// G4S_COLOR_MASK_COLORS held by the coloured ones. A vertex is coloured by the step behind the one that brought its pred to 0, so every vertex enters a
// frontier exactly once and ONE queue of n ints holds all frontiers one behind the other (kcore.hip's layout): [head, end) is the current frontier,
// [end, tail) the one being built. Every step is one kernel; the workgroup that finishes last (a ticket counter, no waiting) turns the page. A step
// that finds nothing to do returns at once, so the host enqueues steps blind, kBatch (doubling to kBatchMax) launches behind one read of the state;
// the first read stands behind the seed, so that the first batch's grid fits frontier 0.
//
//   open   cl_open_rows_kernel: rowptr[0] == 0, non-decreasing; pred = 0, mask = 0, deg[v] = row length (largest-first only). cl_open_ids_kernel
//          (returns at once when the rows were bad, so no entry outside [0, rowptr[n]) is read): ids in [0, n), rows strictly ascending, a stored
//          diagonal entry takes one off deg[v]; rows above kHubCut go to a hub list and through cl_open_hubs_kernel. Every later kernel begins with
//          `if (st->invalid) return`. cl_pred_kernel: one walk over all rows; an entry u → w with w != u and u above w adds one to pred[w] — the same
//          entries, under the same test, that the steps later take one off for, so the count is consistent on any pattern. cl_seed_kernel: the vertices
//          with pred == 0 are frontier 0.
//   step   the frontier walk of frontier.hpp over queue[head, end), hubs out of the hub list. Per row v: c = the lowest clear bit of mask[v]; color[v] = c,
//          round[v] = the step's index; a full mask sends v to the overflow list and c = 64 travels instead. Per entry v → w, w != v, w below v: the bit
//          of c is set in mask[w] (an atomicOr whose value nobody waits for; a plain load in front of it, to skip the atomic when the bit is there, cost
//          6 … 10 % on the R-MAT graphs of profiles/color.txt and is gone), then old = atomicSub(pred + w, 1); the one lane that sees old == 1 appends w. Page turn: the built frontier becomes the current one; stop = 1 when it is empty, 4 when it has more entries than the
//          launch grid of the batch was sized for, 5 when the overflow list has entries and no scan kernel follows the steps of this batch.
//   scan   cl_scan_kernel, behind every step once the host has read stop == 5: for every vertex the step sent to the overflow list, the colours >= 64
//          of its higher-priority neighbours are marked in an LDS bitmap of G4S_COLOR_WINDOW colours and the first clear one is taken; a full window
//          moves up by its width. One wave per vertex, the workgroup for a row above kHubCut.
// Memory model: kernel boundaries are the only ordering between workgroups. "w below v" is a comparison of priorities, a function of the inputs, so it
// cannot move while a kernel runs. Two adjacent vertices are never in one frontier, and every higher-priority neighbour of a frontier vertex was coloured
// behind an earlier kernel boundary, so mask[v] is final when the step reads it with a plain load; inside a step mask[w] is only written, by atomics, and
// the atomicSub on pred[w] alone decides who appends w. The mask carries no colour >= 64: a successor is released whether or not
// an overflowed neighbour has its colour yet, and reads that colour only in a later scan kernel. Nothing spins; every loop is bounded by the queue, a
// row length, or (the window loop) the distinct colours a row can hold.
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "color.hpp"
#include <algorithm>
#include <climits>

namespace {

using g4s::ClState;

constexpr int kBatch = G4S_COLOR_BATCH;      // step launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr int kMaskColors = G4S_COLOR_MASK_COLORS;
constexpr int kWindow = G4S_COLOR_WINDOW;
constexpr int kWindowWords = kWindow / 32;
constexpr size_t kStateBytes = 256;
static_assert(sizeof(ClState) <= kStateBytes, "state block");
static_assert(kMaskColors == 64, "mask[v] is one 64-bit word");
static_assert(kWindow % 32 == 0 && kWindowWords <= 64, "a wave reads the window's words");

enum { KIND_SEED = 0, KIND_STEP = 1 };

struct StepArgs {
    long long grid_cap;    // a frontier with more entries than this asks for a larger grid
    int n;
    int hub_cap;           // room in each hub list
    int resume;            // the first step of a batch goes on from stop == 4 or 5
    int scan_follows;      // a scan kernel is enqueued behind every step of this batch
    int expect;            // scan only: the page turns behind which it runs; a scan behind a step that returned at once returns at once too
    unsigned seed;
};

// What travels with a row's entries in the walks: the vertex, its key and (steps only) the colour it has just been given.
struct Pay {
    int u, key, c;
};

// the murmur3 finaliser: a bijection on 32 bits, so two vertices never tie
__device__ __forceinline__ unsigned fmix32(unsigned x)
{
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ int key_of(const int *__restrict__ key, int v) { return key ? key[v] : 0; }

// Is a above b in the priority order: (key, fmix32(id ^ seed)) lexicographically, larger first.
__device__ __forceinline__ bool above(int ka, int a, int kb, int b, unsigned seed)
{
    return ka != kb ? ka > kb : fmix32((unsigned)a ^ seed) > fmix32((unsigned)b ^ seed);
}

// the lowest colour < 64 that the mask leaves free, 64 when there is none
__device__ __forceinline__ int first_fit(unsigned long long m) { return m == ~0ull ? kMaskColors : __ffsll((long long)~m) - 1; }

// The end of the seed and of a step kernel: the block's shares of the sums and of the largest colour, then the ticket; the last block to arrive turns
// the page (turn_page).
__device__ __forceinline__ void finish(ClState *st, long long len_sum, long long walked, int zeros, int maxc, int kind, const StepArgs a)
{
    __shared__ long long s_len[WG / 64], s_walk[WG / 64];
    __shared__ int s_zero[WG / 64], s_max[WG / 64];
    len_sum = wave_sum(len_sum);
    walked = wave_sum(walked);
    zeros = wave_sum(zeros);
    maxc = wave_max(maxc);
    if ((threadIdx.x & 63) == 0) { s_len[threadIdx.x >> 6] = len_sum; s_walk[threadIdx.x >> 6] = walked; s_zero[threadIdx.x >> 6] = zeros; s_max[threadIdx.x >> 6] = maxc; }
    if (!turn_page(&st->tickets, [&] {
        long long ls = 0, ws = 0, zs = 0;
        int m = -1;
        for (int w = 0; w < WG / 64; ++w) { ls += s_len[w]; ws += s_walk[w]; zs += s_zero[w]; m = s_max[w] > m ? s_max[w] : m; }
        if (ls) atomicAdd((unsigned long long *)&st->edges_next, (unsigned long long)ls);
        if (ws) atomicAdd(&st->edges_walked, (unsigned long long)ws);
        if (zs) atomicAdd(&st->class0, (unsigned long long)zs);
        // the word only grows while the kernel runs, so a value read earlier is too small and costs one atomic; read at agent scope, past the copy of
        // the state line this CU has held since the kernel's first lines
        if (m > __hip_atomic_load(&st->max_color, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st->max_color, m);
    })) return;
    const int ot = atomicAdd(&st->over_tail, 0);
    const QueueFlip f = flip_queue(st);                            // what this kernel appended, what it coloured
    const int pending = ot - st->over_end;                         // what this kernel sent to the overflow list
    st->over_head = st->over_end; st->over_end = ot;
    st->turns += 1;
    if (kind == KIND_STEP && f.walked > 0) st->round += 1;
    // 5 before 1: the last frontier's overflow still wants its scan, and the step that resumes behind it finds an empty frontier and ends the call
    st->stop = pending > 0 && !a.scan_follows ? 5 : f.appended == 0 ? 1 : f.entries > a.grid_cap ? 4 : 0;
}

__global__ __launch_bounds__(WG) void cl_open_rows_kernel(int n, const int *__restrict__ rowptr, int *__restrict__ pred, unsigned long long *__restrict__ mask,
                                                          int *__restrict__ deg, ClState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [&](long long i, int rb, int re) {
        pred[i] = 0;
        mask[i] = 0ull;
        if (deg) deg[i] = re - rb;
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) st->max_color = -1;
}

// The column ids (open_ids / open_hubs, strictly ascending rows); the diagonal does not count in the degree, where the call keeps one.
__global__ __launch_bounds__(WG) void cl_open_ids_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *deg,
                                                         int *__restrict__ hubs, ClState *st)
{
    if (st->invalid) return;                                       // rowptr is monotone from 0 beyond this line: [0, rowptr[n]) is the colids array
    open_ids<true>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_cur, &st->invalid, 2, [&](int, int u, int v) { if (v == u && deg) atomicSub(deg + u, 1); });
}

__global__ __launch_bounds__(WG) void cl_open_hubs_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *deg,
                                                          const int *__restrict__ hubs, ClState *st)
{
    if (st->invalid) return;
    open_hubs<true>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_cur, &st->invalid, 2, [&](int, int u, int v) { if (v == u && deg) atomicSub(deg + u, 1); });
}

// pred[w] = the stored entries u → w, u != w, with u above w: on a symmetric pattern the higher-priority neighbours of w. The hub list is the opening
// pass's: every row above kHubCut.
__global__ __launch_bounds__(WG) void cl_pred_kernel(int n, int hub_cap, unsigned seed, const int *__restrict__ rowptr, const int *__restrict__ colids,
                                                     const int *__restrict__ key, int *pred, const int *__restrict__ hubs, const ClState *st)
{
    if (st->invalid) return;
    auto entry = [&](bool valid, int k, Pay p) {
        if (!valid) return;
        const int w = colids[k];
        if (w != p.u && above(p.key, p.u, key_of(key, w), w, seed)) atomicAdd(pred + w, 1);
    };
    walk_tiles<Pay>(n, [&](int i, int &start, int &len, Pay &p) {
        const int rb = rowptr[i], l = rowptr[i + 1] - rb;
        if (l > kHubCut) return;
        p.u = i;
        p.key = key_of(key, i);
        start = rb;
        len = l;
    }, entry);
    walk_hubs<Pay>(st->n_hub_cur < hub_cap ? st->n_hub_cur : hub_cap, [&](int h, int &start, int &len, Pay &p) {
        p.u = hubs[h];
        p.key = key_of(key, p.u);
        start = rowptr[p.u];
        len = rowptr[p.u + 1] - start;
    }, entry);
}

// Frontier 0: the vertices no neighbour is above. Its page turn is a step's, without a round.
__global__ __launch_bounds__(WG) void cl_seed_kernel(const int *__restrict__ rowptr, const int *__restrict__ pred, int *__restrict__ queue, int *hubs0, int *hubs1,
                                                     ClState *st, const StepArgs a)
{
    if (st->invalid) return;
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0;
    for (long long i0 = (long long)blockIdx.x * WG; i0 < a.n; i0 += (long long)gridDim.x * WG) {
        const long long i = i0 + threadIdx.x;
        const bool want = i < a.n && pred[i] == 0;
        const int len = want ? rowptr[i + 1] - rowptr[i] : 0;
        append_frontier(want, (int)i, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);   // appended once per call: the slot is below n
    }
    finish(st, len_sum, 0, 0, -1, KIND_SEED, a);
}

__global__ __launch_bounds__(WG) void cl_step_kernel(const int *__restrict__ rowptr, const int *__restrict__ colids, const int *__restrict__ key, int *pred,
                                                     unsigned long long *mask, int *color, int *round, int *queue, int *over, int *hubs0, int *hubs1,
                                                     ClState *st, const StepArgs a)
{
    if (st->invalid || !(st->stop == 0 || ((st->stop == 4 || st->stop == 5) && a.resume))) return;   // the same words for every block
    const int r = st->round, head = st->head;
    const int *hubs_cur = st->hub_cur ? hubs1 : hubs0;
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0, walked = 0;
    int zeros = 0, maxc = -1;
    auto entry = [&](bool valid, int k, Pay p) {
        bool want = false;
        int w = 0, len = 0;
        if (valid) {
            w = colids[k];
            if (w != p.u) {
                walked += 1;
                if (above(p.key, p.u, key_of(key, w), w, a.seed)) {
                    const unsigned long long bit = 1ull << (p.c & 63);
                    if (p.c < kMaskColors) atomicOr(mask + w, bit);            // no value comes back: the lane does not wait for it
                    want = atomicSub(pred + w, 1) == 1;
                    if (want) len = rowptr[w + 1] - rowptr[w];
                }
            }
        }
        append_frontier(want, w, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);
    };
    walk_tiles<Pay>(st->end - head, [&](int i, int &start, int &len, Pay &p) {
        const int v = queue[head + i];
        const int c = first_fit(mask[v]);                          // every neighbour above v was coloured behind an earlier kernel boundary
        if (c < kMaskColors) {
            color[v] = c;
            zeros += c == 0;
            maxc = c > maxc ? c : maxc;
        } else {
            const int o = atomicAdd(&st->over_tail, 1);            // rare: the scan gives v its colour
            if ((unsigned)o < (unsigned)a.n) over[o] = v;
        }
        if (round) round[v] = r;
        const int rb = rowptr[v], l = rowptr[v + 1] - rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        p.u = v;
        p.key = key_of(key, v);
        p.c = c;
        start = rb;
        len = l;
    }, entry);
    walk_hubs<Pay>(st->n_hub_cur < a.hub_cap ? st->n_hub_cur : a.hub_cap, [&](int h, int &start, int &len, Pay &p) {
        p.u = hubs_cur[h];
        p.key = key_of(key, p.u);
        p.c = first_fit(mask[p.u]);                                // the colour another workgroup is writing: the same function of the same word
        start = rowptr[p.u];
        len = rowptr[p.u + 1] - start;
    }, entry);
    finish(st, len_sum, walked, zeros, maxc, KIND_STEP, a);
}

// The colours >= 64 of v's higher-priority neighbours, window by window, by `width` threads of which this is thread `t`; bm: the unit's kWindowWords
// words. Called by every thread of the workgroup (the barriers), `active` false for a unit without a vertex. The first colour not held, for an active
// unit. A full window holds kWindow distinct colours of the row, so the loop ends after at most row length / kWindow + 1 passes.
__device__ __forceinline__ int scan_row(bool active, int v, int t, int width, unsigned *bm, const int *__restrict__ rowptr, const int *__restrict__ colids,
                                        const int *__restrict__ key, const int *color, unsigned seed)
{
    const int rb = active ? rowptr[v] : 0, re = active ? rowptr[v + 1] : 0, kv = active ? key_of(key, v) : 0;
    int base = kMaskColors, c = -1;
    bool done = !active;
    for (;;) {
        if (t < kWindowWords) bm[t] = 0u;
        __syncthreads();
        if (!done)
            for (int k = rb + t; k < re; k += width) {
                const int w = colids[k];
                if (w == v || !above(key_of(key, w), w, kv, v, seed)) continue;
                const int cw = color[w] - base;                    // final: written behind an earlier kernel boundary
                if ((unsigned)cw < (unsigned)kWindow) atomicOr(bm + (cw >> 5), 1u << (cw & 31));
            }
        __syncthreads();
        if (!done) {
            int found = -1;
            for (int j = kWindowWords - 1; j >= 0; --j) {
                const unsigned x = ~bm[j];
                if (x) found = j * 32 + __ffs((int)x) - 1;
            }
            if (found >= 0) { c = base + found; done = true; }
            else base += kWindow;
        }
        if (!__syncthreads_or(!done)) break;                       // also: nobody clears the words while another thread still reads them
    }
    return c;
}

__global__ __launch_bounds__(WG) void cl_scan_kernel(const int *__restrict__ rowptr, const int *__restrict__ colids, const int *__restrict__ key, int *color,
                                                     const int *__restrict__ over, ClState *st, const StepArgs a)
{
    __shared__ unsigned s_bm[WG / 64][kWindowWords];
    if (st->invalid || st->turns != a.expect) return;
    const int lo = st->over_head, hi = st->over_end < a.n ? st->over_end : a.n;   // changed only by a step's page turn
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long i0 = lo + (long long)blockIdx.x * (WG / 64); i0 < hi; i0 += (long long)gridDim.x * (WG / 64)) {   // one wave per ordinary row
        const bool have = i0 + wave < hi;
        const int v = have ? over[i0 + wave] : 0;
        const bool active = have && rowptr[v + 1] - rowptr[v] <= kHubCut;
        const int c = scan_row(active, v, lane, 64, s_bm[wave], rowptr, colids, key, color, a.seed);
        if (active && lane == 0) {
            color[v] = c;
            atomicMax(&st->max_color, c);
        }
    }
    for (long long i = lo + (long long)blockIdx.x; i < hi; i += gridDim.x) {                                          // the workgroup per hub row
        const int v = over[i];
        if (rowptr[v + 1] - rowptr[v] <= kHubCut) continue;
        const int c = scan_row(true, v, t, WG, s_bm[0], rowptr, colids, key, color, a.seed);
        if (t == 0) {
            color[v] = c;
            atomicMax(&st->max_color, c);
        }
    }
}

struct ColorCounts : Counts {
    int scan_resumes = 0;
};

struct Work {
    ClState *st;
    int *pred, *queue, *over, *deg, *hubs[2];
    unsigned long long *mask;
};

// The whole colouring on device arrays; returns behind a wait on `s` with *h the final state.
int run(int n, const int *rowptr, const int *colids, const int *key, unsigned seed, int *color, int *round, const Work &w, int hub_cap, int cus, ClState *h,
        ColorCounts *cnt, hipStream_t s)
{
    // G4S_COLOR_MIN_GRID is an A/B switch: the outputs do not depend on it.
    const g4s::StepGrid sized(env_int("G4S_COLOR_MIN_GRID", g4s::kMinGrid, 1, 2 * cus), 2 * cus);
    const int g_rows = grid_rows(n, cus), g_walk = grid_for<WG>(n, 2048);
    StepArgs a;
    a.grid_cap = LLONG_MAX;                                        // the seed stops nothing: the first grid is sized behind it
    a.n = n;
    a.hub_cap = hub_cap;
    a.resume = 0;
    a.scan_follows = 0;
    a.expect = 0;
    a.seed = seed;
    G4S_HIP_TRY(hipMemsetAsync(w.st, 0, kStateBytes, s));
    hipLaunchKernelGGL(cl_open_rows_kernel, dim3(g_rows), dim3(WG), 0, s, n, rowptr, w.pred, w.mask, w.deg, w.st);
    hipLaunchKernelGGL(cl_open_ids_kernel, dim3(g_walk), dim3(WG), 0, s, n, hub_cap, rowptr, colids, w.deg, w.hubs[0], w.st);
    hipLaunchKernelGGL(cl_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, hub_cap, rowptr, colids, w.deg, w.hubs[0], w.st);
    hipLaunchKernelGGL(cl_pred_kernel, dim3(g_walk), dim3(WG), 0, s, n, hub_cap, seed, rowptr, colids, key, w.pred, w.hubs[0], w.st);
    hipLaunchKernelGGL(cl_seed_kernel, dim3(g_rows), dim3(WG), 0, s, rowptr, w.pred, w.queue, w.hubs[0], w.hubs[1], w.st, a);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 5;

    // One read behind the seed: frontier 0 under a hash order is a fixed share of all vertices, under an explicit order it may be one vertex, and the
    // first batch's grid is sized for what is there. A bad pattern ends here.
    g4s::ReadScope reads(s);
    G4S_HIP_TRY(reads.fetch(*h, w.st));
    cnt->waits += 1;
    bool scans = false;                                            // a scan follows every step
    int batch = kBatch;
    while (!h->invalid && h->stop != 1) {
        const int grid = sized.grid(h->edges_cur + (h->end - h->head) + h->n_hub_cur);
        const bool resumed = h->stop == 4 || h->stop == 5;
        a.grid_cap = sized.cap(grid);
        if (h->stop == 5) {                                        // the overflow of the step that stopped the last batch
            scans = true;
            a.expect = h->turns;
            hipLaunchKernelGGL(cl_scan_kernel, dim3(cus), dim3(WG), 0, s, rowptr, colids, key, color, w.over, w.st, a);
            cnt->launches += 1;
            cnt->scan_resumes += 1;
        } else if (resumed) {
            cnt->resumes += 1;
        }
        a.scan_follows = scans;
        for (int b = 0; b < batch; ++b) {
            a.resume = b == 0 && resumed;
            hipLaunchKernelGGL(cl_step_kernel, dim3(grid), dim3(WG), 0, s, rowptr, colids, key, w.pred, w.mask, color, round, w.queue, w.over, w.hubs[0],
                               w.hubs[1], w.st, a);
            a.expect = h->turns + b + 1;
            if (scans) hipLaunchKernelGGL(cl_scan_kernel, dim3(cus), dim3(WG), 0, s, rowptr, colids, key, color, w.over, w.st, a);
        }
        a.resume = 0;
        G4S_HIP_TRY(hipGetLastError());
        cnt->launches += scans ? 2 * batch : batch;
        G4S_HIP_TRY(reads.fetch(*h, w.st));
        cnt->waits += 1;
        batch = sized.next_batch(batch);
    }
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_color(int32_t n, const int32_t *rowptr, const int32_t *colids, const int32_t *key, uint32_t seed, int32_t *color, int32_t *round,
                             unsigned flags, g4s_color_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_DEVICE_POINTERS | G4S_COLOR_LARGEST_FIRST)) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and G4S_COLOR_LARGEST_FIRST");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr && color, "rowptr or color is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0, largest = (flags & G4S_COLOR_LARGEST_FIRST) != 0;
    G4S_REQUIRE(!(largest && key), "key must be NULL with G4S_COLOR_LARGEST_FIRST");
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        const size_t nb = sizeof(int32_t) * (size_t)n;
        const Span outs[] = {{color, nb}, {round, nb}}, ins[] = {{rowptr, nb + sizeof(int32_t)}, {colids, sizeof(int32_t) * (size_t)nnz}, {key, nb}};
        G4S_REQUIRE(!any_overlap(outs, ins), "color and round must not overlap the inputs or each other");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) *info = g4s_color_info{};
    if (n == 0) return G4S_OK;

    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const int hub_cap = std::min(n, kHubCap);
    ClState h{};
    Work w{};
    Carver work;
    work.piece(&w.st, kStateBytes);
    work.piece(&w.mask, sizeof(unsigned long long) * (size_t)n);
    work.piece(&w.pred, sizeof(int) * (size_t)n);
    work.piece(&w.queue, sizeof(int) * (size_t)n);
    work.piece(&w.over, sizeof(int) * (size_t)n);
    if (largest) work.piece(&w.deg, sizeof(int) * (size_t)n);
    work.piece(&w.hubs[0], sizeof(int) * (size_t)hub_cap);
    work.tail(&w.hubs[1], sizeof(int) * (size_t)hub_cap);
    Staged stage(s);
    ColorCounts cnt;
    int status = work.alloc();
    const int *rp = rowptr, *ci = colids, *ke = key;
    int *co = color, *ro = round;
    if (status == G4S_OK && !device) {
        rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        ci = stage.in(colids, sizeof(int) * (size_t)nnz);
        ke = stage.in(key, sizeof(int) * (size_t)n);
        co = stage.out<int>(sizeof(int) * (size_t)n);
        if (round) ro = stage.out<int>(sizeof(int) * (size_t)n);
        status = stage.error();
    }
    if (largest) ke = w.deg;                                       // the key is the degree without the diagonal, complete behind the opening pass
    if (status == G4S_OK) status = run(n, rp, ci, ke, seed, co, ro, w, hub_cap, cus, &h, &cnt, s);
    if (status == G4S_OK && !device && !h.invalid) {
        status = stage.to_host(color, co, sizeof(int) * (size_t)n);
        if (status == G4S_OK && round) status = stage.to_host(round, ro, sizeof(int) * (size_t)n);
        if (status == G4S_OK) status = stage.wait();
        cnt.waits += 1;
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    work.idle();
    if (status == G4S_OK && h.invalid)
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_color: %s", csr_invalid_text(h.invalid));
    if (status == G4S_OK && info) {
        info->edges_walked = (int64_t)h.edges_walked;
        info->class0 = (int64_t)h.class0;
        info->colors = h.max_color + 1;
        info->rounds = h.round;
        info->overflow = h.over_tail;
        info->launches = cnt.launches;
        info->resumes = cnt.resumes;
        info->scan_resumes = cnt.scan_resumes;
        info->host_waits = cnt.waits;
    }
    return status;
}
