// msf.hip — g4s_minimum_spanning_forest (include/g4s.h): the minimum (or maximum) spanning forest of the undirected weighted graph whose edges are the
// stored off-diagonal entries of an n × n CSR, as the ascending positions of the forest's entries, with the canonical component labels. Borůvka rounds on
// the union-find forest of components.hip (union_find.hpp), on the frontier walk with hubs (frontier.hpp). DESIGN §4.19.
//
// Order. Entry k = (i, j, w) has the key (w', min(i,j), max(i,j), k), w' = w (−w under G4S_MSF_MAXIMUM) with −0.0 made +0.0, compared as a double: a strict
// total order on entries, so the forest is unique — the one Kruskal builds scanning the entries in that order — and no schedule can change it.
//
//   open    ms_open_rows_kernel (rowptr[0] == 0, non-decreasing; parent[v] = v, the key words at NONE, every non-empty row into the live list, long ones
//           into its hub list), ms_open_ids_kernel / ms_open_hubs_kernel (ids in [0, n)), ms_open_values_kernel (no NaN), ms_begin_kernel (the first page).
//           Every later kernel begins with `if (st->invalid) return`: no id is an index before it has been checked.
//   round   FIND, in stages because the key is wider than an atomic: the live rows are walked once per stage; an entry whose ends have the same root is
//           dropped behind one 4-byte gather (parent[] is flat here, see below), every other one is OUTGOING for both roots and offers
//             stage 0  the order-preserving 64-bit image of w' to key_w[root]      (atomicMin; skipped when values == NULL)
//             stage 1  (lo << 32) | hi to key_p[root], if its image is key_w[root]
//             stage 2  k to key_k[root], if its pair is key_p[root] too.
//           A wave whose offering lanes share the root (a row's own root: lanes of a wave walk consecutive entries) reduces first and sends one atomic;
//           every atomic sits behind a load of the word that skips it when it cannot lower the word (a stale word is too large: it only lets an atomic
//           through). The first stage also stamps the rows that saw an outgoing entry.
//           PICK    one thread per root with a key: the forest list gets k by one atomicAdd per wave, unless the other end's root chose the same k
//                   and is smaller (two roots choose the same entry only mutually). Nothing writes parent[] here, so both roots are exact.
//           LINK    the same threads: the key words go back to NONE and link_from joins the two ends. Under a strict total order the chosen entries are
//                   acyclic over the components, so every hook is a tree edge; the smaller id wins every hook, so the root is the canonical label.
//           JUMP    kJumpPasses passes of pointer jumping; a pass that has nothing left returns at once. Behind them parent[v] is v's root for every v.
//           TURN    the stamped rows of the live list make the next one (a row without an outgoing entry never gets one again: components only grow);
//                   the last workgroup (turn_page) swaps the lists. No root with a key, or no live row: stop = 1.
//   close   the list of positions is sorted ascending with the radix sort of prims.hpp, and the weights are summed in ascending position order in a
//           shape that depends on the number of edges alone: tiles of 2048 (8 consecutive per lane, the shuffle ladder, four waves left to right), then
//           the tile sums the same way in one workgroup. The same bits on every run.
// Rounds: a root with an outgoing entry is hooked to, or hooks, another one, so the components that still have outgoing entries at least halve:
// rounds <= ceil(log2 n) + 1 (the last one may find nothing).
// Memory model: parent[] is written by LINK and JUMP only, and there is a kernel boundary between them and every reader, so FIND, PICK and
// TURN read exact roots. Inside LINK the loads may be stale; union_find.hpp says why that is sound. Were a root read in FIND ever stale, it would be a
// former ancestor: an internal entry could look outgoing, never the reverse; PICK therefore checks the winner's ends again and drops an internal one.
// Driver: the host enqueues whole rounds blind, at least kBatch launches behind one read of the state, doubling up to kBatchMax (step_batch.hpp); every
// kernel returns at once when the stop word is set. host_waits <= launches / 16 + 3.
// Environment: G4S_MSF_FIRST_GRID (the grid of the first batch; default 0: sized from rowptr[n] with host pointers, the largest grid with
// device pointers), G4S_MSF_WAVE_MIN (default 1; 0: no reduction across the wave in front of the atomics). The outputs do not depend on either.
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "union_find.hpp"
#include "prims.hpp"
#include <algorithm>
#include <climits>

namespace {

using namespace g4s;

typedef unsigned long long u64;

constexpr int kBatch = G4S_MSF_BATCH;        // launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr size_t kStateBytes = 256;
constexpr u64 kNone64 = ~0ull;               // above the image of +inf (0xfff0…) and above every pair of ids
constexpr int kNone = INT_MAX;               // above every position: nnz <= INT_MAX means k < INT_MAX
constexpr int kSumTile = 2048;               // weights per tile of the sum: 8 consecutive per lane of a workgroup

struct MsState {
    u64 entries_walked;              // stored entries walked by the find stages
    long long work_cur;              // entries of the live rows: what the launch grid is sized from
    long long work_next;             // of the live list being built
    double weight;
    int invalid;                     // 1 rowptr, 2 an id out of range, 8 a NaN among the values
    int stop;                        // 0 go on; 1 the forest is complete; 4 the live rows outgrew the launch grid
    int tickets;                     // workgroups of the running turn kernel that have finished
    int round;                       // rounds run
    int cur;                         // which live list (and hub list) is the current one
    int live_n, live_next;           // rows in the current list, in the one being built
    int n_hub_cur, n_hub_next;       // the hubs among them
    int open_hubs;                   // hubs found by the check of the ids
    int found;                       // some root has a key in this round
    int n_edges;                     // positions in the forest list
    int nnz;                         // rowptr[n]
    int pending[kJumpPasses + 1];    // pending[p]: pass p of this round's compression has work
};
static_assert(sizeof(MsState) <= kStateBytes, "state block");

struct StepArgs {
    long long grid_cap;    // live rows with more entries than this ask for a larger grid
    int n;
    int hub_cap;           // room in each hub list
    int resume;            // the first launch of a batch goes on from stop == 4
    int first;             // the first find stage of a round: it stamps the rows and may resume
    int wave_min;          // reduce across the wave in front of the atomics
};

struct Arrays {
    const int *rp, *ci;
    const double *val;     // NULL: all weights equal
    int *parent;           // the union-find forest: the caller's labels, or scratch
    u64 *key_w, *key_p;    // per root: the smallest weight image, the smallest pair among the entries that have it
    int *key_k;            // the smallest position among the entries that have both
    int *stamp;            // the last round in which the row saw an outgoing entry
    int *live[2], *hubs[2];
    int *flist;            // the forest's positions, in the order they were chosen
    int maximum;
};

struct RowPay {
    int u, ru;             // the row and its root
};

template <typename K> __device__ __forceinline__ K ldk(const K *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// The order-preserving 64-bit image of a weight: a < b as doubles ⇔ image(a) < image(b); −0.0 and +0.0 have one image. No NaN comes here.
__device__ __forceinline__ u64 weight_image(double w, int maximum)
{
    if (maximum) w = -w;
    if (w == 0.0) w = 0.0;
    const u64 b = (u64)__double_as_longlong(w);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// keys[root] = min(keys[root], key) for every offering lane; called by all lanes of the wave. Where the offering lanes share one root (two ballots,
// as ktruss.hip's peel) the wave reduces and lane 0 sends the one atomic. The load in front skips an atomic that cannot lower the word.
template <typename K>
__device__ __forceinline__ void min_to_root(bool offer, int root, K key, K none, K *keys, int wave_min_on)
{
    const u64 m = __ballot(offer);
    if (!m) return;
    if (wave_min_on) {
        const int r0 = __shfl(root, __ffsll((long long)m) - 1);
        if (__ballot(offer && root == r0) == m) {
            const K least = wave_min(offer ? key : none);
            if (__lane_id() == 0 && least < ldk(keys + r0)) atomicMin(keys + r0, least);
            return;
        }
    }
    if (offer && key < ldk(keys + root)) atomicMin(keys + root, key);
}

__device__ __forceinline__ bool runs(const MsState *st) { return !st->invalid && st->stop == 0; }

// The block's sum into *word by one atomicAdd; called by every thread of the workgroup.
__device__ __forceinline__ void block_add(long long x, u64 *word)
{
    __shared__ long long s_x[WG / 64];
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) s_x[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_x[w];
        if (sum) atomicAdd(word, (u64)sum);
    }
}

// The page turn, by one thread behind the last ticket (or alone, after the opening pass): the list that was built becomes the current one.
__device__ __forceinline__ void turn(MsState *st, const StepArgs &a, bool opening)
{
    const long long work = (long long)atomicAdd((u64 *)&st->work_next, 0ull);
    int ln = atomicAdd(&st->live_next, 0);
    const int nh = atomicAdd(&st->n_hub_next, 0), found = atomicAdd(&st->found, 0);
    ln = ln < a.n ? ln : a.n;
    st->cur ^= 1;
    st->live_n = ln;
    st->n_hub_cur = nh;
    st->work_cur = work;
    st->live_next = 0;
    st->n_hub_next = 0;
    st->work_next = 0;
    st->found = 0;
    for (int p = 0; p <= kJumpPasses; ++p) st->pending[p] = 0;
    st->tickets = 0;
    if (!opening) st->round += 1;
    st->stop = (ln == 0 || (!opening && !found)) ? 1 : work > a.grid_cap ? 4 : 0;
}

// ------------------------------------------------------------------------------------------------ open
__global__ __launch_bounds__(WG) void ms_open_rows_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    long long work = 0;
    open_rows(a.n, g.rp, &st->invalid, 1, [&](long long i, int rb, int re) {
        g.parent[i] = (int)i;
        g.key_w[i] = kNone64;
        g.key_p[i] = kNone64;
        g.key_k[i] = kNone;
        g.stamp[i] = 0;
        if (i == a.n - 1) st->nnz = re;
        // a bad rowptr gives a length that means nothing: it is compared and summed, never an index
        append_frontier(re > rb, (int)i, re - rb, a.n, a.hub_cap, g.live[1], g.hubs[1], &st->live_next, &st->n_hub_next, work);
    });
    block_add(work, (u64 *)&st->work_next);
}

__global__ __launch_bounds__(WG) void ms_open_ids_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    if (st->invalid) return;                                       // rowptr is monotone from 0 beyond this line: [0, rowptr[n]) is the colids array
    open_ids<false>(a.n, a.hub_cap, g.rp, g.ci, g.hubs[0], &st->open_hubs, &st->invalid, 2, [](int, int, int) {});
}

__global__ __launch_bounds__(WG) void ms_open_hubs_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    if (st->invalid) return;
    open_hubs<false>(a.n, a.hub_cap, g.rp, g.ci, g.hubs[0], &st->open_hubs, &st->invalid, 2, [](int, int, int) {});
}

__global__ __launch_bounds__(WG) void ms_open_values_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    if (st->invalid) return;
    const long long nnz = g.rp[a.n];
    int bad = 0;
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) bad |= g.val[k] != g.val[k];
    if (bad) atomicOr(&st->invalid, 8);
}

__global__ void ms_begin_kernel(MsState *st, const StepArgs a)
{
    if (st->invalid) return;
    turn(st, a, true);
}

// ------------------------------------------------------------------------------------------------ a round
template <int STAGE>
__global__ __launch_bounds__(WG) void ms_find_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    const int stop = st->stop;
    if (st->invalid || !step_runs(stop, a.resume)) return;
    // every workgroup of this launch runs whether it reads 4 or 0; the kernels behind it want 0
    if (stop == 4 && blockIdx.x == 0 && threadIdx.x == 0) st->stop = 0;
    const int round = st->round + 1, cur = st->cur;
    const int *live = g.live[cur], *hubs = g.hubs[cur];
    const int live_n = st->live_n < a.n ? st->live_n : a.n, nh = st->n_hub_cur < a.hub_cap ? st->n_hub_cur : a.hub_cap;
    long long walked = 0;
    auto entry = [&](bool valid, int k, RowPay p) {
        bool out = false;
        int v = 0, rv = 0;
        if (valid) {
            v = g.ci[k];
            rv = ld(g.parent + v);
            out = rv != p.ru;
            walked += 1;
        }
        u64 img = 0;
        if (out && g.val) img = weight_image(g.val[k], g.maximum);
        if (a.first && out && g.stamp[p.u] != round) g.stamp[p.u] = round;
        if (STAGE == 0) {
            min_to_root(out, p.ru, img, kNone64, g.key_w, a.wave_min);
            min_to_root(out, rv, img, kNone64, g.key_w, a.wave_min);
            return;
        }
        const u64 pair = p.u < v ? ((u64)(unsigned)p.u << 32) | (unsigned)v : ((u64)(unsigned)v << 32) | (unsigned)p.u;
        bool ou = out, ov = out;
        if (out && g.val) {
            ou = img == g.key_w[p.ru];
            ov = img == g.key_w[rv];
        }
        if (STAGE == 1) {
            min_to_root(ou, p.ru, pair, kNone64, g.key_p, a.wave_min);
            min_to_root(ov, rv, pair, kNone64, g.key_p, a.wave_min);
            return;
        }
        ou = ou && pair == g.key_p[p.ru];
        ov = ov && pair == g.key_p[rv];
        min_to_root(ou, p.ru, k, kNone, g.key_k, a.wave_min);
        min_to_root(ov, rv, k, kNone, g.key_k, a.wave_min);
    };
    walk_tiles<RowPay>(live_n, [&](int i, int &start, int &len, RowPay &p) {
        const int u = live[i];
        const int rb = g.rp[u], l = g.rp[u + 1] - rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        p = RowPay{u, ld(g.parent + u)};
        start = rb;
        len = l;
    }, entry);
    walk_hubs<RowPay>(nh, [&](int h, int &start, int &len, RowPay &p) {
        const int u = hubs[h];
        p = RowPay{u, ld(g.parent + u)};
        start = g.rp[u];
        len = g.rp[u + 1] - start;
    }, entry);
    block_add(walked, &st->entries_walked);
}

// The two ends of the entry a root chose, out of its pair word.
__device__ __forceinline__ void ends_of(u64 pair, int &lo, int &hi) { lo = (int)(pair >> 32); hi = (int)(pair & 0xffffffffull); }

__global__ __launch_bounds__(WG) void ms_pick_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    if (!runs(st)) return;
    int any = 0;
    for (long long v0 = (long long)blockIdx.x * WG; v0 < a.n; v0 += (long long)gridDim.x * WG) {
        const long long v = v0 + threadIdx.x;
        const int k = v < a.n ? g.key_k[v] : kNone;
        bool app = false;
        if (k != kNone) {
            int lo, hi;
            ends_of(g.key_p[v], lo, hi);
            const int rl = g.parent[lo], rh = g.parent[hi];        // exact: nothing writes parent[] in this kernel or in the find stages
            const int other = rl == (int)v ? rh : rl;
            app = rl != rh && !(other < (int)v && g.key_k[other] == k);
            any = 1;
        }
        const int idx = wave_append(app, &st->n_edges);
        if (app && (unsigned)idx < (unsigned)(a.n - 1)) g.flist[idx] = k;   // a forest has at most n − 1 edges
    }
    if (__ballot(any) && __lane_id() == 0) atomicOr(&st->found, 1);
}

__global__ __launch_bounds__(WG) void ms_link_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    if (!runs(st)) return;
    for (long long v = (long long)blockIdx.x * WG + threadIdx.x; v < a.n; v += (long long)gridDim.x * WG) {
        if (g.key_k[v] == kNone) continue;
        int lo, hi;
        ends_of(g.key_p[v], lo, hi);
        g.key_w[v] = kNone64;
        g.key_p[v] = kNone64;
        g.key_k[v] = kNone;
        link_from(ld(g.parent + lo), ld(g.parent + hi), g.parent);
    }
}

__global__ __launch_bounds__(WG) void ms_jump_kernel(int n, int *parent, MsState *st, int pass)
{
    if (!runs(st) || (pass && !st->pending[pass])) return;
    if (jump_pass(n, parent)) atomicOr(&st->pending[pass + 1], 1);
}

__global__ __launch_bounds__(WG) void ms_turn_kernel(const Arrays g, MsState *st, const StepArgs a)
{
    __shared__ long long s_work[WG / 64];
    if (!runs(st)) return;
    const int round = st->round + 1, cur = st->cur;
    const int *live = g.live[cur];
    const int live_n = st->live_n < a.n ? st->live_n : a.n;
    long long work = 0;
    for (long long i0 = (long long)blockIdx.x * WG; i0 < live_n; i0 += (long long)gridDim.x * WG) {
        const long long i = i0 + threadIdx.x;
        const int u = i < live_n ? live[i] : 0;
        const bool want = i < live_n && g.stamp[u] == round;
        const int len = want ? g.rp[u + 1] - g.rp[u] : 0;
        append_frontier(want, u, len, a.n, a.hub_cap, g.live[cur ^ 1], g.hubs[cur ^ 1], &st->live_next, &st->n_hub_next, work);
    }
    work = wave_sum(work);
    if ((threadIdx.x & 63) == 0) s_work[threadIdx.x >> 6] = work;
    if (!turn_page(&st->tickets, [&] {
        long long ws = 0;
        for (int w = 0; w < WG / 64; ++w) ws += s_work[w];
        if (ws) atomicAdd((u64 *)&st->work_next, (u64)ws);
    })) return;
    turn(st, a, false);
}

// ------------------------------------------------------------------------------------------------ close
// keys[i] = nnz − 1 − list[i]: the library's sort is descending
__global__ __launch_bounds__(WG) void ms_sort_keys_kernel(int m, int nnz, const int *__restrict__ list, int *__restrict__ keys)
{
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < m; i += (long long)gridDim.x * WG) keys[i] = nnz - 1 - list[i];
}

// The sum of a workgroup's values in a fixed shape: the shuffle ladder inside a wave, the four waves left to right. Thread 0 has it.
__device__ __forceinline__ double block_sum_fixed(double x)
{
    __shared__ double s_x[WG / 64];
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) s_x[threadIdx.x >> 6] = x;
    __syncthreads();
    double sum = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WG / 64; ++w) sum += s_x[w];
    __syncthreads();
    return sum;
}

__global__ __launch_bounds__(WG) void ms_weight_tiles_kernel(int m, const int *__restrict__ edges, const double *__restrict__ val, double *__restrict__ partial)
{
    const int tiles = (m + kSumTile - 1) / kSumTile;
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
        const long long base = (long long)tile * kSumTile + (long long)threadIdx.x * (kSumTile / WG);
        double x = 0.0;
        for (int u = 0; u < kSumTile / WG; ++u)
            if (base + u < m) x += val[edges[base + u]];
        const double sum = block_sum_fixed(x);
        if (threadIdx.x == 0) partial[tile] = sum;
    }
}

__global__ __launch_bounds__(WG) void ms_weight_total_kernel(int tiles, const double *__restrict__ partial, MsState *st)
{
    double x = 0.0;
    for (int j = (int)threadIdx.x; j < tiles; j += WG) x += partial[j];
    const double sum = block_sum_fixed(x);
    if (threadIdx.x == 0) st->weight = sum;
}

// ------------------------------------------------------------------------------------------------ host side
int bits_of(long long x)
{
    int b = 1;
    while (b < 31 && (1LL << b) <= x) ++b;
    return b;
}

template <typename Kernel, typename... Args>
void go(Kernel kernel, int grid, hipStream_t s, Counts *cnt, Args... args)
{
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(WG), 0, s, args...);
    cnt->launches += 1;
}

// The whole call on device arrays; returns behind a wait on `s` with *h the final state. nnz_hint: rowptr[n] when the host knows it, −1 otherwise.
int run(int n, const Arrays &g, int *edges, MsState *st, int hub_cap, int cus, long long nnz_hint, MsState *h, Counts *cnt, hipStream_t s)
{
    // G4S_MSF_FIRST_GRID and G4S_MSF_WAVE_MIN are A/B switches: the outputs do not depend on them. The live rows only shrink from round
    // to round, so a grid can be too small only for the first batch: when the switch says so.
    const int forced = env_int("G4S_MSF_FIRST_GRID", 0, 0, 2 * cus);
    const StepGrid sized(forced ? std::min(forced, kMinGrid) : kMinGrid, 2 * cus);
    const int first_grid = forced ? forced : nnz_hint >= 0 ? sized.grid(nnz_hint) : sized.max_grid;
    const int g_n = grid_for<WG>(n, 8192), g_turn = grid_for<WG>(n, cus), g_nnz = nnz_hint >= 0 ? grid_for<WG>(nnz_hint, 8192) : 8192;
    const int stages = g.val ? 3 : 2, per_round = stages + 3 + kJumpPasses;
    StepArgs a;
    a.grid_cap = sized.cap(first_grid);
    a.n = n;
    a.hub_cap = hub_cap;
    a.resume = 0;
    a.first = 0;
    a.wave_min = env_int("G4S_MSF_WAVE_MIN", 1, 0, 1);

    go(ms_open_rows_kernel, grid_for<WG>(n, cus), s, cnt, g, st, a);
    go(ms_open_ids_kernel, grid_for<WG>(n, 2048), s, cnt, g, st, a);
    go(ms_open_hubs_kernel, 1024, s, cnt, g, st, a);
    if (g.val) go(ms_open_values_kernel, g_nnz, s, cnt, g, st, a);
    hipLaunchKernelGGL(ms_begin_kernel, dim3(1), dim3(1), 0, s, st, a);
    cnt->launches += 1;
    G4S_HIP_TRY(hipGetLastError());

    ReadScope reads(s);
    bool know = false;                                             // *h is the device's state
    int rounds = (kBatch + per_round - 1) / per_round;             // whole rounds per batch
    for (;;) {
        const int grid = know ? sized.grid(h->work_cur) : first_grid;
        a.grid_cap = sized.cap(grid);
        for (int r = 0; r < rounds; ++r) {
            for (int stage = 3 - stages; stage < 3; ++stage) {
                a.first = stage == 3 - stages;
                a.resume = r == 0 && a.first && know && h->stop == 4;
                if (stage == 0) go(ms_find_kernel<0>, grid, s, cnt, g, st, a);
                else if (stage == 1) go(ms_find_kernel<1>, grid, s, cnt, g, st, a);
                else go(ms_find_kernel<2>, grid, s, cnt, g, st, a);
            }
            a.first = a.resume = 0;
            go(ms_pick_kernel, g_n, s, cnt, g, st, a);
            go(ms_link_kernel, g_n, s, cnt, g, st, a);
            for (int p = 0; p < kJumpPasses; ++p) go(ms_jump_kernel, g_n, s, cnt, n, g.parent, st, p);
            go(ms_turn_kernel, std::min(grid, g_turn), s, cnt, g, st, a);
        }
        G4S_HIP_TRY(hipGetLastError());
        if (know && h->stop == 4) cnt->resumes += 1;
        const MsState before = *h;
        G4S_HIP_TRY(reads.fetch(*h, st));
        cnt->waits += 1;
        if (h->invalid || h->stop == 1) break;
        // a batch that began with stop == 0, or resumed from 4, runs at least one round
        if (know && h->round == before.round)
            return g4s::set_error(G4S_ERR_HIP, "g4s_minimum_spanning_forest: internal: a batch of %d rounds made no step (stop %d)", rounds, h->stop);
        if (know) rounds = std::max(rounds, std::min(2 * rounds, kBatchMax / per_round));
        know = true;
    }
    if (h->invalid) return G4S_OK;

    const int m = std::min(h->n_edges, std::max(n - 1, 0));
    if (m > 0) {
        // the live lists, the stamps and the key words are free now: the sort's keys and its ping-pong partners
        go(ms_sort_keys_kernel, grid_for<WG>(m, 8192), s, cnt, m, h->nnz, (const int *)g.flist, g.live[0]);
        const int kb = bits_of(h->nnz);
        G4S_TRY(prims::sort_pairs_descending(g.live[0], g.flist, g.live[1], edges, g.stamp, g.key_k, m, kb, s));
        cnt->launches += 3 * ((kb + 3) / 4);
        if (g.val) {
            const int tiles = (m + kSumTile - 1) / kSumTile;
            go(ms_weight_tiles_kernel, std::min(tiles, 8 * cus), s, cnt, m, (const int *)edges, g.val, (double *)g.key_w);
            go(ms_weight_total_kernel, 1, s, cnt, tiles, (const double *)g.key_w, st);
        }
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(reads.fetch(*h, st));                          // the weight, and the end of the sort: the call is synchronous
        cnt->waits += 1;
    }
    return G4S_OK;
}

const char *invalid_text(int bits)
{
    const char *t = csr_invalid_text(bits);
    return t ? t : "a value is NaN";
}

} // namespace

G4S_API g4s_status g4s_minimum_spanning_forest(int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values, int32_t *edges, int32_t *labels,
                                               unsigned flags, g4s_msf_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_DEVICE_POINTERS | G4S_MSF_MAXIMUM)) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and G4S_MSF_MAXIMUM");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr || n == 0, "rowptr is NULL");               // one vertex still has a row to check
    G4S_REQUIRE(edges || n <= 1, "edges is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    const size_t nb = sizeof(int32_t) * (size_t)n, eb = sizeof(int32_t) * (size_t)std::max(n - 1, 0);
    long long nnz = -1;
    if (n > 0) {
        size_t cb = sizeof(int32_t), vb = sizeof(double);          // with device pointers rowptr[n] is not known here: the first element stands for the array
        if (!device) {
            nnz = rowptr[n];
            G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
            cb = sizeof(int32_t) * (size_t)nnz;
            vb = sizeof(double) * (size_t)nnz;
        }
        const Span outs[] = {{edges, eb}, {labels, nb}}, ins[] = {{rowptr, nb + sizeof(int32_t)}, {colids, cb}, {values, vb}};
        G4S_REQUIRE(!any_overlap(outs, ins), "edges and labels must not overlap the inputs or each other");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) *info = g4s_msf_info{};
    if (n == 0) return G4S_OK;

    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const int hub_cap = std::min(n, kHubCap);
    MsState *st, h{};
    Arrays g{};
    int *own_parent = nullptr;
    Carver work;
    work.piece(&st, kStateBytes);
    for (u64 **p : {&g.key_w, &g.key_p}) work.piece(p, sizeof(u64) * (size_t)n);
    for (int **p : {&g.key_k, &g.stamp, &g.live[0], &g.live[1], &g.flist}) work.piece(p, sizeof(int) * (size_t)n);
    if (!labels) work.piece(&own_parent, nb);
    work.piece(&g.hubs[0], sizeof(int) * (size_t)hub_cap);
    work.tail(&g.hubs[1], sizeof(int) * (size_t)hub_cap);
    Staged stage(s);
    Counts cnt;
    int status = work.alloc();
    g.rp = rowptr; g.ci = colids; g.val = values; g.parent = labels;
    g.maximum = (flags & G4S_MSF_MAXIMUM) != 0;
    int *edges_dev = edges;
    if (status == G4S_OK && !device) {
        g.rp = stage.in(rowptr, nb + sizeof(int32_t));
        g.ci = nnz ? stage.in(colids, sizeof(int32_t) * (size_t)nnz) : stage.out<int>(sizeof(int32_t));   // of an empty array nothing is read
        if (values) g.val = nnz ? stage.in(values, sizeof(double) * (size_t)nnz) : stage.out<double>(sizeof(double));
        if (labels) g.parent = stage.out<int>(nb);
        edges_dev = stage.out<int>(std::max(eb, sizeof(int32_t)));
        status = stage.error();
    }
    if (!labels) g.parent = own_parent;
    auto hip_ok = [](hipError_t e, const char *what) { return e == hipSuccess ? G4S_OK : g4s::set_error(G4S_ERR_HIP, "g4s_minimum_spanning_forest: %s: %s", what, hipGetErrorString(e)); };
    if (status == G4S_OK) status = hip_ok(hipMemsetAsync(st, 0, kStateBytes, s), "hipMemsetAsync");
    if (status == G4S_OK) status = run(n, g, edges_dev, st, hub_cap, cus, nnz, &h, &cnt, s);
    const int m = std::min(h.n_edges, std::max(n - 1, 0));
    if (status == G4S_OK && !device && !h.invalid) {
        status = stage.to_host(edges, edges_dev, sizeof(int32_t) * (size_t)m);
        if (status == G4S_OK && labels) status = stage.to_host(labels, g.parent, nb);
        if (status == G4S_OK) status = stage.wait();
        cnt.waits += 1;
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    work.idle();
    if (status == G4S_OK && h.invalid) status = g4s::set_error(G4S_ERR_INVALID, "g4s_minimum_spanning_forest: %s", invalid_text(h.invalid));
    if (status == G4S_OK && info) {
        info->components = (int64_t)n - m;
        info->edges = m;
        info->weight = values ? h.weight : 0.0;
        info->entries_walked = (int64_t)h.entries_walked;
        info->rounds = h.round;
        info->launches = cnt.launches;
        info->resumes = cnt.resumes;
        info->host_waits = cnt.waits;
    }
    return status;
}
