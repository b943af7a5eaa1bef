// scc.hip — g4s_strongly_connected_components (include/g4s.h): the strongly connected components of the directed graph whose edges u → v are the stored
// entries (u, v) of an n × n CSR pattern, as canonical labels (labels[v] = the smallest vertex id of v's component). The Multistep shape (Slota,
// Rajamanickam, Madduri 2014) on this library's pieces: trim to the fixpoint, one pivot by forward / backward reach, colouring rounds for the rest,
// and the peel of kcore.hip between them. DESIGN §4.18.
//
// State lives on the device (scc.hpp, ScState), and so does the decision what to do next: st->phase names the one kernel that may run, every kernel
// begins with `if (st->phase != mine) return`, and the workgroup that finishes last (a ticket counter, no waiting: turn_page of frontier.hpp) turns
// the page — it swaps the frontiers and sets the next phase. The host therefore only GUESSES: it enqueues batches of kBatch (doubling to kBatchMax)
// launches blind, in the order the phases usually follow each other, behind one read of the state; a wrong guess costs launches that return at once,
// never a wrong result.
//
//   open    sc_check_rows_kernel for A and for Aᵀ (zero-based, non-decreasing; rowptr[n] kept), sc_open_kernel (trowptr[n] == rowptr[n]; labels = −1,
//           dout / din = the row lengths, mark = 0, stamp = −1), sc_open_ids_kernel / sc_open_hubs_kernel for each pattern: ids in [0, n), a stored
//           diagonal entry takes one off the row's counter. Every later kernel begins with `if (st->invalid) return`.
//   SCAN    every vertex with din == 0 or dout == 0 labels itself and joins the queue. Runs once: afterwards a counter reaches 0 only under a peel.
//   PEEL    the frontier walk over queue[head, end), rows of A (one atomicSub of din[w] per entry u → w) and rows of Aᵀ (of dout[u]); the lane that
//           brings a counter to 0 claims labels[w] by one compare-and-swap from −1 and appends w. Runs dry → nobody live: DONE; else the pivot, or
//           after it a colouring round.
//   PVMAX, PVMIN  two reductions over the live vertices: the largest din·dout (64 bits), then the smallest id that has it. PVMIN's page turn seeds FWD.
//   FWD     push steps over A on the work queue: mark bit 1 by atomicOr, live vertices only. Dry → BWD, seeded with the pivot.
//   BWD     push steps over Aᵀ on the queue, entering only vertices whose mark is exactly 1 (forward-reached, not yet backward): what it queues IS the
//           pivot's component, behind round_start, and the smallest id among it is reduced on the way. Dry → LABEL.
//   LABEL   labels[queue[i]] = that id; the page turn makes queue[round_start, tail) the frontier of the PEEL that removes the component.
//   CINIT   colour[v] = v on live vertices (mark's array: the marks are not read again), all of them into the work queue.
//   CPUSH   push steps over A: colour[v] read once per row (per chunk of a hub), atomicMin on the colour of each live out-neighbour; a vertex that was
//           lowered joins the next frontier once, decided by atomicExch of a per-vertex stamp with the step's number (never reused within a call).
//   CROOTS  live vertices with colour[v] == v: labels[v] = v, into the queue. The smallest live id is always one, so a round removes a component.
//   CBWD    push steps over Aᵀ on the queue: u with labels[u] == −1 and colour[u] == the row's label is claimed by compare-and-swap. Dry → PEEL of
//           queue[round_start, tail): everything the round labelled.
//   count   behind the loop: roots, one atomicAdd per (wave, label) for the sizes (in din's array), the largest by a max over (size, −label).
// The queue holds every vertex once, when it dies, so it has n ints and tail == n means nobody is live; the lists of queued vertices whose row of A or
// of Aᵀ is a hub have the queue's own layout. The work queue is double-buffered: a vertex may be lowered in many steps, but once per step.
// Memory model: kernel boundaries and the ticket of turn_page are the only ordering between workgroups. Plain loads that may be
// stale, and why that is harmless: labels[w] in PEEL / CBWD (a stale −1 sends the lane to an atomic: the compare-and-swap decides, and a decrement
// on a dead vertex's counter is never read); mark[w] in FWD / BWD (bits are only set: a stale value sends the lane to the atomicOr, whose return
// decides); colour[w] in CPUSH (colours only decrease: a stale value is too large and the atomicMin decides) and the row's own colour (too large: it
// pushes a value that atomicMin ignores or that lowers less, and whoever lowered the row's vertex has queued it for the next step). Nothing spins;
// every loop is bounded by a queue or a row length.
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "scc.hpp"
#include <algorithm>
#include <climits>

namespace {

using namespace g4s;   // ScState, SC_*

constexpr int kBatch = G4S_SCC_BATCH;        // launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr int kReps = 3;                     // launches of a stepped phase the host guesses before it moves on
constexpr size_t kStateBytes = 256;
static_assert(sizeof(ScState) <= kStateBytes, "state block");

struct StepArgs {
    long long grid_cap;    // a frontier with more work than this asks for a larger grid
    int n;
    int hub_cap;           // room in each hub list
    int resume;            // the first launch of a batch goes on from stop == 4
};

struct Arrays {
    const int *rp, *ci, *trp, *tci;
    int *labels, *din, *dout, *queue, *colour, *stamp;
    int *wq[2], *whub[2];  // the work queue and its hubs (rows of A)
    int *hub_a, *hub_t;    // the queued vertices with a hub row in A, in Aᵀ
};

struct Tally {
    long long work = 0, walked = 0;
    int cnt = 0, mn = INT_MAX;
    unsigned long long mx = 0;
};

// A vertex that dies, or that a backward reach enters: behind the tail of the queue, and into the hub lists when its rows are long. Called by every
// lane that is active at the call site. A vertex is queued once per call: idx < n by construction.
__device__ __forceinline__ void append_queue(bool want, int v, const StepArgs &a, const Arrays &g, ScState *st, Tally &t)
{
    const int idx = wave_append(want, &st->tail);
    if (!want) return;
    if ((unsigned)idx < (unsigned)a.n) g.queue[idx] = v;
    const int la = g.rp[v + 1] - g.rp[v], lt = g.trp[v + 1] - g.trp[v];
    if (la > kHubCut) {
        const int h = atomicAdd(&st->ha_tail, 1);
        if ((unsigned)h < (unsigned)a.hub_cap) g.hub_a[h] = v;
    }
    if (lt > kHubCut) {
        const int h = atomicAdd(&st->ht_tail, 1);
        if ((unsigned)h < (unsigned)a.hub_cap) g.hub_t[h] = v;
    }
    t.work += (long long)la + lt + 1;
}

// A vertex for the next frontier of FWD / CPUSH: once per step by construction (the mark, the stamp), so idx < n.
__device__ __forceinline__ void append_work(bool want, int v, int *__restrict__ wq, int *__restrict__ whub, const StepArgs &a, const Arrays &g, ScState *st, Tally &t)
{
    const int idx = wave_append(want, &st->w_next);
    if (!want) return;
    if ((unsigned)idx < (unsigned)a.n) wq[idx] = v;
    const int la = g.rp[v + 1] - g.rp[v];
    if (la > kHubCut) {
        const int h = atomicAdd(&st->wh_next, 1);
        if ((unsigned)h < (unsigned)a.hub_cap) whub[h] = v;
    }
    t.work += (long long)la + 1;
}

__device__ __forceinline__ int row_len(const int *rp, int v) { return rp[v + 1] - rp[v]; }

// The page turn of phase PH, by thread 0 of the workgroup that took the last ticket: the totals of the kernel, read with atomics, become the next
// step's state, written with plain stores for the next kernel.
template <int PH>
__device__ __forceinline__ void turn(ScState *st, const StepArgs &a, const Arrays &g)
{
    long long work = (long long)atomicAdd((unsigned long long *)&st->work_next, 0ull);
    int tail = atomicAdd(&st->tail, 0), ha = atomicAdd(&st->ha_tail, 0), ht = atomicAdd(&st->ht_tail, 0);
    const int wn = atomicAdd(&st->w_next, 0), whn = atomicAdd(&st->wh_next, 0);
    const int cnt = atomicAdd(&st->cnt_acc, 0), mn = atomicAdd(&st->mn_acc, 0);
    const unsigned long long mx = atomicAdd(&st->mx_acc, 0ull);
    tail = tail < a.n ? tail : a.n;
    const int got = tail - st->end;                                // what this kernel appended to the queue
    st->work_next = 0;
    st->cnt_acc = 0;
    st->mn_acc = INT_MAX;
    st->mx_acc = 0;
    st->tickets = 0;
    int phase = PH;
    // the queue: the built frontier becomes the current one; a reach remembers where it began, and ends by handing all of it to the peel
    auto next_frontier = [&] { st->head = st->end; st->end = tail; st->ha_head = st->ha_end; st->ha_end = ha; st->ht_head = st->ht_end; st->ht_end = ht; };
    auto reach_begins = [&] { st->round_start = st->end; st->ha_round = st->ha_end; st->ht_round = st->ht_end; st->round_work = 0; };   // end == tail here
    auto reach_to_peel = [&] { st->head = st->round_start; st->ha_head = st->ha_round; st->ht_head = st->ht_round; phase = SC_PEEL; work = st->round_work; };
    auto next_work = [&](int n_, int nh_) { st->w_cur ^= 1; st->w_n = n_; st->w_next = 0; st->wh_n = nh_; st->wh_next = 0; };
    if (PH == SC_SCAN || PH == SC_PEEL) {
        st->trimmed += cnt;
        next_frontier();
        if (PH == SC_SCAN) phase = SC_PEEL;
        else if (got == 0) phase = tail >= a.n ? SC_DONE : st->pivot_done ? SC_CINIT : SC_PVMAX;
    } else if (PH == SC_PVMAX) {
        st->best_prod = mx;
        phase = SC_PVMIN;
    } else if (PH == SC_PVMIN) {
        const int p = mn < a.n ? mn : 0;                           // live vertices exist: mn is one of them
        const int la = row_len(g.rp, p);
        st->pivot = p;
        g.colour[p] = 1;
        g.wq[st->w_cur ^ 1][0] = p;
        if (la > kHubCut) g.whub[st->w_cur ^ 1][0] = p;
        next_work(1, la > kHubCut ? 1 : 0);
        work = (long long)la + 1;
        phase = SC_FWD;
    } else if (PH == SC_FWD) {
        next_work(wn, whn);
        if (wn == 0) {                                             // the forward set is complete: the pivot opens the backward reach, in the queue
            const int p = st->pivot, la = row_len(g.rp, p), lt = row_len(g.trp, p);
            reach_begins();
            g.colour[p] = 3;
            if (tail < a.n) g.queue[tail++] = p;                   // p is live: not yet in the queue
            if (la > kHubCut && ha < a.hub_cap) g.hub_a[ha++] = p;
            if (lt > kHubCut && ht < a.hub_cap) g.hub_t[ht++] = p;
            st->tail = tail; st->ha_tail = ha; st->ht_tail = ht;
            st->minid = p;
            work = (long long)la + lt + 1;
            next_frontier();
            st->round_work = work;
            phase = SC_BWD;
        }
    } else if (PH == SC_BWD || PH == SC_CBWD) {
        if (PH == SC_BWD && mn < st->minid) st->minid = mn;
        st->round_work += work;
        next_frontier();
        if (got == 0) {
            if (PH == SC_BWD) { phase = SC_LABEL; work = tail - st->round_start; }
            else reach_to_peel();
        }
    } else if (PH == SC_LABEL) {
        st->pivot_size = tail - st->round_start;
        st->pivot_done = 1;
        reach_to_peel();
    } else if (PH == SC_CINIT) {
        next_work(wn, whn);
        st->color_rounds += 1;
        phase = SC_CPUSH;
    } else if (PH == SC_CPUSH) {
        next_work(wn, whn);
        st->cstep += 1;
        if (wn == 0) phase = SC_CROOTS;
    } else if (PH == SC_CROOTS) {
        reach_begins();
        next_frontier();
        st->round_work = work;
        phase = SC_CBWD;
    }
    st->work_cur = work;
    st->phase = phase;
    st->stop = phase == SC_DONE ? 1 : work > a.grid_cap ? 4 : 0;
}

// The end of every phase kernel: the block's shares of the sums, the minimum and the maximum, then the ticket; the last block turns the page.
template <int PH>
__device__ __forceinline__ void finish(ScState *st, Tally t, const StepArgs &a, const Arrays &g)
{
    __shared__ long long s_work[WG / 64], s_walk[WG / 64];
    __shared__ unsigned long long s_mx[WG / 64];
    __shared__ int s_cnt[WG / 64], s_mn[WG / 64];
    t.work = wave_sum(t.work);
    t.walked = wave_sum(t.walked);
    t.cnt = wave_sum(t.cnt);
    t.mn = wave_min(t.mn);
    t.mx = wave_max(t.mx);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_work[w] = t.work; s_walk[w] = t.walked; s_cnt[w] = t.cnt; s_mn[w] = t.mn; s_mx[w] = t.mx;
    }
    if (!turn_page(&st->tickets, [&] {
        long long ws = 0, ks = 0;
        int c = 0, m = INT_MAX;
        unsigned long long x = 0;
        for (int w = 0; w < WG / 64; ++w) { ws += s_work[w]; ks += s_walk[w]; c += s_cnt[w]; m = s_mn[w] < m ? s_mn[w] : m; x = s_mx[w] > x ? s_mx[w] : x; }
        if (ws) atomicAdd((unsigned long long *)&st->work_next, (unsigned long long)ws);
        if (ks) atomicAdd(&st->edges_walked, (unsigned long long)ks);
        if (c) atomicAdd(&st->cnt_acc, c);
        if (m != INT_MAX) atomicMin(&st->mn_acc, m);
        if (x) atomicMax(&st->mx_acc, x);
    })) return;
    turn<PH>(st, a, g);
}

// May the kernel of phase PH run? The same words for every block: they change only after the last ticket.
template <int PH>
__device__ __forceinline__ bool my_turn(const ScState *st, const StepArgs &a) { return !st->invalid && st->phase == PH && step_runs(st->stop, a.resume); }

// ------------------------------------------------------------------------------------------------ open
__global__ __launch_bounds__(WG) void sc_check_rows_kernel(int n, const int *__restrict__ rowptr, int slot, ScState *st)
{
    open_rows(n, rowptr, &st->invalid, slot ? 4 : 1, [&](long long i, int, int re) { if (i == n - 1) st->nnz[slot] = re; });
}

__global__ __launch_bounds__(WG) void sc_open_kernel(int n, const Arrays g, ScState *st)
{
    if (st->invalid) return;                                       // both row pointers are monotone from 0 beyond this line
    if (st->nnz[0] != st->nnz[1]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&st->invalid, 16);
        return;
    }
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        g.labels[i] = -1;
        g.dout[i] = g.rp[i + 1] - g.rp[i];
        g.din[i] = g.trp[i + 1] - g.trp[i];
        g.colour[i] = 0;
        g.stamp[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->mn_acc = INT_MAX;
}

// The column ids of a pattern (open_ids / open_hubs; rows in any order): the diagonal does not count in the row's counter.
// `which`: 0 the pattern of A (counter = dout), 1 of Aᵀ (counter = din)
__global__ __launch_bounds__(WG) void sc_open_ids_kernel(int n, int hub_cap, int which, const int *__restrict__ rowptr, const int *__restrict__ colids, int *counter,
                                                         int *__restrict__ hubs, ScState *st)
{
    if (st->invalid) return;                                       // [0, rowptr[n]) is the colids array
    open_ids<false>(n, hub_cap, rowptr, colids, hubs, &st->open_hubs[which], &st->invalid, which ? 8 : 2, [&](int, int u, int v) { if (v == u) atomicSub(counter + u, 1); });
}

__global__ __launch_bounds__(WG) void sc_open_hubs_kernel(int n, int hub_cap, int which, const int *__restrict__ rowptr, const int *__restrict__ colids, int *counter,
                                                          const int *__restrict__ hubs, ScState *st)
{
    if (st->invalid) return;
    open_hubs<false>(n, hub_cap, rowptr, colids, hubs, &st->open_hubs[which], &st->invalid, which ? 8 : 2, [&](int, int u, int v) { if (v == u) atomicSub(counter + u, 1); });
}

// ------------------------------------------------------------------------------------------------ kernels over all vertices
// Calls body(valid, v) for every vertex, by all lanes of a wave together (the appends ballot).
template <typename Body>
__device__ __forceinline__ void for_vertices(int n, Body body)
{
    for (long long v0 = (long long)blockIdx.x * WG; v0 < n; v0 += (long long)gridDim.x * WG) {
        const long long v = v0 + threadIdx.x;
        body(v < n, (int)v);
    }
}

__global__ __launch_bounds__(WG) void sc_scan_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_SCAN>(st, a)) return;
    Tally t;
    for_vertices(a.n, [&](bool valid, int v) {
        const bool want = valid && (g.din[v] <= 0 || g.dout[v] <= 0);
        if (want) g.labels[v] = v;
        t.cnt += want;
        append_queue(want, v, a, g, st, t);
    });
    finish<SC_SCAN>(st, t, a, g);
}

__device__ __forceinline__ unsigned long long degree_product(const Arrays &g, int v)
{
    const int i = g.din[v], o = g.dout[v];
    return i > 0 && o > 0 ? (unsigned long long)i * (unsigned long long)o : 0ull;
}

__global__ __launch_bounds__(WG) void sc_pvmax_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_PVMAX>(st, a)) return;
    Tally t;
    for_vertices(a.n, [&](bool valid, int v) {
        if (valid && g.labels[v] == -1) {
            const unsigned long long p = degree_product(g, v) + 1ull;   // + 1: a live vertex always counts
            t.mx = p > t.mx ? p : t.mx;
        }
    });
    finish<SC_PVMAX>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_pvmin_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_PVMIN>(st, a)) return;
    const unsigned long long best = st->best_prod;
    Tally t;
    for_vertices(a.n, [&](bool valid, int v) {
        if (valid && g.labels[v] == -1 && degree_product(g, v) + 1ull == best) t.mn = v < t.mn ? v : t.mn;
    });
    finish<SC_PVMIN>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_label_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_LABEL>(st, a)) return;
    const int lo = st->round_start, hi = st->end < a.n ? st->end : a.n, id = st->minid;
    Tally t;
    for (long long i = lo + (long long)blockIdx.x * WG + threadIdx.x; i < hi; i += (long long)gridDim.x * WG) g.labels[g.queue[i]] = id;
    finish<SC_LABEL>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_cinit_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_CINIT>(st, a)) return;
    int *wq = g.wq[st->w_cur ^ 1], *whub = g.whub[st->w_cur ^ 1];
    Tally t;
    for_vertices(a.n, [&](bool valid, int v) {
        const bool want = valid && g.labels[v] == -1;
        if (want) g.colour[v] = v;
        append_work(want, v, wq, whub, a, g, st, t);
    });
    finish<SC_CINIT>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_croots_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_CROOTS>(st, a)) return;
    Tally t;
    for_vertices(a.n, [&](bool valid, int v) {
        const bool want = valid && g.labels[v] == -1 && g.colour[v] == v;
        if (want) g.labels[v] = v;
        append_queue(want, v, a, g, st, t);
    });
    finish<SC_CROOTS>(st, t, a, g);
}

// ------------------------------------------------------------------------------------------------ stepped kernels
// The rows of `rowptr` of the queue's current frontier, hubs out of `hubs`[h0, h1): entry(valid, k, payload of the row).
template <typename Pay, typename Entry>
__device__ __forceinline__ void walk_queue(const ScState *st, const StepArgs &a, const int *__restrict__ rowptr, const int *__restrict__ queue, const int *__restrict__ hubs,
                                           int h0, int h1, Pay pay_of, Entry entry)
{
    const int head = st->head, end = st->end < a.n ? st->end : a.n;
    walk_tiles<int>(end - head, [&](int i, int &start, int &len, int &pay) {
        const int u = queue[head + i];
        const int rb = rowptr[u], l = rowptr[u + 1] - rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        pay = pay_of(u);
        start = rb;
        len = l;
    }, entry);
    h0 = h0 < a.hub_cap ? h0 : a.hub_cap;
    h1 = h1 < a.hub_cap ? h1 : a.hub_cap;
    walk_hubs<int>(h1 - h0, [&](int h, int &start, int &len, int &pay) {
        const int u = hubs[h0 + h];
        pay = pay_of(u);
        start = rowptr[u];
        len = rowptr[u + 1] - start;
    }, entry);
}

// The rows of A of the work queue's current frontier.
template <typename Pay, typename Entry>
__device__ __forceinline__ void walk_work(const ScState *st, const StepArgs &a, const Arrays &g, Pay pay_of, Entry entry)
{
    const int *wq = g.wq[st->w_cur], *whub = g.whub[st->w_cur];
    walk_tiles<int>(st->w_n < a.n ? st->w_n : a.n, [&](int i, int &start, int &len, int &pay) {
        const int u = wq[i];
        const int rb = g.rp[u], l = g.rp[u + 1] - rb;
        if (l > kHubCut) return;
        pay = pay_of(u);
        start = rb;
        len = l;
    }, entry);
    walk_hubs<int>(st->wh_n < a.hub_cap ? st->wh_n : a.hub_cap, [&](int h, int &start, int &len, int &pay) {
        const int u = whub[h];
        pay = pay_of(u);
        start = g.rp[u];
        len = g.rp[u + 1] - start;
    }, entry);
}

__global__ __launch_bounds__(WG) void sc_peel_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_PEEL>(st, a)) return;
    Tally t;
    // one entry u → w of a dying u in `ids`, whose other end's counter is `counter`: the lane that brings it to 0 claims w
    auto entry_of = [&](const int *__restrict__ ids, int *counter) {
        return [&, ids, counter](bool valid, int k, int u) {
            bool want = false;
            int w = 0;
            if (valid) {
                w = ids[k];
                if (w != u) {
                    t.walked += 1;
                    if (ld(g.labels + w) == -1 && atomicSub(counter + w, 1) == 1) want = atomicCAS(g.labels + w, -1, w) == -1;
                }
            }
            t.cnt += want;
            append_queue(want, w, a, g, st, t);
        };
    };
    auto self = [](int u) { return u; };
    walk_queue(st, a, g.rp, g.queue, g.hub_a, st->ha_head, st->ha_end, self, entry_of(g.ci, g.din));
    walk_queue(st, a, g.trp, g.queue, g.hub_t, st->ht_head, st->ht_end, self, entry_of(g.tci, g.dout));
    finish<SC_PEEL>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_fwd_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_FWD>(st, a)) return;
    int *wq = g.wq[st->w_cur ^ 1], *whub = g.whub[st->w_cur ^ 1];
    Tally t;
    walk_work(st, a, g, [](int u) { return u; }, [&](bool valid, int k, int) {
        bool want = false;
        int w = 0;
        if (valid) {
            w = g.ci[k];
            t.walked += 1;
            if (ld(g.labels + w) == -1 && !(ld(g.colour + w) & 1)) want = !(atomicOr(g.colour + w, 1) & 1);
        }
        append_work(want, w, wq, whub, a, g, st, t);
    });
    finish<SC_FWD>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_bwd_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_BWD>(st, a)) return;
    Tally t;
    walk_queue(st, a, g.trp, g.queue, g.hub_t, st->ht_head, st->ht_end, [](int u) { return u; }, [&](bool valid, int k, int) {
        bool want = false;
        int u = 0;
        if (valid) {
            u = g.tci[k];
            t.walked += 1;
            if (ld(g.colour + u) == 1) want = atomicOr(g.colour + u, 2) == 1;   // forward-reached, hence live
            if (want) t.mn = u < t.mn ? u : t.mn;
        }
        append_queue(want, u, a, g, st, t);
    });
    finish<SC_BWD>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_cpush_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_CPUSH>(st, a)) return;
    int *wq = g.wq[st->w_cur ^ 1], *whub = g.whub[st->w_cur ^ 1];
    const int step = st->cstep;
    Tally t;
    walk_work(st, a, g, [&](int u) { return ld(g.colour + u); }, [&](bool valid, int k, int c) {
        bool want = false;
        int w = 0;
        if (valid) {
            w = g.ci[k];
            t.walked += 1;
            if (ld(g.labels + w) == -1 && ld(g.colour + w) > c && atomicMin(g.colour + w, c) > c) want = atomicExch(g.stamp + w, step) != step;
        }
        append_work(want, w, wq, whub, a, g, st, t);
    });
    finish<SC_CPUSH>(st, t, a, g);
}

__global__ __launch_bounds__(WG) void sc_cbwd_kernel(const Arrays g, ScState *st, const StepArgs a)
{
    if (!my_turn<SC_CBWD>(st, a)) return;
    Tally t;
    walk_queue(st, a, g.trp, g.queue, g.hub_t, st->ht_head, st->ht_end, [&](int u) { return g.labels[u]; }, [&](bool valid, int k, int c) {
        bool want = false;
        int u = 0;
        if (valid) {
            u = g.tci[k];
            t.walked += 1;
            if (ld(g.labels + u) == -1 && g.colour[u] == c) want = atomicCAS(g.labels + u, -1, c) == -1;
        }
        append_queue(want, u, a, g, st, t);
    });
    finish<SC_CBWD>(st, t, a, g);
}

// ------------------------------------------------------------------------------------------------ the statistics (components.hip's)
__global__ __launch_bounds__(WG) void sc_zero_kernel(int n, int *__restrict__ count, const ScState *st)
{
    if (st->invalid) return;
    for (long long v = (long long)blockIdx.x * WG + threadIdx.x; v < n; v += (long long)gridDim.x * WG) count[v] = 0;
}

// Roots, and the size of every label: lanes of a wave that share a label issue one add.
__global__ __launch_bounds__(WG) void sc_count_kernel(int n, const int *__restrict__ labels, int *__restrict__ count, ScState *st)
{
    __shared__ long long s_red[WG / 64];
    if (st->invalid) return;
    const int lane = (int)threadIdx.x & 63;
    long long roots = 0;
    for (long long v0 = (long long)blockIdx.x * WG; v0 < n; v0 += (long long)gridDim.x * WG) {
        const long long v = v0 + threadIdx.x;
        const bool valid = v < n;
        const int l = valid ? labels[v] : -1;
        const bool act = valid && (unsigned)l < (unsigned)n;
        roots += act && l == v;
        unsigned long long m = __ballot(act);                      // the same for every lane: the loop below is uniform
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const int lbl = __shfl(l, leader);
            const unsigned long long same = __ballot(act && l == lbl);
            if (lane == leader) atomicAdd(count + lbl, __popcll(same));
            m &= ~same;
        }
    }
    roots = wave_sum(roots);
    if (lane == 0) s_red[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long r = 0;
        for (int w = 0; w < WG / 64; ++w) r += s_red[w];
        if (r) atomicAdd(&st->components, (unsigned long long)r);
    }
}

__global__ __launch_bounds__(WG) void sc_largest_kernel(int n, const int *__restrict__ labels, const int *__restrict__ count, ScState *st)
{
    __shared__ unsigned long long s_red[WG / 64];
    if (st->invalid) return;
    unsigned long long best = 0;
    for (long long v = (long long)blockIdx.x * WG + threadIdx.x; v < n; v += (long long)gridDim.x * WG) {
        if (labels[v] != v) continue;
        const unsigned long long key = ((unsigned long long)(unsigned)count[v] << 32) | (unsigned)(INT_MAX - (int)v);
        best = key > best ? key : best;
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WG / 64; ++w) best = s_red[w] > best ? s_red[w] : best;
        if (best) atomicMax(&st->best, best);
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool stepped(int ph) { return ph == SC_PEEL || ph == SC_FWD || ph == SC_BWD || ph == SC_CPUSH || ph == SC_CBWD; }

// The phase the host expects behind `ph`. Only a guess: the device decides.
int guess_next(int ph, bool pivot_done)
{
    switch (ph) {
    case SC_PEEL: return pivot_done ? SC_CINIT : SC_PVMAX;
    case SC_LABEL: case SC_CBWD: return SC_PEEL;
    default: return ph + 1;                                        // SCAN → PEEL, PVMAX → PVMIN → FWD → BWD → LABEL, CINIT → CPUSH → CROOTS → CBWD
    }
}

void launch(int ph, int grid, int g_scan, const Arrays &g, ScState *st, const StepArgs &a, hipStream_t s)
{
    switch (ph) {
    case SC_PEEL: hipLaunchKernelGGL(sc_peel_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    case SC_PVMAX: hipLaunchKernelGGL(sc_pvmax_kernel, dim3(g_scan), dim3(WG), 0, s, g, st, a); break;
    case SC_PVMIN: hipLaunchKernelGGL(sc_pvmin_kernel, dim3(g_scan), dim3(WG), 0, s, g, st, a); break;
    case SC_FWD: hipLaunchKernelGGL(sc_fwd_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    case SC_BWD: hipLaunchKernelGGL(sc_bwd_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    case SC_LABEL: hipLaunchKernelGGL(sc_label_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    case SC_CINIT: hipLaunchKernelGGL(sc_cinit_kernel, dim3(g_scan), dim3(WG), 0, s, g, st, a); break;
    case SC_CPUSH: hipLaunchKernelGGL(sc_cpush_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    case SC_CROOTS: hipLaunchKernelGGL(sc_croots_kernel, dim3(g_scan), dim3(WG), 0, s, g, st, a); break;
    default: hipLaunchKernelGGL(sc_cbwd_kernel, dim3(grid), dim3(WG), 0, s, g, st, a); break;
    }
}

// The checks of both patterns and the opening state, enqueued on `s` behind sc_check_rows_kernel of A (the caller's, which may have read it back).
int enqueue_open(int n, const Arrays &g, ScState *st, int hub_cap, int cus, const StepArgs &a, Counts *cnt, hipStream_t s)
{
    const int g_rows = grid_rows(n, cus), g_ids = grid_for<WG>(n, 2048);
    hipLaunchKernelGGL(sc_check_rows_kernel, dim3(g_rows), dim3(WG), 0, s, n, g.trp, 1, st);
    hipLaunchKernelGGL(sc_open_kernel, dim3(g_rows), dim3(WG), 0, s, n, g, st);
    hipLaunchKernelGGL(sc_open_ids_kernel, dim3(g_ids), dim3(WG), 0, s, n, hub_cap, 0, g.rp, g.ci, g.dout, g.whub[0], st);
    hipLaunchKernelGGL(sc_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, hub_cap, 0, g.rp, g.ci, g.dout, g.whub[0], st);
    hipLaunchKernelGGL(sc_open_ids_kernel, dim3(g_ids), dim3(WG), 0, s, n, hub_cap, 1, g.trp, g.tci, g.din, g.whub[1], st);
    hipLaunchKernelGGL(sc_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, hub_cap, 1, g.trp, g.tci, g.din, g.whub[1], st);
    hipLaunchKernelGGL(sc_scan_kernel, dim3(grid_for<WG>(n, cus)), dim3(WG), 0, s, g, st, a);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 7;
    return G4S_OK;
}

// The labelling on device arrays behind the opening pass; returns behind a wait on `s` with *h the final state.
int run(int n, const Arrays &g, ScState *st, int hub_cap, int cus, ScState *h, Counts *cnt, hipStream_t s)
{
    // G4S_SCC_MIN_GRID is an A/B switch: the outputs do not depend on it. The kernels over all vertices end in one ticket per workgroup
    // on one word, so their grid stays at one workgroup per CU at most (kcore.hip's scan).
    const StepGrid sized(env_int("G4S_SCC_MIN_GRID", kMinGrid, 1, 2 * cus), 2 * cus);
    const int g_scan = grid_for<WG>(n, cus);
    StepArgs a;
    a.grid_cap = LLONG_MAX;
    a.n = n;
    a.hub_cap = hub_cap;
    a.resume = 0;
    G4S_TRY(enqueue_open(n, g, st, hub_cap, cus, a, cnt, s));

    ReadScope reads(s);
    bool know = false;                                             // *h is the device's state
    int batch = kBatch, last_phase = -1;
    for (;;) {
        const int grid = know ? sized.grid(h->work_cur) : sized.max_grid;
        a.grid_cap = sized.cap(grid);
        // the phase last seen, for half the batch when it is stepped (all of it when two reads in a row saw it); then what usually follows
        int ph = know ? h->phase : SC_PEEL;
        bool pivot_done = know && h->pivot_done;
        int left = !stepped(ph) ? 1 : ph == last_phase ? batch : std::max(kReps, batch / 2);
        for (int b = 0; b < batch; ++b) {
            a.resume = b == 0 && know && h->stop == 4;
            launch(ph, grid, g_scan, g, st, a, s);
            if (--left == 0) {
                pivot_done = pivot_done || ph == SC_LABEL;
                ph = guess_next(ph, pivot_done);
                left = stepped(ph) ? kReps : 1;
            }
        }
        a.resume = 0;
        G4S_HIP_TRY(hipGetLastError());
        cnt->launches += batch;
        if (know && h->stop == 4) cnt->resumes += 1;
        last_phase = know ? h->phase : -1;
        const ScState before = *h;
        G4S_HIP_TRY(reads.fetch(*h, st));
        cnt->waits += 1;
        if (h->invalid || h->stop == 1) break;
        // every kernel that runs turns a page, and the first launch of a batch is the kernel of the phase last seen: a batch that changed nothing cannot be
        if (know && memcmp(&before, h, sizeof(ScState)) == 0) return g4s::set_error(G4S_ERR_HIP, "g4s_strongly_connected_components: internal: a batch of %d launches made no step in phase %d", batch, h->phase);
        if (know) batch = sized.next_batch(batch);
        know = true;
    }
    if (h->invalid) return G4S_OK;
    const int g_rows = grid_for<WG>(n, 8192);
    hipLaunchKernelGGL(sc_zero_kernel, dim3(g_rows), dim3(WG), 0, s, n, g.din, st);
    hipLaunchKernelGGL(sc_count_kernel, dim3(g_rows), dim3(WG), 0, s, n, g.labels, g.din, st);
    hipLaunchKernelGGL(sc_largest_kernel, dim3(g_rows), dim3(WG), 0, s, n, g.labels, g.din, st);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 3;
    G4S_HIP_TRY(reads.fetch(*h, st));
    cnt->waits += 1;
    return G4S_OK;
}

const char *invalid_text(int bits)
{
    // bits 1 and 2 are the opening pass's on A (csr_invalid_text), 4 and 8 the same two on Aᵀ
    return (bits & 1) ? csr_invalid_text(1) : (bits & 4) ? "trowptr must start at 0 and never decrease"
         : (bits & 16) ? "trowptr[n] differs from rowptr[n]" : (bits & 2) ? csr_invalid_text(2) : "a column id of the transpose is outside [0, n)";
}

} // namespace

G4S_API g4s_status g4s_strongly_connected_components(int32_t n, const int32_t *rowptr, const int32_t *colids, const int32_t *trowptr, const int32_t *tcolids,
                                                     int32_t *labels, unsigned flags, g4s_scc_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr && labels, "rowptr or labels is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    G4S_REQUIRE((trowptr == nullptr) == (tcolids == nullptr), "trowptr and tcolids come together: both given or both NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0, build = trowptr == nullptr;
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        const long long tnnz = build ? 0 : trowptr[n];
        G4S_REQUIRE(tnnz >= 0, "trowptr[n] is negative");
        const size_t nb = sizeof(int32_t) * (size_t)n;
        const Span outs[] = {{labels, nb}}, ins[] = {{rowptr, nb + sizeof(int32_t)}, {colids, sizeof(int32_t) * (size_t)nnz},
                                                     {trowptr, nb + sizeof(int32_t)}, {tcolids, sizeof(int32_t) * (size_t)tnnz}};
        G4S_REQUIRE(!any_overlap(outs, ins), "labels must not overlap the inputs");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) *info = g4s_scc_info{};
    if (info) info->pivot = -1;
    if (n == 0) return G4S_OK;

    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const int hub_cap = std::min(n, kHubCap);
    ScState *st, h{};
    Arrays g{};
    Carver work;
    work.piece(&st, kStateBytes);
    for (int **p : {&g.din, &g.dout, &g.queue, &g.colour, &g.stamp, &g.wq[0], &g.wq[1]}) work.piece(p, sizeof(int) * (size_t)n);
    for (int **p : {&g.whub[0], &g.whub[1], &g.hub_a}) work.piece(p, sizeof(int) * (size_t)hub_cap);
    work.tail(&g.hub_t, sizeof(int) * (size_t)hub_cap);
    Staged stage(s);
    BigBuf t_rp, t_ci;                                             // the transpose, when the call builds it
    Counts cnt;
    int status = work.alloc();
    g.rp = rowptr; g.ci = colids; g.trp = trowptr; g.tci = tcolids; g.labels = labels;
    if (status == G4S_OK && !device) {
        g.rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        g.ci = stage.in(colids, sizeof(int) * (size_t)nnz);
        if (!build) {
            g.trp = stage.in(trowptr, sizeof(int) * ((size_t)n + 1));
            g.tci = stage.in(tcolids, sizeof(int) * (size_t)trowptr[n]);
        }
        g.labels = stage.out<int>(sizeof(int) * (size_t)n);
        status = stage.error();
    }
    auto hip_ok = [](hipError_t e, const char *what) { return e == hipSuccess ? G4S_OK : g4s::set_error(G4S_ERR_HIP, "g4s_strongly_connected_components: %s: %s", what, hipGetErrorString(e)); };
    if (status == G4S_OK) status = hip_ok(hipMemsetAsync(st, 0, kStateBytes, s), "hipMemsetAsync");
    if (status == G4S_OK) {
        hipLaunchKernelGGL(sc_check_rows_kernel, dim3(grid_rows(n, cus)), dim3(WG), 0, s, n, g.rp, 0, st);
        status = hip_ok(hipGetLastError(), "launch");
        cnt.launches += 1;
    }
    if (status == G4S_OK && build) {
        // the row pointers are read back before anything is sized by rowptr[n]; the library's own transpose then checks the ids itself
        status = hip_ok(ReadScope(s).fetch(h, st), "read");
        cnt.waits += 1;
        if (status == G4S_OK && !h.invalid) {
            nnz = h.nnz[0];
            status = t_rp.alloc(sizeof(int) * ((size_t)n + 1));
            if (status == G4S_OK) status = t_ci.alloc(sizeof(int) * (size_t)std::max(nnz, 1LL));
            if (status == G4S_OK)
                status = g4s_csr_transpose(n, n, nnz, g.rp, g.ci, nullptr, t_rp.as<int32_t>(), t_ci.as<int32_t>(), nullptr, nullptr, G4S_DEVICE_POINTERS, s);
            cnt.waits += 2;                                        // its verdict, its end
            g.trp = t_rp.as<int>();
            g.tci = t_ci.as<int>();
        }
    }
    if (status == G4S_OK && !h.invalid) status = run(n, g, st, hub_cap, cus, &h, &cnt, s);
    if (status == G4S_OK && !device && !h.invalid) {
        status = stage.to_host(labels, g.labels, sizeof(int) * (size_t)n);
        if (status == G4S_OK) status = stage.wait();
        cnt.waits += 1;
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    work.idle();
    t_rp.idle = t_ci.idle = true;
    if (status == G4S_OK && h.invalid) status = g4s::set_error(G4S_ERR_INVALID, "g4s_strongly_connected_components: %s", invalid_text(h.invalid));
    if (status == G4S_OK && info) {
        info->components = (int64_t)h.components;
        info->largest = (int64_t)(h.best >> 32);
        info->edges_walked = (int64_t)h.edges_walked;
        info->largest_label = INT_MAX - (int32_t)(h.best & 0xffffffffull);
        info->trimmed = h.trimmed;
        info->pivot = h.pivot_done ? h.pivot : -1;
        info->pivot_size = h.pivot_size;
        info->color_rounds = h.color_rounds;
        info->launches = cnt.launches;
        info->resumes = cnt.resumes;
        info->host_waits = cnt.waits;
        info->built_transpose = build ? 1 : 0;
    }
    return status;
}
