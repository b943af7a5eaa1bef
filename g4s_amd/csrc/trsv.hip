// trsv.hip — g4s_sptrsv_* (include/g4s.h): a level-scheduled sparse triangular solve on the lower or upper triangle of an n × n CSR. DESIGN §4.20.
//
// The analysis is paid once. It is a Kahn peel of the dependency DAG on the stepped driver of the graph calls (frontier.hpp, step_batch.hpp), the
// pred-count peel of color.hip on another DAG: row i depends on column c for every stored off-diagonal entry (i, c) of the triangle.
//   open     tr_open_rows_kernel: rowptr[0] == 0, non-decreasing. tr_open_ids_kernel / tr_open_hubs_kernel (return at once when the rows were bad):
//            ids in [0, n); per triangle entry (u, v): v == u counts in dcnt[u], else in ocnt[u] and in tcnt[v], the length of row v of the transposed
//            pattern. tr_count_kernel: the totals and the smallest row without a diagonal. One read of the state: a refusal ends here.
//   pattern  tptr = scan(tcnt); tr_scatter_kernel walks A once more and writes row u behind a cursor of column v: the rows that wait for v, in any
//            order (the order decides which lane appends a row, never a level).
//   peel     tr_seed_kernel: pred[i] = ocnt[i], the rows with pred == 0 are frontier 0 (level 0). tr_step_kernel: the frontier walk over the
//            frontier's rows of the transposed pattern; per entry v → w one atomicSub on pred[w]; the lane that sees 1 appends w and writes
//            level[w] = the step's index + 1. One launch per level; kBatch (doubling to kBatchMax) launches behind one read of the state.
//   layout   a stable radix sort of the rows by level (prims.hpp) gives the (level, id) order; a histogram and a scan the level offsets; a scan of
//            the row lengths the entry offsets; tr_gather_kernel (one wave per row, ballots keep the stored order) writes each row's off-diagonal
//            entries and behind them its diagonal entries, with the position map update_values refreshes them through.
// The solve enqueues the launch list (for_each_launch, level_schedule.hpp) and waits for nothing. Every launch solves whole levels, so a row reads only
// x values written behind a kernel boundary or — inside a chain — by its own workgroup behind a fence and a barrier: the frame and its memory model
// are level_tile.hpp's (deal_tile, for_chain_levels, ld_prior), shared with ilu.hip. No wave waits for another workgroup; nothing spins.
// The arithmetic shape of a row (g4s.h) depends on its own entry count alone: solve_tile is the one place that computes it, for both kernels and for
// both entry points. g4s_sptrsv_solve_multi solves a block of k right-hand sides on the same launch list: the solve is written over the
// right-hand sides' type — RhsVector, a tile of one column, or RhsBlock<kCol>, a tile of G4S_TRSV_RHS_TILE columns per workgroup — and
// tr_level_kernel and tr_chain_kernel are instantiated for each.
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "prims.hpp"
#include "trsv.hpp"
#include "level_tile.hpp"
#include <algorithm>
#include <climits>
#include <new>

struct g4s_trsv_s {
    int n = 0;                          // first: the refusals of g4s_sptrsv_solve_multi read nothing else (tests/test_trsv_multi_cpu.py asks them of a bare n)
    unsigned flags = 0;
    long long nnz_in = 0;               // entries of the arrays the handle was analysed from: what update_values reads
    long long nnz_tri = 0;
    g4s::DevBuf block;                  // the (level, row) layout, one allocation
    int *ebeg = nullptr, *noff = nullptr, *lcol = nullptr, *emap = nullptr;
    double *diag = nullptr, *lval = nullptr;
    g4s::LevelSchedule sched;           // rowid and loff point into the block
    g4s_trsv_info info{};
};

namespace {

using g4s::TrState;

constexpr int kBatch = 16;                    // step launches behind one state read, at least; doubles up to g4s::kBatchMax (step_batch.hpp)
constexpr int kWaveRow = G4S_TRSV_WAVE_ROW;
constexpr size_t kStateBytes = 256;
constexpr unsigned kFlagMask = G4S_DEVICE_POINTERS | G4S_TRSV_UPPER | G4S_TRSV_UNIT_DIAGONAL | G4S_TRSV_NO_CHAINS;
static_assert(sizeof(TrState) <= kStateBytes, "state block");

enum { KIND_SEED = 0, KIND_STEP = 1 };

struct StepArgs {
    long long grid_cap;    // a frontier with more entries than this asks for a larger grid
    int n;
    int hub_cap;
    int resume;            // the first step of a batch goes on from stop == 4
};

__device__ __forceinline__ bool in_triangle(int upper, int u, int v) { return upper ? v >= u : v <= u; }

// ------------------------------------------------------------------------------------------------------------------------------ the analysis
__global__ __launch_bounds__(WG) void tr_open_rows_kernel(int n, const int *__restrict__ rowptr, TrState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [](long long, int, int) {});
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->bad_row = n;
        st->nnz_in = rowptr[n];                                    // means something only on a valid rowptr, and is used only then
    }
}

struct Counting {
    int upper, unit;
    int *ocnt, *dcnt, *tcnt;
    __device__ void operator()(int, int u, int v) const
    {
        if (!in_triangle(upper, u, v)) return;
        if (v == u) { if (!unit) atomicAdd(dcnt + u, 1); }
        else { atomicAdd(ocnt + u, 1); atomicAdd(tcnt + v, 1); }
    }
};

__global__ __launch_bounds__(WG) void tr_open_ids_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *__restrict__ hubs,
                                                         TrState *st, const Counting c)
{
    if (st->invalid) return;                                       // rowptr is monotone from 0 beyond this line: [0, rowptr[n]) is the colids array
    open_ids<false>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_open, &st->invalid, 2, c);
}

__global__ __launch_bounds__(WG) void tr_open_hubs_kernel(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids,
                                                          const int *__restrict__ hubs, TrState *st, const Counting c)
{
    if (st->invalid) return;
    open_hubs<false>(n, hub_cap, rowptr, colids, hubs, &st->n_hub_open, &st->invalid, 2, c);
}

// the totals, and the smallest row that stores no diagonal entry (unit: dcnt is all zero and nobody asks)
__global__ __launch_bounds__(WG) void tr_count_kernel(int n, int unit, const int *__restrict__ ocnt, const int *__restrict__ dcnt, TrState *st)
{
    if (st->invalid) return;
    long long so = 0, sd = 0;
    int bad = n;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        const int d = dcnt[i];
        so += ocnt[i];
        sd += d;
        if (!unit && d == 0 && (int)i < bad) bad = (int)i;
    }
    so = wave_sum(so);
    sd = wave_sum(sd);
    bad = wave_min(bad);
    if ((threadIdx.x & 63) == 0) {
        if (so) atomicAdd(&st->nnz_off, (unsigned long long)so);
        if (sd) atomicAdd(&st->nnz_diag, (unsigned long long)sd);
        if (bad < n) atomicMin(&st->bad_row, bad);
    }
}

// The transposed pattern: row u behind column v's cursor, for every off-diagonal entry (u, v) of the triangle. The hub list is the opening pass's.
__global__ __launch_bounds__(WG) void tr_scatter_kernel(int n, int hub_cap, int upper, const int *__restrict__ rowptr, const int *__restrict__ colids,
                                                        const int *__restrict__ hubs, const int *__restrict__ tptr, int *fill, int *__restrict__ trows,
                                                        const TrState *st)
{
    auto entry = [&](bool valid, int k, int u) {
        if (!valid) return;
        const int v = colids[k];
        if (v != u && in_triangle(upper, u, v)) trows[tptr[v] + atomicAdd(fill + v, 1)] = u;
    };
    walk_tiles<int>(n, [&](int i, int &start, int &len, int &u) {
        const int rb = rowptr[i], l = rowptr[i + 1] - rb;
        if (l > kHubCut) return;
        u = i;
        start = rb;
        len = l;
    }, entry);
    walk_hubs<int>(st->n_hub_open < hub_cap ? st->n_hub_open : hub_cap, [&](int h, int &start, int &len, int &u) {
        u = hubs[h];
        start = rowptr[u];
        len = rowptr[u + 1] - start;
    }, entry);
}

// The end of the seed and of a step kernel: the block's share of the built frontier's entries, then the ticket; the last block to arrive turns the
// page (turn_page).
__device__ __forceinline__ void finish(TrState *st, long long len_sum, int kind, const StepArgs a)
{
    __shared__ long long s_len[WG / 64];
    len_sum = wave_sum(len_sum);
    if ((threadIdx.x & 63) == 0) s_len[threadIdx.x >> 6] = len_sum;
    if (!turn_page(&st->tickets, [&] {
        long long ls = 0;
        for (int w = 0; w < WG / 64; ++w) ls += s_len[w];
        if (ls) atomicAdd((unsigned long long *)&st->edges_next, (unsigned long long)ls);
    })) return;
    const QueueFlip f = flip_queue(st);
    if (kind == KIND_STEP && f.walked > 0) st->round += 1;
    st->stop = f.appended == 0 ? 1 : f.entries > a.grid_cap ? 4 : 0;
}

// Frontier 0: the rows that wait for nothing. Its page turn is a step's, without a round.
__global__ __launch_bounds__(WG) void tr_seed_kernel(const int *__restrict__ tptr, const int *__restrict__ ocnt, int *__restrict__ pred, int *__restrict__ level,
                                                     int *__restrict__ queue, int *hubs0, int *hubs1, TrState *st, const StepArgs a)
{
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0;
    for (long long i0 = (long long)blockIdx.x * WG; i0 < a.n; i0 += (long long)gridDim.x * WG) {
        const long long i = i0 + threadIdx.x;
        const int p = i < a.n ? ocnt[i] : -1;
        const bool want = p == 0;
        if (i < a.n) { pred[i] = p; level[i] = want ? 0 : -1; }
        const int len = want ? tptr[i + 1] - tptr[i] : 0;
        append_frontier(want, (int)i, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);   // appended once per call: the slot is below n
    }
    finish(st, len_sum, KIND_SEED, a);
}

__global__ __launch_bounds__(WG) void tr_step_kernel(const int *__restrict__ tptr, const int *__restrict__ trows, int *pred, int *level, int *queue, int *hubs0,
                                                     int *hubs1, TrState *st, const StepArgs a)
{
    if (!step_runs(st->stop, a.resume)) return;                    // the same word for every block
    const int r = st->round, head = st->head;
    const int *hubs_cur = st->hub_cur ? hubs1 : hubs0;
    int *hubs_next = st->hub_cur ? hubs0 : hubs1;
    long long len_sum = 0;
    auto entry = [&](bool valid, int k, int) {
        bool want = false;
        int w = 0, len = 0;
        if (valid) {
            w = trows[k];
            want = atomicSub(pred + w, 1) == 1;                    // the atomic alone decides who appends w
            if (want) {
                level[w] = r + 1;                                  // the last column w waited for is in frontier r
                len = tptr[w + 1] - tptr[w];
            }
        }
        append_frontier(want, w, len, a.n, a.hub_cap, queue, hubs_next, &st->tail, &st->n_hub_next, len_sum);
    };
    walk_tiles<int>(st->end - head, [&](int i, int &start, int &len, int &u) {
        u = queue[head + i];
        const int rb = tptr[u], l = tptr[u + 1] - rb;
        if (l > kHubCut) return;                                   // walked out of the hub list
        start = rb;
        len = l;
    }, entry);
    walk_hubs<int>(st->n_hub_cur < a.hub_cap ? st->n_hub_cur : a.hub_cap, [&](int h, int &start, int &len, int &u) {
        u = hubs_cur[h];
        start = tptr[u];
        len = tptr[u + 1] - start;
    }, entry);
    finish(st, len_sum, KIND_STEP, a);
}

// keys of the stable descending sort: the level reversed, so that level 0 comes first and ids ascend inside a level; the level histogram beside it
__global__ __launch_bounds__(WG) void tr_keys_kernel(int n, int levels, const int *__restrict__ level, int *__restrict__ keys, int *__restrict__ ids, int *lcnt)
{
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        const int l = level[i];
        keys[i] = levels - 1 - l;
        ids[i] = (int)i;
        atomicAdd(lcnt + l, 1);
    }
}

__global__ __launch_bounds__(WG) void tr_rowlen_kernel(int n, const int *__restrict__ rowid, const int *__restrict__ ocnt, const int *__restrict__ dcnt,
                                                       int *__restrict__ noff, int *__restrict__ tot)
{
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < n; p += (long long)gridDim.x * WG) {
        const int r = rowid[p], o = ocnt[r];
        noff[p] = o;
        tot[p] = o + dcnt[r];
    }
}

// lent[l] = the entry offset of level l's first row, l = 0 … levels: the host sizes a level's launch from its rows and its entries
__global__ __launch_bounds__(WG) void tr_level_entries_kernel(int levels, const int *__restrict__ loff, const int *__restrict__ ebeg, int *__restrict__ lent)
{
    for (int l = blockIdx.x * WG + threadIdx.x; l <= levels; l += gridDim.x * WG) lent[l] = ebeg[loff[l]];
}

// Row rowid[p] of A into the layout, one wave per row, 64 entries a trip: the off-diagonal entries of the triangle in stored order at ebeg[p], the
// diagonal entries in stored order behind them; diag[p] = their sum from the left (1.0 with a unit diagonal, which keeps none).
__global__ __launch_bounds__(WG) void tr_gather_kernel(int n, int upper, int unit, const int *__restrict__ rowptr, const int *__restrict__ colids,
                                                       const double *__restrict__ values, const int *__restrict__ rowid, const int *__restrict__ ebeg,
                                                       const int *__restrict__ noff, int *__restrict__ lcol, double *__restrict__ lval, int *__restrict__ emap,
                                                       double *__restrict__ diag)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (long long p = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6); p < n; p += (long long)gridDim.x * (WG / 64)) {
        const int r = rowid[p], rb = rowptr[r], re = rowptr[r + 1], e0 = ebeg[p], m = noff[p];
        int ob = 0, db = 0;
        double d = 1.0;
        for (int k0 = rb; k0 < re; k0 += 64) {
            const int k = k0 + lane;
            const bool valid = k < re;
            const int c = valid ? colids[k] : -1;
            const double v = valid ? values[k] : 0.0;
            const bool tri = valid && in_triangle(upper, r, c) && !(unit && c == r);
            const bool isd = tri && c == r, iso = tri && c != r;
            const unsigned long long mo = __ballot(iso);
            unsigned long long md = __ballot(isd);
            if (tri) {
                const int pos = iso ? e0 + ob + __popcll(mo & below) : e0 + m + db + __popcll(md & below);
                lcol[pos] = c;
                lval[pos] = v;
                emap[pos] = k;
            }
            ob += __popcll(mo);
            while (md) {                                           // the same for every lane: the diagonal entries of this trip, from the left
                const int j = __ffsll((long long)md) - 1;
                md &= md - 1;
                const double vj = __shfl(v, j);
                d = db == 0 ? vj : d + vj;
                db += 1;
            }
        }
        if (lane == 0) diag[p] = d;
    }
}

// New values through the position map: every kept entry, and every row's diagonal sum from the caller's array itself.
__global__ __launch_bounds__(WG) void tr_update_kernel(int n, long long nnz_tri, const double *__restrict__ values, const int *__restrict__ emap,
                                                       const int *__restrict__ ebeg, const int *__restrict__ noff, double *__restrict__ lval,
                                                       double *__restrict__ diag)
{
    for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < nnz_tri; e += (long long)gridDim.x * WG) lval[e] = values[emap[e]];
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < n; p += (long long)gridDim.x * WG) {
        const int d0 = ebeg[p] + noff[p], d1 = ebeg[p + 1];
        if (d0 == d1) continue;                                    // a unit diagonal keeps none
        double d = values[emap[d0]];
        for (int j = d0 + 1; j < d1; ++j) d = d + values[emap[j]];
        diag[p] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------- the solve
struct TrView {
    const int *rowid, *ebeg, *noff, *lcol, *loff;
    const double *diag, *lval;
    int unit;
};

// The right-hand sides of a solve, by value into the kernels: b and x, kTile columns a workgroup — a thread that owns a row owns it for a tile of
// columns, and an entry's column and value are loaded once for all of them —, the entries each row class loads ahead of its additions, and where an
// element lies. Column j of a block is solved as the vector is, bit for bit: every column's products are added in the order and the shape of its
// row's class, whatever kTile and the unrolls.
// A vector: one column and no leading dimension — element i is at [i], and nothing of a tile is left at run time.
struct RhsVector {
    static constexpr int kTile = 1, kLaneUnroll = 4, kWaveUnroll = 8, kHubUnroll = 8;
    const double *b;
    double *x;
    __device__ int tile_cols(int) const { return 1; }
    __device__ long long b_at(int i, int) const { return i; }
    __device__ long long x_at(int i, int) const { return i; }
    __device__ long long b_step() const { return 1; }
    __device__ long long x_step() const { return 1; }
};

// The n × k blocks B and X. Element (i, j) is at [i·ld + j], kCol: at [i + j·ld].
template <bool kCol>
struct RhsBlock {
    static constexpr int kTile = G4S_TRSV_RHS_TILE, kLaneUnroll = 2, kWaveUnroll = 4, kHubUnroll = 4;
    const double *b;
    double *x;
    long long ldb, ldx;
    int k;
    static __device__ long long at(long long ld, int i, int j) { return kCol ? (long long)i + (long long)j * ld : (long long)i * ld + j; }
    __device__ int tile_cols(int j0) const { return std::min(kTile, k - j0); }
    __device__ long long b_at(int i, int j) const { return at(ldb, i, j); }
    __device__ long long x_at(int i, int j) const { return at(ldx, i, j); }
    __device__ long long b_step() const { return kCol ? ldb : 1; }   // from a column to the next
    __device__ long long x_step() const { return kCol ? ldx : 1; }
};

// One lane's share of a row's sums: the entries first, first + kStride, … below m of the row whose entries begin at e, added left to right from +0.0;
// s[q] is the sum over the column of x whose element of row 0 is xq[q]. kUnroll entries are loaded before the first of them is added — a lane has one
// dependent pair of loads (the column, then x) per entry and column, and a hub row of 10⁵ entries is 400 such pairs per lane —; the additions keep
// their order, so the bits do not depend on kUnroll.
template <bool kChain, typename Rhs, int kStride, int kUnroll>
__device__ __forceinline__ void strided_sum(const TrView &T, const Rhs &R, const double *const (&xq)[Rhs::kTile], int e, int first, int m,
                                            double (&s)[Rhs::kTile])
{
#pragma unroll
    for (int q = 0; q < Rhs::kTile; ++q) s[q] = 0.0;
    int k = first;
    for (; k + (kUnroll - 1) * kStride < m; k += kUnroll * kStride) {
        int c[kUnroll];
        double v[kUnroll], y[kUnroll][Rhs::kTile];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) c[u] = T.lcol[e + k + u * kStride];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = T.lval[e + k + u * kStride];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
            for (int q = 0; q < Rhs::kTile; ++q) y[u][q] = ld_prior<kChain>(xq[q] + R.x_at(c[u], 0));
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
            for (int q = 0; q < Rhs::kTile; ++q) s[q] = s[q] + v[u] * y[u][q];
    }
    for (; k < m; k += kStride) {
        const int c = T.lcol[e + k];
        const double v = T.lval[e + k];
        double y[Rhs::kTile];
#pragma unroll
        for (int q = 0; q < Rhs::kTile; ++q) y[q] = ld_prior<kChain>(xq[q] + R.x_at(c, 0));
#pragma unroll
        for (int q = 0; q < Rhs::kTile; ++q) s[q] = s[q] + v * y[q];
    }
}

// Rows [lo, hi) of the layout, all of one level, dealt by deal_tile (level_tile.hpp), for the column tile `tile` of R; the owner of a row keeps its
// sums s through the three classes and writes its x. Who sums a row never changes how it is summed, per column:
//   m <= kWaveRow            the lane alone, left to right from +0.0
//   kWaveRow < m <= kHubCut  the row's wave: lane l takes entries l, l + 64, … left to right from +0.0, then the wave_sum ladder
//   m > kHubCut              the workgroup: thread t takes entries t, t + 256, …, a wave_sum ladder per wave, then ((w0 + w1) + w2) + w3
// s_part is [WG / 64][kTile]. xq repeats the tile's last column behind its kn columns (the same for every thread of the workgroup), so a lane never
// loads outside the block and the tail needs no branch; what it sums there is never stored.
// b and x may be the same array: row r is the only reader of b[r] and the only writer of x[r], column by column.
struct TrRow {
    int m, e;                                                      // off-diagonal entries, and where they begin
};

template <bool kChain, typename Rhs>
__device__ __forceinline__ void solve_tile(const TrView &T, int lo, int hi, int stride, const Rhs &R, int tile, int *s_hub, int *s_nh, double *s_part)
{
    constexpr int kTile = Rhs::kTile;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j0 = tile * kTile, kn = R.tile_cols(j0);
    const double *xq[kTile];
#pragma unroll
    for (int q = 0; q < kTile; ++q) xq[q] = R.x + R.x_at(0, j0 + std::min(q, kn - 1));
    double s[kTile];
#pragma unroll
    for (int q = 0; q < kTile; ++q) s[q] = 0.0;
    const int p = deal_tile<kWaveRow, kHubCut>(lo, hi, stride, s_hub, s_nh,
        [&](int p) { return TrRow{T.noff[p], T.ebeg[p]}; },
        [&](const TrRow &r) { strided_sum<kChain, Rhs, 1, Rhs::kLaneUnroll>(T, R, xq, r.e, 0, r.m, s); },
        [&](const TrRow &r, int j) {
            double part[kTile];
            strided_sum<kChain, Rhs, 64, Rhs::kWaveUnroll>(T, R, xq, __shfl(r.e, j), lane, __shfl(r.m, j), part);
#pragma unroll
            for (int q = 0; q < kTile; ++q) {
                const double w = __shfl(wave_sum(part[q]), 0);
                if (lane == j) s[q] = w;
            }
        },
        [&](const TrRow &r, int th) {
            double part[kTile];
            strided_sum<kChain, Rhs, WG, Rhs::kHubUnroll>(T, R, xq, r.e, t, r.m, part);
#pragma unroll
            for (int q = 0; q < kTile; ++q) {
                const double w = wave_sum(part[q]);
                if (lane == 0) s_part[wave * kTile + q] = w;
            }
            __syncthreads();
            if (t == th) {
#pragma unroll
                for (int q = 0; q < kTile; ++q) s[q] = ((s_part[q] + s_part[kTile + q]) + s_part[2 * kTile + q]) + s_part[3 * kTile + q];
            }
        });
    if (p >= 0) {
        const int r = T.rowid[p];
        const double d = T.unit ? 1.0 : T.diag[p];
        const double *bp = R.b + R.b_at(r, j0);
        double *xp = R.x + R.x_at(r, j0);
#pragma unroll
        for (int q = 0; q < kTile; ++q) {
            if (q < kn) {
                double v = *bp - s[q];
                if (!T.unit) v = v / d;
                *xp = canonical_nan(v);
            }
            bp += R.b_step();                                      // the next column; never dereferenced behind the tile
            xp += R.x_step();
        }
    }
}

// one level that is not in a chain: a tile of WG / stride rows (blockIdx.x) times a tile of columns (blockIdx.y) per workgroup
template <typename Rhs>
__global__ __launch_bounds__(WG) void tr_level_kernel(const TrView T, int lo, int hi, int stride, const Rhs R)
{
    __shared__ int s_hub[WG], s_nh;
    __shared__ double s_part[(WG / 64) * Rhs::kTile];
    const int2 tile = level_tile_bounds(lo, hi, stride);
    solve_tile<false>(T, tile.x, tile.y, stride, R, (int)blockIdx.y, s_hub, &s_nh, s_part);
}

// a chain: one workgroup per column tile (blockIdx.x), levels [level_lo, level_hi), each at most WG rows; a later level reads what an earlier one
// stored (for_chain_levels). Nobody else reads or writes a tile's columns: the memory model holds per workgroup, and no workgroup waits for another.
template <typename Rhs>
__global__ __launch_bounds__(WG) void tr_chain_kernel(const TrView T, int level_lo, int level_hi, const Rhs R)
{
    __shared__ int s_hub[WG], s_nh;
    __shared__ double s_part[(WG / 64) * Rhs::kTile];
    const int tile = (int)blockIdx.x;
    for_chain_levels(T.loff, level_lo, level_hi, [&](int lo, int hi, int stride) { solve_tile<true>(T, lo, hi, stride, R, tile, s_hub, &s_nh, s_part); });
}

// The launch list of the plan for the k columns of R: the column tiles are blockIdx.y of a level launch and the workgroups of a chain.
template <typename Rhs>
int enqueue(const g4s_trsv_s *T, const Rhs &R, int k, hipStream_t s)
{
    const TrView V{T->sched.rowid, T->ebeg, T->noff, T->lcol, T->sched.loff, T->diag, T->lval, (T->flags & G4S_TRSV_UNIT_DIAGONAL) != 0};
    const unsigned tiles = (unsigned)((k + Rhs::kTile - 1) / Rhs::kTile);
    g4s::for_each_launch(T->sched, g4s::trsv_stride,
        [&](int level_lo, int level_hi) { hipLaunchKernelGGL(tr_chain_kernel<Rhs>, dim3(tiles), dim3(WG), 0, s, V, level_lo, level_hi, R); },
        [&](int lo, int hi, int stride, int grid) { hipLaunchKernelGGL(tr_level_kernel<Rhs>, dim3((unsigned)grid, tiles), dim3(WG), 0, s, V, lo, hi, stride, R); });
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

int bits_of(int v)
{
    int b = 1;
    while (b < 31 && (v >> b) != 0) ++b;
    return b;
}

struct Work {
    TrState *st;
    int *ocnt, *dcnt, *tcnt, *hubs_open;
    int *trows, *tptr, *fill, *pred, *level, *queue, *hubs[2], *keys, *keys_out, *tmpk, *tmpv, *ids, *lcnt, *tot;
};

// Opening pass and the counts; returns behind a wait on `s` with *h the state.
int open(int n, const int *rowptr, const int *colids, int upper, int unit, const Work &w, int hub_cap, int cus, TrState *h, Counts *cnt, hipStream_t s)
{
    const Counting c{upper, unit, w.ocnt, w.dcnt, w.tcnt};
    const int g_rows = grid_rows(n, cus);
    G4S_HIP_TRY(hipMemsetAsync(w.st, 0, kStateBytes, s));
    G4S_HIP_TRY(hipMemsetAsync(w.ocnt, 0, sizeof(int) * (size_t)n, s));
    G4S_HIP_TRY(hipMemsetAsync(w.dcnt, 0, sizeof(int) * (size_t)n, s));
    G4S_HIP_TRY(hipMemsetAsync(w.tcnt, 0, sizeof(int) * ((size_t)n + 1), s));
    hipLaunchKernelGGL(tr_open_rows_kernel, dim3(g_rows), dim3(WG), 0, s, n, rowptr, w.st);
    hipLaunchKernelGGL(tr_open_ids_kernel, dim3(grid_for<WG>(n, 2048)), dim3(WG), 0, s, n, hub_cap, rowptr, colids, w.hubs_open, w.st, c);
    hipLaunchKernelGGL(tr_open_hubs_kernel, dim3(1024), dim3(WG), 0, s, n, hub_cap, rowptr, colids, w.hubs_open, w.st, c);
    hipLaunchKernelGGL(tr_count_kernel, dim3(g_rows), dim3(WG), 0, s, n, unit, w.ocnt, w.dcnt, w.st);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 4;
    G4S_HIP_TRY(g4s::ReadScope(s).fetch(*h, w.st));
    cnt->waits += 1;
    return G4S_OK;
}

// The transposed pattern and the peel; returns behind a wait on `s` with *h the final state: h->round levels, level[] complete.
int peel(int n, const int *rowptr, const int *colids, int upper, const Work &w, int hub_cap, int cus, TrState *h, Counts *cnt, hipStream_t s)
{
    const g4s::StepGrid sized(g4s::kMinGrid, 2 * cus);
    const int g_rows = grid_rows(n, cus);
    StepArgs a;
    a.grid_cap = LLONG_MAX;                                        // the seed stops nothing: the first grid is sized behind it
    a.n = n;
    a.hub_cap = hub_cap;
    a.resume = 0;
    G4S_TRY(g4s::prims::exclusive_scan(w.tcnt, w.tptr, (long long)n + 1, s));
    G4S_HIP_TRY(hipMemsetAsync(w.fill, 0, sizeof(int) * (size_t)n, s));
    hipLaunchKernelGGL(tr_scatter_kernel, dim3(grid_for<WG>(n, 2048)), dim3(WG), 0, s, n, hub_cap, upper, rowptr, colids, w.hubs_open, w.tptr, w.fill, w.trows, w.st);
    hipLaunchKernelGGL(tr_seed_kernel, dim3(g_rows), dim3(WG), 0, s, w.tptr, w.ocnt, w.pred, w.level, w.queue, w.hubs[0], w.hubs[1], w.st, a);
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 5;                                            // the scan counts as three
    g4s::ReadScope reads(s);
    G4S_HIP_TRY(reads.fetch(*h, w.st));
    cnt->waits += 1;
    int batch = kBatch;
    while (h->stop != 1) {
        const int grid = sized.grid(h->edges_cur + (h->end - h->head) + h->n_hub_cur);
        const bool resumed = h->stop == 4;
        a.grid_cap = sized.cap(grid);
        if (resumed) cnt->resumes += 1;
        for (int b = 0; b < batch; ++b) {
            a.resume = b == 0 && resumed;
            hipLaunchKernelGGL(tr_step_kernel, dim3(grid), dim3(WG), 0, s, w.tptr, w.trows, w.pred, w.level, w.queue, w.hubs[0], w.hubs[1], w.st, a);
        }
        a.resume = 0;
        G4S_HIP_TRY(hipGetLastError());
        cnt->launches += batch;
        G4S_HIP_TRY(reads.fetch(*h, w.st));
        cnt->waits += 1;
        batch = sized.next_batch(batch);
    }
    return G4S_OK;
}

// The (level, row) layout into the handle's arrays, and the level offsets and the levels' entry offsets to the host; returns behind a wait on `s`.
int layout(g4s_trsv_s *T, int levels, const int *rowptr, const int *colids, const double *values, int upper, int unit, const Work &w, int cus, Counts *cnt,
           hipStream_t s)
{
    g4s::LevelSchedule &S = T->sched;
    const int n = T->n, g_rows = grid_rows(n, cus);
    G4S_HIP_TRY(hipMemsetAsync(w.lcnt, 0, sizeof(int) * ((size_t)levels + 1), s));
    G4S_HIP_TRY(hipMemsetAsync(w.tot + n, 0, sizeof(int), s));
    hipLaunchKernelGGL(tr_keys_kernel, dim3(g_rows), dim3(WG), 0, s, n, levels, w.level, w.keys, w.ids, w.lcnt);
    G4S_TRY(g4s::prims::sort_pairs_descending(w.keys, w.ids, w.keys_out, S.rowid, w.tmpk, w.tmpv, n, bits_of(levels - 1), s));
    G4S_TRY(g4s::prims::exclusive_scan(w.lcnt, S.loff, (long long)levels + 1, s));
    hipLaunchKernelGGL(tr_rowlen_kernel, dim3(g_rows), dim3(WG), 0, s, n, S.rowid, w.ocnt, w.dcnt, T->noff, w.tot);
    G4S_TRY(g4s::prims::exclusive_scan(w.tot, T->ebeg, (long long)n + 1, s));
    hipLaunchKernelGGL(tr_gather_kernel, dim3(grid_for<WG / 64>(n, 16LL * cus)), dim3(WG), 0, s, n, upper, unit, rowptr, colids, values, S.rowid, T->ebeg, T->noff,
                       T->lcol, T->lval, T->emap, T->diag);
    G4S_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tr_level_entries_kernel, dim3(grid_for<WG>((long long)levels + 1, 64)), dim3(WG), 0, s, levels, S.loff, T->ebeg, w.lcnt);   // lcnt is free again
    G4S_HIP_TRY(hipGetLastError());
    cnt->launches += 4 + 3 * ((bits_of(levels - 1) + 3) / 4) + 6;  // a scan counts as three, a sort pass as three
    S.loff_host.resize((size_t)levels + 1);
    S.lent_host.resize((size_t)levels + 1);
    G4S_HIP_TRY(hipMemcpyAsync(S.loff_host.data(), S.loff, sizeof(int) * ((size_t)levels + 1), hipMemcpyDeviceToHost, s));
    G4S_HIP_TRY(hipMemcpyAsync(S.lent_host.data(), w.lcnt, sizeof(int) * ((size_t)levels + 1), hipMemcpyDeviceToHost, s));
    G4S_HIP_TRY(hipStreamSynchronize(s));
    cnt->waits += 1;
    return G4S_OK;
}

// the launch list from the level offsets on the host, and what the info says of it
void plan_launches(g4s_trsv_s *T, int levels)
{
    g4s::LevelSchedule &S = T->sched;
    const int *loff = S.loff_host.data();
    S.levels = levels;
    S.launches = g4s::trsv_launches(loff, levels, G4S_TRSV_CHAIN_WIDTH, G4S_TRSV_CHAIN_LEVELS, (T->flags & G4S_TRSV_NO_CHAINS) != 0);
    int widest = 0, chains = 0;
    for (int l = 0; l < levels; ++l) widest = std::max(widest, loff[l + 1] - loff[l]);
    for (const g4s::TrLaunch &L : S.launches) chains += L.chain;
    T->info.levels = levels;
    T->info.widest_level = widest;
    T->info.launches_per_solve = (int)S.launches.size();
    T->info.chains = chains;
}

} // namespace

const g4s::LevelSchedule &g4s::trsv_schedule(const g4s_trsv_s *T) { return T->sched; }

G4S_API g4s_status g4s_sptrsv_analyse(g4s_trsv_t *out, int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values, int32_t *level,
                                      unsigned flags, g4s_trsv_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~kFlagMask) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and the G4S_TRSV_* bits");
    G4S_REQUIRE(out, "out is NULL");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    G4S_REQUIRE((colids && values) || n == 0, "colids or values is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    const int upper = (flags & G4S_TRSV_UPPER) != 0, unit = (flags & G4S_TRSV_UNIT_DIAGONAL) != 0;
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        const size_t nb = sizeof(int32_t) * (size_t)n;
        const Span outs[] = {{level, nb}}, ins[] = {{rowptr, nb + sizeof(int32_t)}, {colids, sizeof(int32_t) * (size_t)nnz}, {values, sizeof(double) * (size_t)nnz}};
        G4S_REQUIRE(!any_overlap(outs, ins), "level must not overlap the inputs");
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) { *info = g4s_trsv_info{}; info->n = n; info->bad_row = -1; }
    g4s_trsv_s *T = new (std::nothrow) g4s_trsv_s;
    if (!T) return g4s::set_error(G4S_ERR_NOMEM, "g4s_sptrsv_analyse: no memory for the handle");
    T->n = n;
    T->flags = flags;
    T->info.n = n;
    T->info.bad_row = -1;
    if (n == 0) {
        if (info) *info = T->info;
        *out = T;
        return G4S_OK;
    }

    int cus = 1;
    int status = G4S_OK;
    if (g4s::device_cus(&cus) != hipSuccess) status = g4s::set_error(G4S_ERR_HIP, "g4s_sptrsv_analyse: no device");
    const int hub_cap = std::min(n, kHubCap);
    TrState h{};
    Work w{};
    Carver first, second;
    first.piece(&w.st, kStateBytes);
    first.piece(&w.ocnt, sizeof(int) * (size_t)n);
    first.piece(&w.dcnt, sizeof(int) * (size_t)n);
    first.piece(&w.tcnt, sizeof(int) * ((size_t)n + 1));
    first.tail(&w.hubs_open, sizeof(int) * (size_t)hub_cap);
    Staged stage(s);
    Counts cnt;
    if (status == G4S_OK) status = first.alloc();
    const int *rp = rowptr, *ci = colids;
    const double *va = values;
    int *lv = level;
    if (status == G4S_OK && !device) {
        rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        ci = stage.in(colids, sizeof(int) * (size_t)nnz);
        va = stage.in(values, sizeof(double) * (size_t)nnz);
        status = stage.error();
    }
    if (status == G4S_OK) status = open(n, rp, ci, upper, unit, w, hub_cap, cus, &h, &cnt, s);
    const bool refused = status == G4S_OK && (h.invalid || h.bad_row < n);
    int levels = 0;
    if (status == G4S_OK && !refused) {
        const size_t ni = sizeof(int) * (size_t)n;
        second.piece(&w.trows, sizeof(int) * (size_t)h.nnz_off);
        second.piece(&w.tptr, ni + sizeof(int));
        second.piece(&w.fill, ni);
        second.piece(&w.pred, ni);
        second.piece(&w.level, ni);
        second.piece(&w.queue, ni);
        second.piece(&w.hubs[0], sizeof(int) * (size_t)hub_cap);
        second.piece(&w.hubs[1], sizeof(int) * (size_t)hub_cap);
        second.piece(&w.keys, ni);
        second.piece(&w.keys_out, ni);
        second.piece(&w.tmpk, ni);
        second.piece(&w.tmpv, ni);
        second.piece(&w.ids, ni);
        second.piece(&w.lcnt, ni + sizeof(int));
        second.tail(&w.tot, ni + sizeof(int));
        status = second.alloc();
        if (status == G4S_OK) status = peel(n, rp, ci, upper, w, hub_cap, cus, &h, &cnt, s);
        if (status == G4S_OK) {
            levels = h.round;
            T->nnz_in = device ? (long long)h.nnz_in : nnz;
            T->nnz_tri = (long long)(h.nnz_off + h.nnz_diag);
            const size_t nt = (size_t)T->nnz_tri;
            const size_t o_rowid = 0, o_ebeg = o_rowid + pad256(ni), o_noff = o_ebeg + pad256(ni + sizeof(int)), o_loff = o_noff + pad256(ni),
                         o_lcol = o_loff + pad256(sizeof(int) * ((size_t)levels + 1)), o_emap = o_lcol + pad256(sizeof(int) * nt),
                         o_diag = o_emap + pad256(sizeof(int) * nt), o_lval = o_diag + pad256(sizeof(double) * (size_t)n),
                         total = o_lval + pad256(sizeof(double) * nt);
            status = T->block.alloc(total);
            char *base = T->block.as<char>();
            T->sched.rowid = reinterpret_cast<int *>(base + o_rowid);
            T->ebeg = reinterpret_cast<int *>(base + o_ebeg);
            T->noff = reinterpret_cast<int *>(base + o_noff);
            T->sched.loff = reinterpret_cast<int *>(base + o_loff);
            T->lcol = reinterpret_cast<int *>(base + o_lcol);
            T->emap = reinterpret_cast<int *>(base + o_emap);
            T->diag = reinterpret_cast<double *>(base + o_diag);
            T->lval = reinterpret_cast<double *>(base + o_lval);
        }
        if (status == G4S_OK) status = layout(T, levels, rp, ci, va, upper, unit, w, cus, &cnt, s);
        if (status == G4S_OK && level) {
            if (!device) status = stage.to_host(level, w.level, ni);
            else if (hipMemcpyAsync(lv, w.level, ni, hipMemcpyDeviceToDevice, s) != hipSuccess) status = g4s::set_error(G4S_ERR_HIP, "g4s_sptrsv_analyse: the copy of level failed");
            if (status == G4S_OK) status = stage.wait();
            cnt.waits += 1;
        }
    }
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    first.idle();
    second.idle();
    if (status == G4S_OK && h.invalid)
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_sptrsv_analyse: %s", csr_invalid_text(h.invalid));
    if (status == G4S_OK && h.bad_row < n) {
        if (info) info->bad_row = h.bad_row;
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_sptrsv_analyse: row %d stores no diagonal entry in the triangle", h.bad_row);
    }
    if (status != G4S_OK) {
        delete T;
        return status;
    }
    plan_launches(T, levels);
    T->info.nnz_triangle = T->nnz_tri;
    T->info.launches = cnt.launches;
    T->info.host_waits = cnt.waits;
    T->info.resumes = cnt.resumes;
    if (info) *info = T->info;
    *out = T;
    return G4S_OK;
}

G4S_API g4s_status g4s_sptrsv_solve(g4s_trsv_t T, const double *b_dev, double *x_dev, void *stream)
{
    G4S_REQUIRE(T, "the handle is NULL");
    if (T->n == 0) return G4S_OK;
    G4S_REQUIRE(b_dev && x_dev, "b or x is NULL");
    return enqueue(T, RhsVector{b_dev, x_dev}, 1, g4s::as_stream(stream));
}

static_assert((G4S_TRSV_COL_MAJOR & (kFlagMask | G4S_ILU0_NO_CHAINS)) == 0u, "a bit of its own");
static_assert(G4S_TRSV_RHS_TILE >= 1 && (G4S_TRSV_MAX_RHS + G4S_TRSV_RHS_TILE - 1) / G4S_TRSV_RHS_TILE <= 65535, "the column tiles are a grid dimension");

G4S_API g4s_status g4s_sptrsv_solve_multi(g4s_trsv_t T, int32_t k, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx, unsigned flags,
                                          void *stream)
{
    G4S_REQUIRE(T, "the handle is NULL");
    const g4s::BlockCall call = g4s::check_block_call(__func__, T->n, k, "B", B_dev, ldb, "X", X_dev, ldx, flags);
    if (!call.go_on) return call.status;
    const hipStream_t s = g4s::as_stream(stream);
    if (flags & G4S_TRSV_COL_MAJOR) return enqueue(T, RhsBlock<true>{B_dev, X_dev, (long long)ldb, (long long)ldx, k}, k, s);
    return enqueue(T, RhsBlock<false>{B_dev, X_dev, (long long)ldb, (long long)ldx, k}, k, s);
}

G4S_API g4s_status g4s_sptrsv_update_values(g4s_trsv_t T, const double *values, unsigned flags, void *stream)
{
    G4S_REQUIRE(T, "the handle is NULL");
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    if (T->n == 0 || T->nnz_tri == 0) return G4S_OK;
    G4S_REQUIRE(values, "values is NULL");
    const hipStream_t s = g4s::as_stream(stream);
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const int grid = grid_rows(std::max<long long>(T->nnz_tri, T->n), cus);
    if (device) {
        hipLaunchKernelGGL(tr_update_kernel, dim3(grid), dim3(WG), 0, s, T->n, T->nnz_tri, values, T->emap, T->ebeg, T->noff, T->lval, T->diag);
        G4S_HIP_TRY(hipGetLastError());
        return G4S_OK;
    }
    G4S_TRY(not_capturing(__func__, s, "nothing back, but copies a host array in and waits for it"));
    Staged stage(s);
    const double *va = stage.in(values, sizeof(double) * (size_t)T->nnz_in);
    int status = stage.error();
    if (status == G4S_OK) {
        hipLaunchKernelGGL(tr_update_kernel, dim3(grid), dim3(WG), 0, s, T->n, T->nnz_tri, va, T->emap, T->ebeg, T->noff, T->lval, T->diag);
        if (hipGetLastError() != hipSuccess) status = g4s::set_error(G4S_ERR_HIP, "g4s_sptrsv_update_values: the launch failed");
    }
    if (status == G4S_OK) status = stage.wait();
    return stage.finish(status);
}

G4S_API g4s_status g4s_sptrsv_get_info(g4s_trsv_t T, g4s_trsv_info *info)
{
    G4S_REQUIRE(T && info, "the handle or info is NULL");
    *info = T->info;
    return G4S_OK;
}

G4S_API g4s_status g4s_sptrsv_destroy(g4s_trsv_t T)
{
    delete T;                                                      // hipFree waits for whatever still reads the layout
    return G4S_OK;
}
