// components.hip — g4s_connected_components (include/g4s.h): the weakly connected components of the graph whose edges are the stored entries of an
// n × n CSR pattern, as canonical labels (labels[v] = the smallest vertex id of v's component). A concurrent union-find forest in HBM in the shape
// of Afforest (Sutton, Ben-Nun, Barak 2018), written on this library's own building blocks; `labels` itself is the parent array.
//
//   open       cc_open_rows_kernel: rowptr[0] == 0, non-decreasing, parent[v] = v, count[v] = 0. cc_open_ids_kernel (returns at once when the rows
//              were bad, so no entry outside [0, rowptr[n]) is ever read): every column id in [0, n). From here on every kernel begins with
//              `if (st->invalid) return`, so an id is never dereferenced before it has been checked. Nothing is read back in between.
//   sample     round r = 0 … rounds − 1: vertex v links itself to its r-th stored neighbour; a compress after every round (without it the second
//              round walks the first round's chains: 1000 hops per vertex on the 1000 × 1000 grid).
//   link(u,v)  (link_from of union_find.hpp, shared with msf.hip) a, b = parent[u], parent[v]; while a != b: high / low = max / min; if parent[high] == low, done; if parent[high] == high, one
//              atomicCAS(parent + high, high, low) — done when it succeeds; otherwise go on from (parent[p], parent[low]) where p is what the load or
//              the FAILED CAS returned (p < high). parent[x] <= x always holds, so max(a, b) strictly decreases: at most `high` turns, no lane ever
//              waits for another, nothing spins. The smaller id wins every hook, so the final root is the minimum id: the canonical label.
//   compress   pointer jumping in passes with a kernel boundary between them: a pass moves every vertex 16 hops up (or to its root), which divides
//              every depth by 16, so 8 passes flatten any forest of fewer than 2^31 vertices. A pass in which every vertex saw its root leaves the
//              `pending` word of the next pass at zero and the remaining launches return at once: usually one pass does the work.
//   pick       one workgroup: the most frequent label among 1024 vertices at a fixed stride (ties: the smaller label) stays in a device word. With
//              G4S_CC_SYMMETRIC (and without G4S_CC_NO_SKIP) rows that carry it are skipped below; it is always the label counted by reduction.
//   link rest  entries r >= rounds of every row that is not skipped, on the frontier walk of frontier.hpp: a row above kHubCut remaining entries
//              goes to a hub list (cc_link_hubs_kernel). parent[row] is read once per row, once per chunk of a hub; after the compress
//              most links end at the first compare (one 4-byte gather per entry).
//   compress, then the statistics: roots, the size of the picked label by reduction, every other label by one atomicAdd per (wave, label), and
//              the largest component by a max over (size, −label).
// Memory model: the XCDs' L2s are not coherent for plain loads inside a kernel, so a read of parent[] may be stale. Parents only ever
// decrease along the tree, so a stale value is a FORMER ancestor: still in the same tree (exits on equality stay sound) and never too small; hooks are
// decided by the CAS alone, and after a failed CAS the descent goes on from the value it returned. Kernel boundaries are the only ordering between
// phases. Parent reads are relaxed atomic loads of wavefront scope: plain global loads that the compiler may neither tear nor assume race-free.
// One host wait per call: no decision is taken on the host between kernels (the picked label, the hub list and the error word stay on the device).
// Environment switches: G4S_CC_SAMPLE_ROUNDS (0 … 4, default 2), G4S_CC_NO_SKIP=1; every setting gives the same labels.
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "union_find.hpp"
#include <algorithm>
#include <climits>

namespace {

constexpr int kMaxRounds = 4;
constexpr int kRoundsDefault = 2;
constexpr int kCompressions = kMaxRounds + 1;
constexpr int kSamples = 1024;       // vertices looked at by the pick
constexpr size_t kStateBytes = 512;

struct CcState {
    int invalid;
    int big_label;                   // the picked label
    int skip;                        // 1: the link step skips the rows that carry it
    int n_hubs;
    unsigned long long edges_linked;
    unsigned long long components;
    unsigned long long best;         // (size << 32) | (INT_MAX − label): the maximum is the largest component, ties to the smaller label
    int pending[kCompressions * (kJumpPasses + 1)];
};
static_assert(sizeof(CcState) <= kStateBytes, "state block");

__global__ __launch_bounds__(WG) void cc_open_rows_kernel(int n, const int *__restrict__ rowptr, int *__restrict__ parent, int *__restrict__ count, CcState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [&](long long i, int, int) {
        parent[i] = (int)i;
        count[i] = 0;
    });
}

__global__ __launch_bounds__(WG) void cc_open_ids_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ colids, CcState *st)
{
    if (st->invalid) return;                                       // rowptr is monotone from 0 beyond this line: [0, rowptr[n]) is the colids array
    const long long nnz = rowptr[n];
    int bad = 0;
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) bad |= (unsigned)colids[k] >= (unsigned)n;
    if (bad) atomicOr(&st->invalid, 2);
}

__global__ __launch_bounds__(WG) void cc_sample_kernel(int n, int r, const int *__restrict__ rowptr, const int *__restrict__ colids, int *parent, const CcState *st)
{
    if (st->invalid) return;
    for (long long v = (long long)blockIdx.x * WG + threadIdx.x; v < n; v += (long long)gridDim.x * WG) {
        const int rb = rowptr[v];
        if (rowptr[v + 1] - rb > r) link_from(ld(parent + v), ld(parent + colids[rb + r]), parent);
    }
}

// One pass of pointer jumping. `slot`: this pass's word of st->pending; pass 0 of a compression always runs, a later one only if the pass before
// left a vertex short of its root. No link runs beside it.
__global__ __launch_bounds__(WG) void cc_jump_kernel(int n, int *parent, CcState *st, int slot, int first)
{
    if (st->invalid || (!first && !st->pending[slot])) return;
    if (jump_pass(n, parent)) atomicOr(&st->pending[slot + 1], 1);
}

__global__ __launch_bounds__(WG) void cc_pick_kernel(int n, const int *__restrict__ parent, CcState *st, int allow_skip)
{
    __shared__ int s_lab[kSamples];
    __shared__ unsigned long long s_red[WG / 64];
    if (st->invalid) return;
    const int ns = n < kSamples ? n : kSamples, t = (int)threadIdx.x;
    for (int i = t; i < ns; i += WG) s_lab[i] = parent[(long long)i * n / ns];
    __syncthreads();
    unsigned long long best = 0;
    for (int i = t; i < ns; i += WG) {
        const int l = s_lab[i];
        unsigned c = 0;
        for (int j = 0; j < ns; ++j) c += s_lab[j] == l;
        const unsigned long long key = ((unsigned long long)c << 32) | (unsigned)(INT_MAX - l);
        best = key > best ? key : best;
    }
    best = wave_max(best);
    if ((t & 63) == 0) s_red[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < WG / 64; ++w) best = s_red[w] > best ? s_red[w] : best;
        st->big_label = INT_MAX - (int)(best & 0xffffffffull);
        st->skip = allow_skip;
    }
}

__device__ __forceinline__ void add_linked(long long linked, CcState *st)
{
    __shared__ long long s_lk[WG / 64];
    linked = wave_sum(linked);
    if ((threadIdx.x & 63) == 0) s_lk[threadIdx.x >> 6] = linked;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_lk[w];
        if (sum) atomicAdd(&st->edges_linked, (unsigned long long)sum);
    }
}

// The entries from `rounds` on of every row that is not skipped, 256 rows per tile, lanes over the concatenated entries.
__global__ __launch_bounds__(WG) void cc_link_kernel(int n, int rounds, const int *__restrict__ rowptr, const int *__restrict__ colids, int *parent, int *__restrict__ hubs,
                                                     CcState *st)
{
    if (st->invalid) return;
    const int skip = st->skip, big = st->big_label;
    long long linked = 0;
    walk_tiles<int>(n, [&](int i, int &start, int &len, int &pu) {
        pu = ld(parent + i);
        if (skip && pu == big) return;
        const int rb = rowptr[i], rest = rowptr[i + 1] - rb - rounds;
        if (rest <= 0) return;
        if (rest > kHubCut) {
            const int h = atomicAdd(&st->n_hubs, 1);
            if (h < kHubCap) hubs[h] = i;                          // fewer than 2^31 / kHubCut such rows exist
            return;
        }
        start = rb + rounds;
        len = rest;
        linked += rest;
    }, [&](bool valid, int k, int pu) {
        if (valid) link_from(pu, ld(parent + colids[k]), parent);  // pu: an ancestor of the row's vertex, maybe a former one
    });
    add_linked(linked, st);
}

// Hub rows, by all workgroups; parent[u] is read again for every chunk.
__global__ __launch_bounds__(WG) void cc_link_hubs_kernel(int rounds, const int *__restrict__ rowptr, const int *__restrict__ colids, int *parent, const int *__restrict__ hubs,
                                                          CcState *st)
{
    if (st->invalid) return;
    long long linked = 0;
    walk_hubs<int>(st->n_hubs < kHubCap ? st->n_hubs : kHubCap, [&](int h, int &start, int &len, int &pu) {
        const int u = hubs[h];
        start = rowptr[u] + rounds;
        len = rowptr[u + 1] - start;                               // > kHubCut
        pu = ld(parent + u);
    }, [&](bool valid, int k, int pu) {
        if (!valid) return;
        link_from(pu, ld(parent + colids[k]), parent);
        linked += 1;
    });
    add_linked(linked, st);
}

// Roots, the size of the picked label (plain reduction) and of every other label (lanes of a wave that share a label issue one add).
__global__ __launch_bounds__(WG) void cc_count_kernel(int n, const int *__restrict__ labels, int *__restrict__ count, CcState *st)
{
    __shared__ long long s_red[2][WG / 64];
    if (st->invalid) return;
    const int big = st->big_label, lane = (int)threadIdx.x & 63;
    long long roots = 0, bigc = 0;
    for (long long v0 = (long long)blockIdx.x * WG; v0 < n; v0 += (long long)gridDim.x * WG) {
        const long long v = v0 + threadIdx.x;
        const bool valid = v < n;
        const int l = valid ? labels[v] : -1;
        roots += valid && l == v;
        bigc += valid && l == big;
        const bool act = valid && l != big;
        unsigned long long m = __ballot(act);                      // the same for every lane: the loop below is uniform
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const int lbl = __shfl(l, leader);
            const unsigned long long same = __ballot(act && l == lbl);
            if (lane == leader) atomicAdd(count + lbl, __popcll(same));
            m &= ~same;
        }
    }
    roots = wave_sum(roots), bigc = wave_sum(bigc);
    if (lane == 0) { s_red[0][threadIdx.x >> 6] = roots; s_red[1][threadIdx.x >> 6] = bigc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long r = 0, b = 0;
        for (int w = 0; w < WG / 64; ++w) { r += s_red[0][w]; b += s_red[1][w]; }
        if (r) atomicAdd(&st->components, (unsigned long long)r);
        if (b) atomicAdd(count + big, (int)b);
    }
}

__global__ __launch_bounds__(WG) void cc_largest_kernel(int n, const int *__restrict__ labels, const int *__restrict__ count, CcState *st)
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
// Enqueues the whole labelling on device arrays. `st` has room for kStateBytes, `count` for n ints, `hubs` for min(n, kHubCap).
int enqueue(int n, const int *rowptr, const int *colids, int *labels, bool symmetric, int rounds, bool no_skip, CcState *st, int *count, int *hubs, hipStream_t s)
{
    const int g = grid_for<WG>(n, 8192), g_edges = grid_for<WG>(n, 2048);
    int compression = 0;
    auto compress = [&]() {
        const int base = compression++ * (kJumpPasses + 1);
        for (int k = 0; k < kJumpPasses; ++k) hipLaunchKernelGGL(cc_jump_kernel, dim3(g), dim3(WG), 0, s, n, labels, st, base + k, k == 0);
    };
    G4S_HIP_TRY(hipMemsetAsync(st, 0, kStateBytes, s));
    hipLaunchKernelGGL(cc_open_rows_kernel, dim3(g), dim3(WG), 0, s, n, rowptr, labels, count, st);
    hipLaunchKernelGGL(cc_open_ids_kernel, dim3(8192), dim3(WG), 0, s, n, rowptr, colids, st);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(cc_sample_kernel, dim3(g), dim3(WG), 0, s, n, r, rowptr, colids, labels, st);
        compress();
    }
    hipLaunchKernelGGL(cc_pick_kernel, dim3(1), dim3(WG), 0, s, n, labels, st, symmetric && !no_skip ? 1 : 0);
    hipLaunchKernelGGL(cc_link_kernel, dim3(g_edges), dim3(WG), 0, s, n, rounds, rowptr, colids, labels, hubs, st);
    hipLaunchKernelGGL(cc_link_hubs_kernel, dim3(1024), dim3(WG), 0, s, rounds, rowptr, colids, labels, hubs, st);
    compress();
    hipLaunchKernelGGL(cc_count_kernel, dim3(g), dim3(WG), 0, s, n, labels, count, st);
    hipLaunchKernelGGL(cc_largest_kernel, dim3(g), dim3(WG), 0, s, n, labels, count, st);
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

int fetch_state(CcState *h, const CcState *st, hipStream_t s)
{
    G4S_HIP_TRY(g4s::ReadScope(s).fetch(*h, st));
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_connected_components(int32_t n, const int32_t *rowptr, const int32_t *colids, int32_t *labels, unsigned flags, g4s_cc_info *info,
                                            void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_DEVICE_POINTERS | G4S_CC_SYMMETRIC)) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and G4S_CC_SYMMETRIC");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr && labels, "rowptr or labels is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its result"));
    if (info) *info = g4s_cc_info{};
    if (n == 0) return G4S_OK;

    const int rounds = env_int("G4S_CC_SAMPLE_ROUNDS", kRoundsDefault, 0, kMaxRounds);
    const bool no_skip = env_int("G4S_CC_NO_SKIP", 0, 0, 1) != 0, symmetric = (flags & G4S_CC_SYMMETRIC) != 0, device = (flags & G4S_DEVICE_POINTERS) != 0;
    long long nnz = 0;
    if (!device) {
        nnz = rowptr[n];
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
    }
    CcState *st, h{};
    int *count, *hubs;                                             // the size count (n ints), the hub list
    Carver work;
    work.piece(&st, kStateBytes);
    work.piece(&count, sizeof(int) * (size_t)n);
    work.tail(&hubs, sizeof(int) * (size_t)std::min(n, kHubCap));
    Staged stage(s);
    int status = work.alloc();
    const int *rp = rowptr, *ci = colids;
    int *lab = labels;
    if (status == G4S_OK && !device) {
        rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1));
        ci = stage.in(colids, sizeof(int) * (size_t)nnz);
        lab = stage.out<int>(sizeof(int) * (size_t)n);
        status = stage.error();
    }
    if (status == G4S_OK) status = enqueue(n, rp, ci, lab, symmetric, rounds, no_skip, st, count, hubs, s);
    if (status == G4S_OK && !device) status = stage.to_host(labels, lab, sizeof(int) * (size_t)n);
    if (status == G4S_OK) status = fetch_state(&h, st, s);         // the call's one wait
    status = stage.finish(status);                                 // the caller's host arrays and the blocks: nothing in flight touches them
    work.idle();
    if (status == G4S_OK && h.invalid)
        status = g4s::set_error(G4S_ERR_INVALID, "g4s_connected_components: %s", csr_invalid_text(h.invalid));
    if (status == G4S_OK && info) {
        info->components = (int64_t)h.components;
        info->largest = (int64_t)(h.best >> 32);
        info->edges_linked = (int64_t)h.edges_linked;
        info->largest_label = INT_MAX - (int32_t)(h.best & 0xffffffffull);
        info->sample_rounds = rounds;
        info->skipped = h.skip;
        info->host_waits = 1;
    }
    return status;
}
