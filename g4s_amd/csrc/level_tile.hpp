// level_tile.hpp — the device side of a level-scheduled call (trsv.hip: tr_level_kernel<Rhs>, tr_chain_kernel<Rhs>; ilu.hip: ilu_level_kernel,
// ilu_chain_kernel): which workgroup takes which rows of a level, which thread, wave or workgroup works a row off (deal_tile), the walk
// of one workgroup through the levels of a chain and the loads that make it correct. What a row is and the arithmetic on it stay with the two files,
// as callables; level_schedule.hpp is the host side.
#pragma once
#include "common.hpp"
#include "wave_reduce.hpp"
#include "level_schedule.hpp"
#include <algorithm>

namespace {

static_assert(g4s::kLevelWg == WG, "the host sizes the grids for the workgroup the kernels run with");
static_assert(G4S_TRSV_CHAIN_WIDTH == WG, "a level of a chain is one tile of the workgroup");
static_assert(WG / 64 == 4, "four waves: the hub shapes of both calls count on it");

// The stored form of a finished value: IEEE leaves a NaN's sign and payload open (b − s is b + (−s) on this hardware), the header fixes them.
__device__ __forceinline__ double canonical_nan(double v) { return v != v ? __longlong_as_double(0x7FF8000000000000ll) : v; }

// A value that a row of an earlier level stored. Behind a kernel boundary (a level kernel) a plain load does. In a chain the value may be this
// workgroup's of a moment ago, and the CU's vector cache may still hold the line from before: the load is performed in L2 (for_chain_levels).
template <bool kChain>
__device__ __forceinline__ double ld_prior(const double *p)
{
    if constexpr (kChain) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// The rows [x, y) of workgroup blockIdx.x in a level launch over the rows [lo, hi) of the layout: WG / stride a workgroup, the last tile cut by hi.
__device__ __forceinline__ int2 level_tile_bounds(int lo, int hi, int stride)
{
    const long long t0 = (long long)lo + (long long)blockIdx.x * (WG / stride);
    return make_int2((int)t0, (int)std::min<long long>(hi, t0 + WG / stride));
}

// A chain: one workgroup through the levels [level_lo, level_hi) of at most WG rows each, body(lo, hi, stride) per level with every thread — a tile
// whose rows are spread over the four waves by the largest stride that leaves room.
// Memory model: a row of a later level reads what a row of an earlier level of the same kernel stored. Every level therefore ends with
// __threadfence() — its stores are in L2 before anybody passes the barrier — and __syncthreads(), and every such read is ld_prior<true>: an
// agent-scope load, past whatever copy of the line the CU's vector cache holds. No wave waits for another workgroup; nothing spins.
template <typename Body>
__device__ __forceinline__ void for_chain_levels(const int *loff, int level_lo, int level_hi, Body body)
{
    for (int l = level_lo; l < level_hi; ++l) {
        const int lo = loff[l], hi = loff[l + 1];
        int stride = 64;
        while (stride > 1 && WG / stride < hi - lo) stride >>= 1;
        body(lo, hi, stride);
        __threadfence();
        __syncthreads();
    }
}

// Rows [lo, hi) of the layout, hi − lo <= WG / stride, all of one level — no row reads another —; called by every thread of the workgroup. Thread t
// owns row lo + t / stride when stride (a power of two up to 64) divides t; the owner gets its row's index back, every other thread −1. row_of(p)
// names row p: a struct of ints whose member m is the row's own length, the one thing that decides its class — who works a row off never changes a bit:
//   m <= kLaneCut             lane_row(row) by the owner alone
//   kLaneCut < m <= kWaveCut  wave_row(row, j) by every lane of the owner's wave with the lane's OWN row, j the owner's lane (the callee takes what it
//                             wants of row j with __shfl): a wave takes such rows one after another, so where rows are long the launch gives it few
//   m > kWaveCut              hub_row(row, th) by every thread of the workgroup, th the owner: through the list s_hub[WG] behind the counter *s_nh
//                             (LDS of the kernel's), in the order of the list — any order
// The lane and the wave rows come before the barrier behind the hub append, the hubs after it, a barrier behind each.
template <int kLaneCut, int kWaveCut, typename RowOf, typename LaneRow, typename WaveRow, typename HubRow>
__device__ __forceinline__ int deal_tile(int lo, int hi, int stride, int *s_hub, int *s_nh, RowOf row_of, LaneRow lane_row, WaveRow wave_row, HubRow hub_row)
{
    static_assert(kLaneCut >= 1 && kLaneCut < kWaveCut, "the three row classes");
    using Row = decltype(row_of(0));
    const int t = (int)threadIdx.x;
    const int p = lo + t / stride;
    const bool have = t % stride == 0 && p < hi;
    const Row r = have ? row_of(p) : Row{};                        // m == 0: no class but the lane's, which `have` guards
    if (t == 0) *s_nh = 0;
    __syncthreads();
    if (r.m > kWaveCut) s_hub[atomicAdd(s_nh, 1)] = t;
    if (have && r.m <= kLaneCut) lane_row(r);
    unsigned long long wm = __ballot(r.m > kLaneCut && r.m <= kWaveCut);
    while (wm) {                                                   // the same for every lane of the wave
        const int j = __ffsll((long long)wm) - 1;
        wm &= wm - 1;
        wave_row(r, j);
    }
    __syncthreads();
    const int nh = *s_nh;
    for (int h = 0; h < nh; ++h) {
        const int th = s_hub[h];
        hub_row(row_of(lo + th / stride), th);
        __syncthreads();
    }
    return have ? p : -1;
}

} // namespace
