// unit_walk.hpp — the work unit of the row-wise CSR builders (ewise.hip: merge and select; extract.hip: expand by multiplicity), once. A row's sequence of
// positions is cut into units of kUnit = 64; a row of len positions has ceil(len / kUnit) units and an empty row none. uoff — the exclusive scan of the rows'
// unit counts — names the first unit of every row and, in its last element, the number of units. A fixed grid of kGridWG workgroups walks them: wave w owns
// the units [w·chunk, (w + 1)·chunk), its kGroups = 4 groups of kLanes = 16 adjacent lanes take them four at a time, kPer = 4 positions a lane.
// What a unit's positions are and what is done with them is the kernel's own; so are its fail gates, which stay in front of the walk.
#pragma once
#include "common.hpp"
#include <climits>

namespace {   // (one copy per translation unit, as the kernels of prims.hpp)

constexpr int WG = 256, kLanes = 16, kPer = 4, kUnit = kLanes * kPer, kGroups = 64 / kLanes;
constexpr int kGridWG = 2048;                                      // 8 workgroups per CU of the 256: 8192 waves, each with a contiguous run of units
constexpr long long kWaves = (long long)kGridWG * (WG / 64);

enum Mode { COUNT_ROWS = 0, COUNT_UNITS = 1, FILL = 2 };

// Σ ceil(len / kUnit) <= entries / kUnit + rows: every row's last unit may be a partial one. unit_cap: room for that many units and the scan's total;
// too_many_units: more than the int32 unit table holds.
__host__ __device__ inline long long unit_cap(long long rows, unsigned long long entries) { return rows + (long long)(entries / kUnit) + 1; }
__host__ __device__ inline bool too_many_units(long long rows, unsigned long long entries) { return entries / kUnit + (unsigned long long)rows > (unsigned long long)(INT_MAX - 1); }

// the last row r in [lo, rows) with uoff[r] <= u, given uoff[lo] <= u < uoff[rows]: gallop, then bisect (the next unit is mostly in the same or the next row)
__device__ __forceinline__ int row_of_unit(const int *__restrict__ uoff, int rows, int lo, int u)
{
    int step = 1;
    while (lo + step < rows && uoff[lo + step] <= u) {
        lo += step;
        step <<= 1;
    }
    int hi = min(lo + step, rows) - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (uoff[mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the row of unit u, searched from the row of the group's previous unit (prev < 0: it had none). The units of a group ascend.
__device__ __forceinline__ int row_after(const int *__restrict__ uoff, int rows, int prev, int u)
{
    if (prev < 0) return row_of_unit(uoff, rows, 0, u);
    return uoff[prev + 1] <= u ? row_of_unit(uoff, rows, prev + 1, u) : prev;
}

// over the kLanes lanes of a unit; every lane of the wave must arrive
template <typename V>
__device__ __forceinline__ V group_sum(V v)
{
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kLanes);
    return v;
}

template <typename V>
__device__ __forceinline__ V group_inclusive(V v, int lane)
{
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
        const V below = __shfl_up(v, off, kLanes);
        if (lane >= off) v += below;
    }
    return v;
}

// *ptr += Σ v over the workgroup with one 64-bit atomic: thousands of waves adding to one address were most of ex_check_kernel's time (profiles/extract.txt).
// Every thread of the workgroup must arrive.
__device__ __forceinline__ void workgroup_add_u64(unsigned long long *ptr, unsigned long long v)
{
    __shared__ unsigned long long wsum[WG / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < WG / 64; ++w) t += wsum[w];
        if (t) atomicAdd(ptr, t);
    }
}

// The walk of one lane group through its wave's run of units, one round at a time:
//     UnitWalk w(units);
//     int r = -1;
//     for (long long it = 0; it < w.chunk; it += kGroups) {
//         const long long ul = w.unit(it);
//         const bool live = w.live(ul);
//         if (live) r = row_after(uoff, rows, r, (int)ul); ...
// The loop counts rounds, not units: a group whose units have run out stays in it with live == false, so that every lane of the wave makes the same number
// of rounds and a shuffle or ballot in the body is never divergent. (The loop and the row stay in the kernel: with both inside the struct the compiler
// ordered the loads of ew_merge_kernel<FILL> differently and the numeric call measured 1 % slower; in this form the kernels of ewise.hip compile to the
// instructions they had before.)
struct UnitWalk {
    long long chunk, c0, c1;                                       // units per wave; this wave's are [c0, c1)
    int lane, group;
    __device__ __forceinline__ explicit UnitWalk(int units)
        : chunk(((long long)units + kWaves - 1) / kWaves), c0(((long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * chunk),
          c1(min(c0 + chunk, (long long)units)), lane(threadIdx.x & (kLanes - 1)), group((threadIdx.x & 63) / kLanes)
    {
    }
    __device__ __forceinline__ long long unit(long long it) const { return c0 + it + group; }
    __device__ __forceinline__ bool live(long long ul) const { return ul < c1; }
};

} // namespace
