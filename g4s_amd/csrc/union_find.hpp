// union_find.hpp — the concurrent union-find forest in HBM that components.hip and msf.hip share: the wait-free hook (link_from) and one pass of pointer
// jumping (jump_pass). parent[x] <= x always holds and parents only ever decrease, so the root of a tree is its smallest id: the canonical label.
// Memory model: a plain load of parent[] inside a kernel may be stale; a stale value is a FORMER ancestor, still in the same tree and never
// too small, and hooks are decided by the compare-and-swap alone. Kernel boundaries are the only ordering between a linking and a jumping kernel.
#pragma once
#include "frontier.hpp"

namespace {

constexpr int kJumpHops = 16;        // a pass moves a vertex this many hops up
constexpr int kJumpPasses = 8;       // 16^8 = 2^32 > any depth

__device__ __forceinline__ void st_(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// Union of the trees of a and b (ancestors, possibly former ones, of the edge's two ends). max(a, b) strictly decreases: bounded, wait-free.
__device__ __forceinline__ void link_from(int a, int b, int *parent)
{
    while (a != b) {
        const int high = a > b ? a : b, low = a < b ? a : b;
        int p = ld(parent + high);
        if (p == low) return;
        if (p == high) {
            p = (int)atomicCAS(parent + high, high, low);
            if (p == high) return;                                 // hooked: high was a root
        }
        a = ld(parent + p);                                        // p < high: what the load or the failed CAS returned
        b = ld(parent + low);
    }
}

// One pass of pointer jumping over all vertices, by every thread of the grid: each vertex moves kJumpHops hops up, or to its root. Non-zero when a
// vertex of this thread is still short of its root. No link runs beside it.
__device__ __forceinline__ int jump_pass(int n, int *parent)
{
    int more = 0;
    for (long long v = (long long)blockIdx.x * WG + threadIdx.x; v < n; v += (long long)gridDim.x * WG) {
        const int p0 = ld(parent + v);
        int p = p0, g = ld(parent + p);
        for (int h = 1; h < kJumpHops && g != p; ++h) { p = g; g = ld(parent + p); }
        if (p != p0) st_(parent + v, p);
        more |= g != p;
    }
    return more;
}

} // namespace
