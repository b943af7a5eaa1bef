// frontier.hpp — what the frontier algorithms share (traverse.hip, betweenness.hip, components.hip): the walk over the entries of a
// level's rows, balanced over entries (walk_tiles for ordinary rows, walk_hubs for long ones), the one-atomicAdd-per-wave append, the scan for
// stored zeros and the row grid. What a row is, what travels with it (the payload) and what happens per entry stay with the caller, as callables.
#pragma once
#include "common.hpp"
#include "readback.hpp"

namespace {

constexpr int WG = 256;
// A row above kHubCut entries is a hub. Inside a tile a row is one lane's binary-search interval and a tile is one workgroup's loop, so one long row
// would hold a whole workgroup while the others idle; a hub is walked by ALL workgroups instead, kHubChunk entries per visit. 4096 = 16 rounds of a
// workgroup: above it the row is worth the hub loop's header loads in every workgroup, and 256 rows of at most 4096 entries keep a tile's scan total
// (2^20) far inside an int.
constexpr int kHubCut = 4096;
constexpr int kHubChunk = 1024;   // entries of a hub per workgroup visit

inline int grid_rows(long long n, int cus)
{
    const long long g = (n + WG - 1) / WG, cap = 8LL * cus;
    return (int)(g < 1 ? 1 : g < cap ? g : cap);
}

// Rows 0 … n − 1 of a level, 256 per tile, tiles dealt round-robin to the workgroups; call with every thread of a WG-thread workgroup.
//   row(i, start, len, payload)   for i < n: where row i's entries begin, how many there are (<= kHubCut) and what travels with them. start, len and
//                                 payload come in as 0; a row left at len = 0 is skipped — how a caller leaves out hubs and rows it does not want.
//   entry(valid, k, payload)      by EVERY thread in each round of 256 entries, valid = false past the end (k then means nothing): the callers'
//                                 wave-wide ballots need all lanes. k is the entry's index in the matrix arrays, payload its row's.
// The lengths are scanned across the four waves; a lane finds its entry's row by a binary search in the scan whose lower end never decreases as the
// lane's entry index grows. The scan total fits an int: 256 rows of at most kHubCut entries (and were a caller to let longer rows in: distinct
// vertices of one queue, at most nnz <= INT32_MAX entries together).
template <typename P, typename Row, typename Entry>
__device__ __forceinline__ void walk_tiles(int n, Row row, Entry entry)
{
    __shared__ int s_scan[WG + 1];
    __shared__ int s_start[WG];
    __shared__ P s_pay[WG];
    __shared__ int s_wsum[WG / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long s0 = (long long)blockIdx.x * WG; s0 < n; s0 += (long long)gridDim.x * WG) {
        int start = 0, len = 0;
        P pay = P();
        if (s0 + t < n) row((int)(s0 + t), start, len, pay);
        int x = len;                                               // inclusive scan of the 256 lengths
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wsum[wave] = x;
        s_start[t] = start;
        s_pay[t] = pay;
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += s_wsum[w];
        s_scan[t + 1] = off + x;
        if (t == 0) s_scan[0] = 0;
        __syncthreads();
        const int total = s_scan[WG];
        int lo = 0;                                                // the last row with s_scan[lo] <= e: never decreases as e grows
        for (int e0 = 0; e0 < total; e0 += WG) {
            const int e = e0 + t;
            const bool valid = e < total;
            int k = 0;
            if (valid) {
                int hi = WG - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_scan[mid] <= e) lo = mid;
                    else hi = mid - 1;
                }
                k = s_start[lo] + (e - s_scan[lo]);
            }
            entry(valid, k, s_pay[lo]);
        }
        __syncthreads();
    }
}

// Hubs 0 … nh − 1 of a level, every one by all workgroups: chunk c (kHubChunk entries) of hub h belongs to block (c + 4h) mod G, so the first
// chunks of consecutive hubs do not all land on block 0. hub(h, start, len, payload) names hub h's row as `row` does above and is asked once per
// chunk — a caller whose payload moves while the kernel runs (components.hip) gets it fresh for every chunk; `entry` is walk_tiles'.
template <typename P, typename Hub, typename Entry>
__device__ __forceinline__ void walk_hubs(int nh, Hub hub, Entry entry)
{
    const int G = (int)gridDim.x, t = (int)threadIdx.x;
    for (int h = 0; h < nh; ++h) {
        int first = (int)(((long long)blockIdx.x - 4ll * h) % G);
        if (first < 0) first += G;
        for (int c = first;; c += G) {
            int start = 0, len = 0;
            P pay = P();
            hub(h, start, len, pay);
            if ((long long)c * kHubChunk >= len) break;
            for (int j = 0; j < kHubChunk; j += WG) {
                const int e = c * kHubChunk + j + t;
                entry(e < len, start + e, pay);
            }
        }
    }
}

// The slot of each wanting lane behind *counter, by one atomicAdd per wave: ballot, the first wanting lane adds the popcount, every lane takes its
// rank among the wanting lanes below it. −1 for a lane that does not want. Call with every lane that is active at the call site. Where the
// vertex then goes (a queue's front, `order`, a hub list) is the caller's business, and so is the bound on the slot.
__device__ __forceinline__ int wave_append(bool want, int *counter)
{
    const unsigned long long m = __ballot(want);
    if (!want) return -1;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader);
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// *flag |= 1 when a stored value is 0.0: or-and takes a stored zero for no edge, so the kernels of such a matrix have to read the values
__global__ __launch_bounds__(WG) void any_zero_kernel(long long nnz, const double *__restrict__ values, int *flag)
{
    int z = 0;
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < nnz; k += (long long)gridDim.x * WG) z |= values[k] == 0.0;
    if (z) atomicOr(flag, 1);
}

// Does any stored value of a handle equal 0.0? The verdict is kept until g4s_csr_update_values brings new values.
struct ZeroScan {
    int state = 0;   // 0 unknown, 1 no stored value is zero, 2 some are
    void changed() { state = 0; }
    // The pass alone, on `s`: *flag_word = 0, then any_zero_kernel. For a caller that reads the word with something else it reads anyway.
    hipError_t enqueue(long long nnz, const double *values, int cus, int *flag_word, hipStream_t s) const
    {
        const hipError_t e = hipMemsetAsync(flag_word, 0, sizeof(int), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(any_zero_kernel, dim3(grid_rows(nnz, cus)), dim3(WG), 0, s, nnz, values, flag_word);
        return hipGetLastError();
    }
    // The pass and one read, unless the verdict is known. Synchronises `s`.
    int scan(long long nnz, const double *values, int cus, int *flag_word, hipStream_t s, int *waits)
    {
        if (state != 0) return G4S_OK;
        int h = 0;
        if (nnz > 0) {
            G4S_HIP_TRY(enqueue(nnz, values, cus, flag_word, s));
            G4S_HIP_TRY(g4s::ReadScope(s).fetch(h, flag_word));
            if (waits) *waits += 1;
        }
        state = h ? 2 : 1;
        return G4S_OK;
    }
};

} // namespace
