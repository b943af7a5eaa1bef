// frontier.hpp — what the frontier algorithms share (traverse.hip, betweenness.hip, components.hip, kcore.hip, color.hip, ktruss.hip, scc.hip, msf.hip, trsv.hip, ilu.hip; DESIGN
// §4.11): the walk over the entries of a level's rows, balanced over entries (walk_tiles for ordinary rows, walk_hubs for long ones), the opening pass
// of the calls on raw CSR arrays (open_rows: the row check; open_ids / open_hubs: the check of the column ids), the one-atomicAdd-per-wave append and
// the append to a frontier that keeps a hub list (append_frontier), the two ends of a step kernel (step_runs; turn_page: the last workgroup to take a
// ticket turns the page of the state block; flip_queue: what every page turn does to the queue words), the scan for stored zeros and the row grid;
// what a row is, its payload, what happens per entry and what else a page turn writes stay with the caller, as callables. It brings along WG and the
// wave reductions (wave_reduce.hpp, which pagerank.hip takes alone) and the host side of the stepped loop (step_batch.hpp). level_peel.hpp puts the
// page turn and the host loop of kcore.hip and ktruss.hip on top of it.
#pragma once
#include "readback.hpp"
#include "step_batch.hpp"
#include "wave_reduce.hpp"
#include <type_traits>

namespace {

// A row above kHubCut entries is a hub. Inside a tile a row is one lane's binary-search interval and a tile is one workgroup's loop, so one long row
// would hold a whole workgroup while the others idle; a hub is walked by ALL workgroups instead, kHubChunk entries per visit. 4096 = 16 rounds of a
// workgroup: above it the row is worth the hub loop's header loads in every workgroup, and 256 rows of at most 4096 entries keep a tile's scan total
// (2^20) far inside an int.
constexpr int kHubCut = 4096;
constexpr int kHubChunk = 1024;   // entries of a hub per workgroup visit
constexpr int kHubCap = 1 << 19;  // room in a hub list: rows above kHubCut entries are fewer than 2^31 / 4096

// a load that may be stale, which the compiler may neither tear nor assume race-free: a plain global load
__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

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

// The opening pass of a call on raw CSR arrays, in kernels of the caller's (their names, their guards and whatever else they do stay with it). First
// the rows: *invalid |= bit unless rowptr[0] == 0 and rowptr never decreases over rows 0 … n − 1; fill(i, rb, re) per row is the caller's.
template <typename Fill>
__device__ __forceinline__ void open_rows(int n, const int *__restrict__ rowptr, int *invalid, int bit, Fill fill)
{
    int bad = 0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        const int rb = rowptr[i], re = rowptr[i + 1];
        bad |= rb < 0 || re < rb || (i == 0 && rb != 0);
        fill(i, rb, re);
    }
    if (bad) atomicOr(invalid, bit);
}

// Then the column ids, behind a kernel boundary and the caller's `if (*invalid) return` ([0, rowptr[n]) is the colids array beyond it):
// *invalid |= bit for an id outside [0, n) and, with kAscending, |= 2 · bit for one that is not above the id before it in its row;
// accept(k, u, v) for every other entry k of row u, v its id. open_ids walks the ordinary rows and collects the rows above kHubCut entries in hubs[]
// behind the counter *n_hubs; open_hubs, a kernel later, walks those (the count clamped to hub_cap: fewer than 2^31 / kHubCut such rows exist).
struct OpenRow {
    int u, start;                                                  // the order check wants to know where the row begins
};
template <bool kAscending> using OpenPay = std::conditional_t<kAscending, OpenRow, int>;

template <bool kAscending, typename Accept>
__device__ __forceinline__ void open_entry(bool valid, int k, OpenPay<kAscending> p, int n, const int *__restrict__ colids, int bit, int &bad, Accept accept)
{
    if (!valid) return;
    const int v = colids[k];
    if ((unsigned)v >= (unsigned)n) {
        bad |= bit;
    } else if constexpr (kAscending) {
        if (k > p.start && colids[k - 1] >= v) bad |= 2 * bit;
        else accept(k, p.u, v);
    } else {
        accept(k, p, v);
    }
}

template <bool kAscending, typename Accept>
__device__ __forceinline__ void open_ids(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, int *__restrict__ hubs, int *n_hubs,
                                         int *invalid, int bit, Accept accept)
{
    int bad = 0;
    walk_tiles<OpenPay<kAscending>>(n, [&](int i, int &start, int &len, OpenPay<kAscending> &p) {
        const int rb = rowptr[i], l = rowptr[i + 1] - rb;
        if constexpr (kAscending) p = OpenRow{i, rb};
        else p = i;
        if (l > kHubCut) {
            const int h = atomicAdd(n_hubs, 1);
            if ((unsigned)h < (unsigned)hub_cap) hubs[h] = i;
            return;
        }
        start = rb;
        len = l;
    }, [&](bool valid, int k, OpenPay<kAscending> p) { open_entry<kAscending>(valid, k, p, n, colids, bit, bad, accept); });
    if (bad) atomicOr(invalid, bad);
}

template <bool kAscending, typename Accept>
__device__ __forceinline__ void open_hubs(int n, int hub_cap, const int *__restrict__ rowptr, const int *__restrict__ colids, const int *__restrict__ hubs,
                                          const int *n_hubs, int *invalid, int bit, Accept accept)
{
    int bad = 0;
    walk_hubs<OpenPay<kAscending>>(*n_hubs < hub_cap ? *n_hubs : hub_cap, [&](int h, int &start, int &len, OpenPay<kAscending> &p) {
        const int u = hubs[h];
        start = rowptr[u];
        len = rowptr[u + 1] - start;
        if constexpr (kAscending) p = OpenRow{u, start};
        else p = u;
    }, [&](bool valid, int k, OpenPay<kAscending> p) { open_entry<kAscending>(valid, k, p, n, colids, bit, bad, accept); });
    if (bad) atomicOr(invalid, bad);
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

// An item v (a vertex, an edge) whose row has `len` entries, for the frontier being built: behind *tail in the queue (an item is appended once per call,
// so its slot is below `bound` by construction), into the next hub list behind *n_hub_next when the row is long, and len onto the lane's share of
// the frontier's entries. Called by every lane that is active at the call site. False when the hub list had no room for v.
__device__ __forceinline__ bool append_frontier(bool want, int v, int len, int bound, int hub_cap, int *__restrict__ queue, int *__restrict__ hubs_next, int *tail,
                                                int *n_hub_next, long long &len_sum)
{
    const int idx = wave_append(want, tail);
    if ((unsigned)idx < (unsigned)bound) queue[idx] = v;
    bool room = true;
    if (want && len > kHubCut) {
        const int h = atomicAdd(n_hub_next, 1);
        room = (unsigned)h < (unsigned)hub_cap;
        if (room) hubs_next[h] = v;
    }
    if (want) len_sum += len;
    return room;
}

// May a resumable step kernel run? `stop` is the state's word, the same for every block (it changes only after the last ticket): 0 goes on, 4 (the
// frontier outgrew the launch grid) goes on in the first launch of the next batch, which the host marks `resume`; every other value ends the steps.
__device__ __forceinline__ bool step_runs(int stop, int resume) { return stop == 0 || (stop == 4 && resume); }

// The end of a step kernel, called by every thread of every workgroup once its waves' shares are in the caller's LDS slots: thread 0 publishes the
// workgroup's share (`publish()`: atomics on the caller's state) and takes a ticket; true for thread 0 of the workgroup that took the last one, which
// then turns the page: it reads the totals back with atomicAdd(…, 0), writes the next step's state with plain stores and sets *tickets = 0 for the
// next kernel. Nobody waits for anybody. This is the only ordering between workgroups inside a kernel:
//   the first fence, by every thread in front of the barrier, makes the workgroup's own stores and appends visible device-wide before thread 0 can
//     take the ticket (the XCDs' L2s are not coherent with each other for plain stores); the barrier also hands the LDS slots to thread 0;
//   the second fence orders thread 0's publishing atomics before its ticket, so whoever sees the ticket sees them;
//   the ticket is a device-scope atomic on one word: exactly one workgroup reads gridDim.x − 1, and every other ticket came before it;
//   the closing fence keeps the winner's reads behind its ticket, and those reads are atomics, performed in memory and not in a cache that may hold
//     an older copy (a plain load of what another workgroup wrote in this kernel may be stale). The next kernel reads what it writes.
template <typename Publish>
__device__ __forceinline__ bool turn_page(int *tickets, Publish publish)
{
    __shared__ int s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        publish();
        __threadfence();
        s_last = atomicAdd(tickets, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return false;
    __threadfence();
    return true;
}

// What the winner of turn_page does to the queue words that PeelState (step_batch.hpp), ClState (color.hpp) and TrState (trsv.hpp) name alike: the
// frontier that was being built becomes the current one — queue[end, tail), its hub list, its entry sum —, an empty one is begun, and the tickets are
// 0 for the next kernel. The totals are read back with atomics (turn_page says why). The caller's own words and its `stop` rule follow it.
struct QueueFlip {
    int appended, walked;                                          // items this kernel appended; items of the frontier it walked
    long long entries;                                             // the entry sum of what it appended
};
template <typename State>
__device__ __forceinline__ QueueFlip flip_queue(State *st)
{
    const int tail = atomicAdd(&st->tail, 0), nh = atomicAdd(&st->n_hub_next, 0);
    const long long e = (long long)atomicAdd((unsigned long long *)&st->edges_next, 0ull);
    const QueueFlip f{tail - st->end, st->end - st->head, e};
    st->head = st->end; st->end = tail;
    st->n_hub_cur = nh; st->n_hub_next = 0; st->hub_cur ^= 1;
    st->edges_cur = e; st->edges_next = 0;
    st->tickets = 0;
    return f;
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
