// coo.hip — a CSR from an edge list on the device (include/g4s.h: g4s_csr_from_coo_symbolic / _numeric). The reference does this on the host:
// CSR(graph&) sorts each source's edges and sums repeats (mm/inc/CSR.h:255-329), CSC::MergeDuplicates merges (mm/inc/CSC.h:297-342), CSR::construct sorts
// (mm/inc/CSR.h:640-668).
//
// The symbolic call:
//   coo_key_kernel      every id range-checked (fail bit BAD_ID) before anything is made of it; the key row·2^col_bits + col over the significant bits of
//                       (rows − 1, cols − 1); whether any triple is below its predecessor. One read-back: a bad id ends the call, an input in order skips the sort.
//   the sort            stable, least significant digit first, kDigitBits = 8 bits per pass, ceil((row_bits + col_bits) / 8) passes over (key, input index).
//                       A workgroup owns a tile of kTile consecutive elements, each of its four waves a quarter of it, walked 64 at a time:
//     coo_count_kernel    the tile's digit counts into the digit-major table counts[d · ntiles + tile];
//     prims::exclusive_scan over the table: the first output position of every (digit, tile);
//     coo_scatter_kernel  the tile walked in the order it was counted. A wave first counts its quarter (its row of the LDS table), the rows are turned into
//                       the first position of every (wave, digit), then the wave walks its quarter again: an element's rank among the equal digits of its 64 is
//                       popcount(match & lanes_below), where match — the lanes that hold the same digit — is eight ballots, one per digit bit, ANDed; the
//                       group's lowest lane moves the wave's LDS counter on. Earlier waves' counts live in LDS; no workgroup waits on another.
//   coo_heads_kernel    a head flag where the sorted key changes (none under G4S_DUP_KEEP) and the longest run: the last triple of a run gallops back to its first.
//   prims::exclusive_scan of the flags: the output slot of every run; its last element is the entry count.
//   coo_rowptr_kernel   crpt[r] = the slot of the first sorted position whose row is at least r: a binary search per row.
//   One read-back of the entry count and the longest run.
// The numeric call keeps nothing from the symbolic one and trusts nothing in perm or crpt: coo_perm_keys_kernel checks every perm element and every id it
// leads to and rebuilds the keys in perm's order, coo_heads_kernel checks that they never decrease (nor the input index inside a run), the scan gives the
// slots, and coo_fill_kernel starts by comparing its own entry count with crpt[rows] (BAD_CRPT). A head folds its run from left to right: L sequential
// operations of one lane (loads eight at a time). Every kernel behind a set fail flag returns at once; the slots written are below the count just compared
// with crpt[rows], whatever the arrays hold. Nothing goes through a floating-point atomic, nothing depends on timing.
#include "common.hpp"
#include "prims.hpp"
#include "readback.hpp"
#include "call_util.hpp"
#include <algorithm>
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int WG = 256, kWaves = WG / 64, kDigitBits = 8, kRadix = 1 << kDigitBits, kPer = 16, kTile = WG * kPer, kQuarter = kTile / kWaves;
constexpr long long kMaxGrid = 16384;                              // grid-stride kernels: at most 64 workgroups per CU of the 256
constexpr int BAD_ID = 1, BAD_PERM = 2, BAD_ORDER = 4, BAD_CRPT = 8;
static_assert(WG == kRadix, "one thread per digit value");

struct CooState {
    int fail, unsorted, longest, pad;
};

inline int bits_of(int32_t n) { return n > 1 ? 32 - __builtin_clz((unsigned)(n - 1)) : 0; }

__global__ __launch_bounds__(WG) void coo_key_kernel(long long n, int rows, int cols, int col_bits, const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                     u64 *__restrict__ keys, int32_t *__restrict__ perm, CooState *__restrict__ st)
{
    bool unsorted = false;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        const int r = row[i], c = col[i];
        const bool ok = (unsigned)r < (unsigned)rows && (unsigned)c < (unsigned)cols;
        keys[i] = ok ? ((u64)(unsigned)r << col_bits | (u64)(unsigned)c) : 0ull;
        perm[i] = (int)i;
        if (!ok) {
            atomicOr(&st->fail, BAD_ID);
        } else if (i > 0) {                                          // (a predecessor out of range sets the fail bit itself)
            const int r0 = row[i - 1], c0 = col[i - 1];
            unsorted |= r0 > r || (r0 == r && c0 > c);
        }
    }
    // half the triples of a shuffled list are below their predecessor: one atomic per wave at most, none once the flag is up (one per triple measured 95 ms for 1.7e7)
    if (__any(unsorted) && (threadIdx.x & 63) == 0 && !*(volatile int *)&st->unsorted) atomicOr(&st->unsorted, 1);
}

// the lanes of the wave that are live and hold digit d: one ballot per digit bit
__device__ __forceinline__ u64 match_digit(unsigned d, bool live)
{
    u64 m = __ballot(live);
#pragma unroll
    for (int b = 0; b < kDigitBits; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__device__ __forceinline__ unsigned digit_of(u64 key, int shift) { return (unsigned)(key >> shift) & (unsigned)(kRadix - 1); }

__global__ __launch_bounds__(WG) void coo_count_kernel(long long n, const u64 *__restrict__ keys, int shift, int ntiles, int *__restrict__ counts)
{
    __shared__ int h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const long long base = (long long)blockIdx.x * kTile + wave * kQuarter + lane;
#pragma unroll 4
    for (int u = 0; u < kPer; ++u) {
        const long long i = base + u * 64;
        const bool live = i < n;
        const unsigned d = live ? digit_of(keys[i], shift) : 0u;
        const u64 m = match_digit(d, live);
        if (live && (m & below) == 0ull) atomicAdd(&h[d], __popcll(m));   // integer, in LDS: the same count in any order
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// FIRST: the payload of the first pass is the element's own index.
template <bool FIRST>
__global__ __launch_bounds__(WG) void coo_scatter_kernel(long long n, const u64 *__restrict__ keys, const int32_t *__restrict__ idx, int shift, int ntiles,
                                                         const int *__restrict__ first, u64 *__restrict__ keys_out, int32_t *__restrict__ idx_out)
{
    __shared__ int wbase[kWaves][kRadix];                           // a wave reads and writes its own row only, between the two barriers one thread per digit all four
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wbase[w][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kTile + wave * kQuarter + lane;
#pragma unroll 4
    for (int u = 0; u < kPer; ++u) {
        const long long i = base + u * 64;
        const bool live = i < n;
        const unsigned d = live ? digit_of(keys[i], shift) : 0u;
        const u64 m = match_digit(d, live);
        if (live && (m & below) == 0ull) wbase[wave][d] += __popcll(m);   // one lane per digit value present
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        int run = first[(size_t)threadIdx.x * ntiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int t = wbase[w][threadIdx.x];
            wbase[w][threadIdx.x] = run;
            run += t;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int u = 0; u < kPer; ++u) {                                 // (the keys come from L2 this time: sixteen of them in registers cost the occupancy)
        const long long i = base + u * 64;
        const bool live = i < n;
        const u64 k = live ? keys[i] : 0ull;
        const unsigned d = digit_of(k, shift);
        const u64 m = match_digit(d, live);
        if (live) {
            const int pos = wbase[wave][d] + __popcll(m & below);   // < n: the table was counted from these very keys
            keys_out[pos] = k;
            idx_out[pos] = FIRST ? (int)i : idx[i];
        }
        __builtin_amdgcn_wave_barrier();                            // every lane has read the counter before the group's lowest lane moves it on
        if (live && (m & below) == 0ull) wbase[wave][d] += __popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
}

// p in [0, n]: head[p] = the key at p differs from the one before (head[n] = 0, the scan's total behind it); head may be NULL (G4S_DUP_KEEP).
// CHECK (numeric): keys[p − 1] <= keys[p], and perm ascending inside a run, else BAD_ORDER. !CHECK (symbolic): the longest run.
template <bool CHECK>
__global__ __launch_bounds__(WG) void coo_heads_kernel(long long n, const u64 *__restrict__ keys, const int32_t *__restrict__ perm, int *__restrict__ head,
                                                       CooState *__restrict__ st)
{
    if (CHECK && st->fail) return;
    long long longest = 0;
    bool bad = false;
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p <= n; p += (long long)gridDim.x * WG) {
        if (p == n) {
            if (head) head[n] = 0;
            continue;
        }
        const u64 k = keys[p];
        bool is_head = true;
        if (p > 0) {
            const u64 k0 = keys[p - 1];
            is_head = k0 != k;
            if (CHECK) bad |= k0 > k || (k0 == k && perm[p - 1] >= perm[p]);
        }
        if (head) head[p] = is_head;
        if (!CHECK && (p == n - 1 || keys[p + 1] != k)) {           // the last of its run: gallop back to the first, then bisect
            long long hi = p, lo = -1, step = 1;                    // keys[hi] == k, keys[lo] != k (or lo == −1)
            for (;;) {
                const long long q = hi - step;
                if (q < 0) break;
                if (keys[q] != k) { lo = q; break; }
                hi = q;
                step <<= 1;
            }
            while (hi - lo > 1) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (keys[mid] == k) hi = mid;
                else lo = mid;
            }
            longest = max(longest, p - hi + 1);
        }
    }
    if (!CHECK) {
        int v = (int)longest;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
        if ((threadIdx.x & 63) == 0 && v > *(volatile int *)&st->longest) atomicMax(&st->longest, v);
    }
    if (CHECK && bad) atomicOr(&st->fail, BAD_ORDER);
}

// excl == NULL (G4S_DUP_KEEP): every sorted position is its own slot
__global__ __launch_bounds__(WG) void coo_rowptr_kernel(int rows, long long n, int col_bits, const u64 *__restrict__ keys, const int *__restrict__ excl,
                                                        int32_t *__restrict__ crpt)
{
    for (long long r = (long long)blockIdx.x * WG + threadIdx.x; r <= rows; r += (long long)gridDim.x * WG) {
        const u64 target = (u64)r << col_bits;                      // rows <= 2^31 and col_bits <= 31: no overflow
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        crpt[r] = excl ? excl[lo] : (int)lo;
    }
}

__global__ __launch_bounds__(WG) void coo_perm_keys_kernel(long long n, int rows, int cols, int col_bits, const int32_t *__restrict__ row,
                                                           const int32_t *__restrict__ col, const int32_t *__restrict__ perm, u64 *__restrict__ keys,
                                                           CooState *__restrict__ st)
{
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < n; p += (long long)gridDim.x * WG) {
        const int q = perm[p];
        u64 key = 0ull;
        if ((u64)(unsigned)q >= (u64)n) {
            atomicOr(&st->fail, BAD_PERM);
        } else {
            const int r = row[q], c = col[q];
            if ((unsigned)r < (unsigned)rows && (unsigned)c < (unsigned)cols) key = (u64)(unsigned)r << col_bits | (u64)(unsigned)c;
            else atomicOr(&st->fail, BAD_ID);
        }
        keys[p] = key;
    }
}

// head / excl: n + 1 ints each (unused under G4S_DUP_KEEP). Runs behind a clean coo_perm_keys_kernel and coo_heads_kernel<true> only: every perm element is
// then an index into val, the keys are in order, and every slot is below excl[n], which is compared with crpt[rows] first.
template <bool VALUES>
__global__ __launch_bounds__(WG) void coo_fill_kernel(int dup, long long n, int col_bits, const u64 *__restrict__ keys, const int32_t *__restrict__ perm,
                                                      const double *__restrict__ val, const int *__restrict__ head, const int *__restrict__ excl,
                                                      const int32_t *__restrict__ crpt_last, int32_t *__restrict__ ccol, double *__restrict__ cval,
                                                      CooState *__restrict__ st)
{
    if (st->fail) return;
    const bool keep = dup == G4S_DUP_KEEP;
    const long long total = keep ? n : (long long)excl[n];
    if (total != (long long)*crpt_last) {
        if (threadIdx.x == 0) atomicOr(&st->fail, BAD_CRPT);
        return;
    }
    const u64 cmask = (1ull << col_bits) - 1ull;
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p < n; p += (long long)gridDim.x * WG) {
        if (keep) {
            ccol[p] = (int)(keys[p] & cmask);
            if (VALUES) cval[p] = val[perm[p]];
            continue;
        }
        const bool hd = head[p];
        const int slot = excl[p] - (hd ? 0 : 1);
        if (hd) ccol[slot] = (int)(keys[p] & cmask);
        if (!VALUES) continue;
        if (dup == G4S_COMBINE_SECOND) {                            // the latest triple: the last of the run writes
            if (head[p + 1] || p == n - 1) cval[slot] = val[perm[p]];
            continue;
        }
        if (!hd) continue;
        double acc = val[perm[p]];
        if (dup != G4S_COMBINE_FIRST) {
            // the run is [p, end): end + 1 is the first k in (p, n + 1] with more than slot + 1 heads before it (k = n + 1 counts as one)
            long long lo = p, hi, step = 1;
            for (;;) {
                hi = min(lo + step, n + 1);
                if (hi > n || excl[hi] > slot + 1) break;
                lo = hi;
                step <<= 1;
            }
            while (hi - lo > 1) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (excl[mid] > slot + 1) hi = mid;
                else lo = mid;
            }
            const long long end = hi - 1;
            long long k = p + 1;
            for (; k + 8 <= end; k += 8) {                          // eight loads in flight, the fold itself strictly left to right
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = val[perm[k + j]];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc = combine_values(dup, acc, v[j]);
            }
            for (; k < end; ++k) acc = combine_values(dup, acc, val[perm[k]]);
        }
        cval[slot] = acc;
    }
}

struct Shape {
    const char *fn;
    int dup, rows, cols;
    long long n;
    int row_bits, col_bits, passes;
    Shape(const char *f, int d, int r, int c, long long nn)
        : fn(f), dup(d), rows(r), cols(c), n(nn), row_bits(bits_of(r)), col_bits(bits_of(c)), passes((bits_of(r) + bits_of(c) + kDigitBits - 1) / kDigitBits) {}
};

int contract_error(const Shape &sh, int fail)
{
    if (fail & BAD_PERM) return g4s::set_error(G4S_ERR_INVALID, "%s: a perm element is outside [0, %lld)", sh.fn, sh.n);
    if (fail & BAD_ID) return g4s::set_error(G4S_ERR_INVALID, "%s: a row or column id is outside [0, %d) x [0, %d)", sh.fn, sh.rows, sh.cols);
    if (fail & BAD_ORDER) return g4s::set_error(G4S_ERR_INVALID, "%s: perm is not the stable (row, col) order of the triples: perm must come from the symbolic call", sh.fn);
    return g4s::set_error(G4S_ERR_INVALID, "%s: crpt[rows] is not the entry count of these triples: crpt must come from the symbolic call", sh.fn);
}

// Device arrays; the stream is synchronised on return. At most two waits. h_crpt / h_perm (host arrays, or NULL): the copies of crpt and perm a caller with
// host pointers wants, enqueued before the last wait so that they cost none of their own.
int symbolic_device(const Shape &sh, const int32_t *row, const int32_t *col, int32_t *crpt, int32_t *perm, int64_t *cnnz, g4s_coo_info *info, int32_t *h_crpt,
                    int32_t *h_perm, hipStream_t s)
{
    const long long n = sh.n;
    const bool keep = sh.dup == G4S_DUP_KEEP;
    const int ntiles = (int)((n + kTile - 1) / kTile);
    const size_t kb = 8 * ((size_t)n + 1), tb = 4 * ((size_t)kRadix * ntiles + 1);
    CooState *st;
    u64 *ka, *kbuf;                                                 // the keys and their partner of the sort
    int32_t *itmp;
    int *cnt, *first;
    Carver work;
    work.piece(&st, sizeof(CooState));
    work.piece(&ka, kb);
    work.piece(&kbuf, kb);
    work.piece(&itmp, 4 * (size_t)n);
    work.piece(&cnt, tb);
    work.piece(&first, tb);
    G4S_TRY(work.alloc());
    g4s::ReadScope reads(s);
    CooState h{};
    int waits = 0;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(CooState), s));
    if (n > 0) {
        hipLaunchKernelGGL(coo_key_kernel, dim3(grid_for<WG>(n, kMaxGrid)), dim3(WG), 0, s, n, sh.rows, sh.cols, sh.col_bits, row, col, ka, perm, st);
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(reads.fetch(h, st));
        ++waits;
        if (h.fail) {
            work.idle();
            return contract_error(sh, h.fail);
        }
    }
    const bool presorted = !h.unsorted;
    const u64 *sorted = ka;
    if (!presorted) {
        const u64 *src_k = ka;
        u64 *dst_k = kbuf;
        const int32_t *src_i = nullptr;
        for (int p = 0; p < sh.passes; ++p) {                       // the last pass writes perm, the ones before it alternate with the partner
            int32_t *dst_i = ((sh.passes - 1 - p) & 1) ? itmp : perm;
            hipLaunchKernelGGL(coo_count_kernel, dim3(ntiles), dim3(WG), 0, s, n, src_k, kDigitBits * p, ntiles, cnt);
            G4S_HIP_TRY(hipGetLastError());
            G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(cnt), first, (long long)kRadix * ntiles, s));
            if (p == 0) hipLaunchKernelGGL(coo_scatter_kernel<true>, dim3(ntiles), dim3(WG), 0, s, n, src_k, src_i, 0, ntiles, first, dst_k, dst_i);
            else hipLaunchKernelGGL(coo_scatter_kernel<false>, dim3(ntiles), dim3(WG), 0, s, n, src_k, src_i, kDigitBits * p, ntiles, first, dst_k, dst_i);
            G4S_HIP_TRY(hipGetLastError());
            u64 *freed = const_cast<u64 *>(src_k);
            src_k = dst_k;
            src_i = dst_i;
            dst_k = freed;
        }
        sorted = src_k;
    }
    // the key partner is free now: the head flags and their scan, n + 1 ints each
    int *head = reinterpret_cast<int *>(sorted == ka ? kbuf : ka), *excl = head + (n + 1);
    hipLaunchKernelGGL(coo_heads_kernel<false>, dim3(grid_for<WG>(n + 1, kMaxGrid)), dim3(WG), 0, s, n, sorted, (const int32_t *)nullptr, keep ? (int *)nullptr : head, st);
    G4S_HIP_TRY(hipGetLastError());
    if (!keep) G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(head), excl, n + 1, s));
    hipLaunchKernelGGL(coo_rowptr_kernel, dim3(grid_for<WG>((long long)sh.rows + 1, kMaxGrid)), dim3(WG), 0, s, sh.rows, n, sh.col_bits, sorted, keep ? (const int *)nullptr : excl, crpt);
    G4S_HIP_TRY(hipGetLastError());
    if (h_crpt) G4S_HIP_TRY(hipMemcpyAsync(h_crpt, crpt, 4 * ((size_t)sh.rows + 1), hipMemcpyDeviceToHost, s));
    if (h_perm && n > 0) G4S_HIP_TRY(hipMemcpyAsync(h_perm, perm, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    int total = (int)n;
    G4S_HIP_TRY(reads.note(h, st));
    if (!keep) G4S_HIP_TRY(reads.note(total, excl + n));
    G4S_HIP_TRY(reads.wait());
    ++waits;
    work.idle();                                                   // (an early return above leaves it out: the block is then released behind a device-wide wait)
    info->nnz_in = n;
    info->nnz_out = total;
    info->longest_run = h.longest;
    info->presorted = presorted;
    info->host_waits = waits;
    *cnnz = total;
    return G4S_OK;
}

// Device arrays (crpt_last: the one element crpt[rows]); the stream is synchronised on return. One wait. h_ccol / h_cval (host arrays of cn entries, or
// NULL): the copies a caller with host pointers wants, enqueued before the wait (after a refusal they hold what ccol / cval hold: nothing specified).
int numeric_device(const Shape &sh, const int32_t *row, const int32_t *col, const double *val, const int32_t *crpt_last, const int32_t *perm, int32_t *ccol,
                   double *cval, int32_t *h_ccol, double *h_cval, long long cn, hipStream_t s)
{
    const long long n = sh.n;
    const bool keep = sh.dup == G4S_DUP_KEEP;
    const size_t hb = 4 * ((size_t)n + 1);
    CooState *st;
    u64 *keys;
    int *head, *excl;
    Carver work;
    work.piece(&st, sizeof(CooState));
    work.piece(&keys, 8 * ((size_t)n + 1));
    work.piece(&head, hb);
    work.piece(&excl, hb);
    G4S_TRY(work.alloc());
    int fail = 0;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(CooState), s));
    hipLaunchKernelGGL(coo_perm_keys_kernel, dim3(grid_for<WG>(n, kMaxGrid)), dim3(WG), 0, s, n, sh.rows, sh.cols, sh.col_bits, row, col, perm, keys, st);
    hipLaunchKernelGGL(coo_heads_kernel<true>, dim3(grid_for<WG>(n + 1, kMaxGrid)), dim3(WG), 0, s, n, static_cast<const u64 *>(keys), perm, keep ? (int *)nullptr : head, st);
    G4S_HIP_TRY(hipGetLastError());
    if (!keep) G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(head), excl, n + 1, s));   // (behind a set fail flag head is unwritten: the scan reads the library's own block, the fill returns at once)
#define FILL_ARGS sh.dup, n, sh.col_bits, static_cast<const u64 *>(keys), perm, val, static_cast<const int *>(head), static_cast<const int *>(excl), crpt_last, ccol, cval, st
    if (cval) hipLaunchKernelGGL(coo_fill_kernel<true>, dim3(grid_for<WG>(n, kMaxGrid)), dim3(WG), 0, s, FILL_ARGS);
    else hipLaunchKernelGGL(coo_fill_kernel<false>, dim3(grid_for<WG>(n, kMaxGrid)), dim3(WG), 0, s, FILL_ARGS);
#undef FILL_ARGS
    G4S_HIP_TRY(hipGetLastError());
    if (h_ccol && cn > 0) G4S_HIP_TRY(hipMemcpyAsync(h_ccol, ccol, 4 * (size_t)cn, hipMemcpyDeviceToHost, s));
    if (h_cval && cn > 0) G4S_HIP_TRY(hipMemcpyAsync(h_cval, cval, 8 * (size_t)cn, hipMemcpyDeviceToHost, s));
    G4S_HIP_TRY(g4s::ReadScope(s).fetch(fail, &st->fail));
    work.idle();                                                   // (as in symbolic_device)
    if (fail) return contract_error(sh, fail);
    return G4S_OK;
}

bool valid_dup(int d) { return d == G4S_DUP_KEEP || (d >= G4S_COMBINE_PLUS && d <= G4S_COMBINE_SECOND); }

} // namespace

G4S_API g4s_status g4s_csr_from_coo_symbolic(int dup, int32_t rows, int32_t cols, int64_t nnz, const int32_t *row, const int32_t *col, int32_t *crpt, int32_t *perm,
                                             int64_t *cnnz, unsigned flags, g4s_coo_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_dup(dup), "dup is neither G4S_DUP_KEEP nor a G4S_COMBINE_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0 && nnz >= 0, "negative dimension or entry count");
    if (nnz > INT32_MAX) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: %lld triples exceed the int32 row pointers", __func__, (long long)nnz);
    G4S_REQUIRE(crpt && perm && cnnz, "crpt, perm or cnnz is NULL");
    G4S_REQUIRE((row && col) || nnz == 0, "row or col is NULL with nnz > 0");
    const size_t rp = 4 * ((size_t)rows + 1), nb = 4 * (size_t)nnz;
    const bool dev = flags & G4S_DEVICE_POINTERS;
    if (!dev) {
        const Span outs[] = {{crpt, rp}, {perm, nb}, {cnnz, sizeof(int64_t)}}, ins[] = {{row, nb}, {col, nb}};
        if (any_overlap(outs, ins)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input or another output", __func__);
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s));
    const Shape sh(__func__, dup, rows, cols, nnz);
    g4s_coo_info local{};
    if (!info) info = &local;
    *info = g4s_coo_info{};
    info->row_bits = sh.row_bits;
    info->col_bits = sh.col_bits;
    info->digit_bits = kDigitBits;
    info->sort_passes = sh.passes;
    info->tile_entries = kTile;
    *cnnz = 0;
    if (dev) return symbolic_device(sh, row, col, crpt, perm, cnnz, info, nullptr, nullptr, s);
    Staged stage(s);
    const int32_t *d_row = stage.in(row, nb), *d_col = stage.in(col, nb);
    int32_t *d_crpt = stage.out<int32_t>(rp), *d_perm = stage.out<int32_t>(nb);
    int status = stage.error();
    if (status == G4S_OK) status = symbolic_device(sh, d_row, d_col, d_crpt, d_perm, cnnz, info, crpt, perm, s);   // the copies to crpt / perm: its own
    return stage.finish(status);
}

G4S_API g4s_status g4s_csr_from_coo_numeric(int dup, int32_t rows, int32_t cols, int64_t nnz, const int32_t *row, const int32_t *col, const double *val,
                                            const int32_t *crpt, const int32_t *perm, int32_t *ccol, double *cval, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_dup(dup), "dup is neither G4S_DUP_KEEP nor a G4S_COMBINE_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0 && nnz >= 0, "negative dimension or entry count");
    if (nnz > INT32_MAX) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: %lld triples exceed the int32 row pointers", __func__, (long long)nnz);
    G4S_REQUIRE(crpt && perm, "crpt or perm is NULL");
    G4S_REQUIRE((row && col && ccol) || nnz == 0, "row, col or ccol is NULL with nnz > 0");
    G4S_REQUIRE((val == nullptr) == (cval == nullptr), "val and cval must both be given or both be NULL (pattern-only)");
    const size_t rp = 4 * ((size_t)rows + 1), nb = 4 * (size_t)nnz;
    const bool dev = flags & G4S_DEVICE_POINTERS;
    long long cn = 0;
    if (!dev) {
        cn = crpt[rows];
        if (cn < 0 || cn > nnz) return g4s::set_error(G4S_ERR_INVALID, "%s: crpt[rows] = %lld is not an entry count of %lld triples", __func__, cn, (long long)nnz);
        const Span outs[] = {{ccol, 4 * (size_t)cn}, {cval, 8 * (size_t)cn}}, ins[] = {{row, nb}, {col, nb}, {val, 2 * nb}, {crpt, rp}, {perm, nb}};
        if (any_overlap(outs, ins)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input or another output", __func__);
    }
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s));
    const Shape sh(__func__, dup, rows, cols, nnz);
    if (dev) return numeric_device(sh, row, col, val, crpt + rows, perm, ccol, cval, nullptr, nullptr, 0, s);
    Staged stage(s);
    const int32_t *d_row = stage.in(row, nb), *d_col = stage.in(col, nb);
    const double *d_val = stage.in(val, 2 * nb);
    const int32_t *d_last = stage.in(crpt + rows, 4), *d_perm = stage.in(perm, nb);
    int32_t *d_ccol = stage.out<int32_t>(4 * (size_t)cn);
    double *d_cval = cval ? stage.out<double>(8 * (size_t)cn) : nullptr;
    int status = stage.error();
    if (status == G4S_OK) status = numeric_device(sh, d_row, d_col, d_val, d_last, d_perm, d_ccol, d_cval, ccol, cval, cn, s);   // the copies to ccol / cval: its own
    return stage.finish(status);
}
