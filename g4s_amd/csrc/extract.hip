// extract.hip — C = A[I, J] on the device: C(p, q) is stored exactly where A(I[p], J[q]) is (include/g4s.h: g4s_csr_extract_symbolic / _numeric).
// The reference has CSR(const CSR&, M_, N_, M_start, N_start) for a contiguous block (mm/inc/CSR.h:691-733) and CSC::SpRef / SpRef2 for sorted lists
// (mm/inc/CSC.h:513-690), both host loops. I and J may be in any order and may repeat ids — MATLAB's A(I, J).
//
// The work unit is unit_walk.hpp's, cut as sel_kernel (ewise.hip) cuts it: kUnit = 64 stored entries of the source row I[p], taken by kLanes = 16 adjacent lanes, four entries each in
// stored order; short rows share a wave and a hub row spreads over the grid.
//   ex_check_kernel     one pass: the row pointers (zero-based, non-decreasing: BAD_ROWPTR) as in ew_rows_kernel, every id of I and J range-checked (BAD_ID)
//                       before anything is made of it, whether J ever decreases, the units of every output row, the entries of A in the selected rows, and
//                       mult[c] = #{q : J[q] == c} with one integer atomic per id of J.
//   prims::exclusive_scan of the unit counts → the first unit of every output row; of mult → jptr. For a J that never decreases the q's of column c are the
//                       range [jptr[c], jptr[c + 1]) and nothing else is stored; otherwise ex_jlist_kernel fills jlist through per-column cursors (the order
//                       inside a list is free: the sort below fixes it). J == NULL: q = c, no map.
//   ex_walk_kernel      a fixed grid; wave w owns the units [w·chunk, (w + 1)·chunk), its four lane groups take them four at a time.
//     COUNT_ROWS        (symbolic) Σ mult[col[e]] over the unit, added to its output row with one integer atomic into a scratch array whose scan is crpt;
//                       every column id of A is range-checked before it indexes mult (BAD_COL). The symbolic call ends here: one wait.
//     COUNT_UNITS       (numeric) the unit's count stored; a scan gives every unit its first output slot. ex_crpt_kernel then compares EVERY crpt[p] with
//                       the slot of row p's first unit (BAD_CRPT): the numeric call refuses a crpt that is not what it arrives at itself.
//     FILL              the same walk: a 16-lane scan of the multiplicities, then each lane writes the expanded run (q, src = e) of its entry.
//   ex_order_kernel     a descent ccol[x − 1] > ccol[x] inside a row (the row found by bisection in crpt, only where there is a descent) flags the row.
//   ex_classify_kernel  rows without a flag are in order and are left alone; the others go into three lists by their length L (a workgroup walks its run of
//                       rows twice: count, one atomic per list for its range, place).
//   the sort            keys are 64-bit (q << 32) | position in the unsorted output row — distinct, so any correct sort is stable; the payload is src.
//     ex_sort_wave_kernel  L <= 64: one wave per row, four rows per workgroup, a bitonic network over the lanes (shuffles only).
//     ex_sort_lds_kernel   L <= kLdsMax: one workgroup per row, a bitonic network over 64-bit keys in LDS (48 KiB: three workgroups per CU).
//     longer rows          compacted as triples (rank among the long rows, q) and sorted by g4s_csr_from_coo_symbolic(G4S_DUP_KEEP) — the stable radix
//                          sort of coo.hip — whose perm is the answer (ex_long_gather_kernel / ex_long_apply_kernel).
//   ex_values_kernel    cval[x] = val[src[x]], bit for bit.
// No workgroup waits on another, no value goes through an atomic, no atomic touches a result; the integer atomics count into scratch and order work lists,
// which decide who sorts a row, never what comes out.
//
// Memory safety: ids of I, J and the row pointers are checked by ex_check_kernel and every kernel behind it returns at once when a fail bit is set; a
// column id of A is checked where it is read; every write of FILL is below both its unit's end and the entry count the host compared with crpt[ni].
#include "common.hpp"
#include "prims.hpp"
#include "readback.hpp"
#include "call_util.hpp"
#include "unit_walk.hpp"
#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kCheckWG = 1024;                                    // ex_check_kernel: one 64-bit atomic per workgroup on one address
constexpr int kClassifyWG = 512;                                 // ex_classify_kernel: one atomic per workgroup and list
constexpr int kWaveMax = 64, kLdsMax = 4096;                       // 4096 keys of 8 bytes + 4096 payloads of 4: 48 KiB of the CU's 160, three workgroups per CU
constexpr int BAD_ROWPTR = 1, BAD_ID = 2, BAD_COL = 4, BAD_CRPT = 8;

struct ExState {
    int fail, j_unsorted, nnz_a, rows_in_order;
    u64 nnz_rows, cnnz, long_entries;
    int n_wave, n_lds, n_long, pad;
};

__device__ __forceinline__ bool dead(const ExState *st, int ni) { return st->fail || too_many_units(ni, st->nnz_rows); }

// mult (may be NULL: J == NULL): cols + 1 ints, zeroed. upr: ni + 1 ints.
__global__ __launch_bounds__(WG) void ex_check_kernel(int rows, int cols, const int32_t *__restrict__ rpt, int ni, const int32_t *__restrict__ I, int nj,
                                                      const int32_t *__restrict__ J, int *__restrict__ upr, int *__restrict__ mult, ExState *__restrict__ st)
{
    const long long n = (long long)max(rows, max(ni, nj)) + 1;
    u64 len_sum = 0;
    bool unsorted = false;
    int bad = 0;
    for (long long t = (long long)blockIdx.x * WG + threadIdx.x; t < n; t += (long long)gridDim.x * WG) {
        if (t <= rows) {
            const int a0 = rpt[t];
            if ((t == 0 && a0 != 0) || a0 < 0) bad |= BAD_ROWPTR;
            if (t < rows) {
                if (rpt[t + 1] < a0) bad |= BAD_ROWPTR;
            } else {
                st->nnz_a = a0;
            }
        }
        if (t <= ni) {
            int units = 0;
            if (t < ni) {
                const int r = I ? I[t] : (int)t;
                if ((unsigned)r >= (unsigned)rows) {
                    bad |= BAD_ID;
                } else {
                    const long long len = (long long)rpt[r + 1] - rpt[r];   // (garbage under BAD_ROWPTR: nothing behind this kernel runs then)
                    if (len > 0) {
                        units = (int)((len + kUnit - 1) / kUnit);
                        len_sum += (u64)len;
                    }
                }
            }
            upr[t] = units;
        }
        if (J && t < nj) {
            const int c = J[t];
            if ((unsigned)c >= (unsigned)cols) {
                bad |= BAD_ID;
            } else {
                atomicAdd(&mult[c], 1);                             // integer: the same count in any order
                if (t > 0 && J[t - 1] > c) unsorted = true;          // (a predecessor out of range sets the fail bit itself)
            }
        }
    }
    workgroup_add_u64(&st->nnz_rows, len_sum);
    if (__any(unsorted) && (threadIdx.x & 63) == 0 && !*(volatile int *)&st->j_unsorted) atomicOr(&st->j_unsorted, 1);
    if (bad) atomicOr(&st->fail, bad);
}

// jlist[jptr[c] + k] = the k-th q (in arrival order) with J[q] == c. cursor: cols ints, zeroed. Runs only for a J that decreases somewhere.
__global__ __launch_bounds__(WG) void ex_jlist_kernel(int ni, int nj, const int32_t *__restrict__ J, const int *__restrict__ jptr, int *__restrict__ cursor,
                                                      int *__restrict__ jlist, const ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < nj; q += (long long)gridDim.x * WG) {
        const int c = J[q];                                          // checked by ex_check_kernel
        const int pos = jptr[c] + atomicAdd(&cursor[c], 1);
        if ((unsigned)pos < (unsigned)nj) jlist[pos] = (int)q;
    }
}

// cnt: COUNT_ROWS → ni + 1 counters (zeroed), COUNT_UNITS → one per unit. FILL: upos[units + 1] is read, ccol / src (nc entries each) are written.
// mult == NULL: J == NULL (q = c). jlist == NULL: the q's of column c are [jptr[c], jptr[c + 1]).
template <int MODE>
__global__ __launch_bounds__(WG) void ex_walk_kernel(int rows, int cols, const int32_t *__restrict__ rpt, const int32_t *__restrict__ col, int ni,
                                                     const int32_t *__restrict__ I, const int *__restrict__ mult, const int *__restrict__ jptr,
                                                     const int *__restrict__ jlist, const int *__restrict__ uoff, int units_cap, unsigned *__restrict__ cnt,
                                                     const unsigned *__restrict__ upos, long long nc, int32_t *__restrict__ ccol, int32_t *__restrict__ src,
                                                     ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    const int units = uoff[ni];
    if (units > units_cap || units < 0) {                          // the counts changed under the call
        if (threadIdx.x == 0) atomicOr(&st->fail, BAD_ROWPTR);
        return;
    }
    if (MODE == FILL && ((long long)upos[units] != nc || st->cnnz != (u64)nc)) {
        if (threadIdx.x == 0) atomicOr(&st->fail, BAD_CRPT);
        return;
    }
    UnitWalk w(units);
    const int lane = w.lane;
    int p = -1;
    u64 total = 0;
    bool bad = false;
    for (long long it = 0; it < w.chunk; it += kGroups) {          // the same trip count for every lane of the wave: the shuffles below are never divergent
        const long long ul = w.unit(it);
        const bool live = w.live(ul);
        long long k0 = 0, k1 = 0, pos = 0, uend = 0;
        if (live) {
            const int u = (int)ul;
            p = row_after(uoff, ni, p, u);
            const int r = I ? I[p] : p;
            if ((unsigned)r < (unsigned)rows) {
                k0 = rpt[r] + (long long)(u - uoff[p]) * kUnit;
                k1 = min(k0 + kUnit, (long long)rpt[r + 1]);
            }
            if (MODE == FILL) {
                pos = upos[u];
                uend = min((long long)upos[u + 1], nc);
            }
        }
        u64 kept = 0;
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const long long e = k0 + t * kLanes + lane;
            int c = 0;
            unsigned m = 0;
            if (e < k1) {
                c = col[e];
                if ((unsigned)c >= (unsigned)cols) bad = true;
                else m = mult ? (unsigned)mult[c] : 1u;
            }
            if (MODE == FILL) {
                const unsigned incl = group_inclusive(m, lane);
                const unsigned step = __shfl(incl, kLanes - 1, kLanes);
                long long o = pos + (incl - m);
                const int base = mult && m ? jptr[c] : 0;             // (m != 0: c has passed its range check)
                for (unsigned k = 0; k < m && o < uend; ++k, ++o) {   // one lane writes its run: a column that J names very many times is written sequentially
                    ccol[o] = mult ? (jlist ? jlist[base + k] : base + (int)k) : c;
                    src[o] = (int)e;
                }
                pos += step;
            } else {
                kept += m;
            }
        }
        if (MODE != FILL) {
            kept = group_sum(kept);
            if (live && lane == 0) {
                if (MODE == COUNT_ROWS) {
                    if (kept) atomicAdd(&cnt[p], (unsigned)kept);    // (wraps only where the 64-bit total below reports the overflow)
                } else {
                    cnt[(int)ul] = (unsigned)min(kept, (u64)UINT_MAX);
                }
                total += kept;
            }
        }
    }
    if (MODE != FILL) {
        workgroup_add_u64(&st->cnnz, total);
        if (bad) atomicOr(&st->fail, BAD_COL);
    }
}

// crpt[p] must be the slot of row p's first unit, p = 0 … ni (uoff[ni] = units, upos[units] = the entry count)
__global__ __launch_bounds__(WG) void ex_crpt_kernel(int ni, const int *__restrict__ uoff, int units_cap, const unsigned *__restrict__ upos,
                                                     const int32_t *__restrict__ crpt, ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    bool bad = false;
    for (long long p = (long long)blockIdx.x * WG + threadIdx.x; p <= ni; p += (long long)gridDim.x * WG) {
        const int u = uoff[p];
        bad |= (unsigned)u > (unsigned)units_cap || (unsigned)crpt[p] != upos[min(max(u, 0), units_cap)];
    }
    if (bad) atomicOr(&st->fail, BAD_CRPT);
}

// Behind a clean ex_crpt_kernel: crpt is non-decreasing from 0 to nc.
__global__ __launch_bounds__(WG) void ex_order_kernel(int ni, long long nc, const int32_t *__restrict__ crpt, const int32_t *__restrict__ ccol,
                                                      int *__restrict__ rowflag, const ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    for (long long x = (long long)blockIdx.x * WG + threadIdx.x + 1; x < nc; x += (long long)gridDim.x * WG) {
        if (ccol[x - 1] <= ccol[x]) continue;
        int lo = 0, hi = ni - 1;                                     // the last p with crpt[p] <= x: the row that holds x (crpt[ni] = nc > x)
        while (lo < hi) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            if (crpt[mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        if (crpt[lo] != x) rowflag[lo] = 1;                          // (a descent across a row boundary means nothing)
    }
}

// wlist / llist: ni ints each; lrows / llen: long_cap (+ 1 for the scan's total) ints each. A workgroup owns a run of consecutive rows and walks it twice:
// first it counts its rows of each list and takes its ranges with ONE atomic per list — an atomic that returns costs 16–28 ns on one address, and one per
// wave was 0.46 ms of a 3.5 ms call for 10^6 rows (profiles/extract.txt) — then it places the rows, ranks from ballots and the waves' counts in LDS.
__device__ __forceinline__ int row_class(long long p, const int32_t *__restrict__ crpt, const int *__restrict__ rowflag, int *len)
{
    *len = crpt[p + 1] - crpt[p];
    return !rowflag[p] ? 0 : (*len <= kWaveMax ? 1 : (*len <= kLdsMax ? 2 : 3));   // 0 in order, 1 wave, 2 LDS, 3 long
}

__global__ __launch_bounds__(WG) void ex_classify_kernel(int ni, const int32_t *__restrict__ crpt, const int *__restrict__ rowflag, int *__restrict__ wlist,
                                                         int *__restrict__ llist, int *__restrict__ lrows, int *__restrict__ llen, int long_cap,
                                                         ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    __shared__ int wcnt[3][WG / 64], first[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const long long chunk = (((long long)ni + gridDim.x - 1) / gridDim.x + WG - 1) / WG * WG;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = min(p0 + chunk, (long long)ni);
    int cnt[3] = {0, 0, 0}, len;
    for (long long p = p0 + threadIdx.x; p < p1; p += WG) {
        const int cls = row_class(p, crpt, rowflag, &len);
        if (cls < 3) ++cnt[cls];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off, 64);
        if (lane == 0) wcnt[k][wave] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < WG / 64; ++w) t += wcnt[threadIdx.x][w];
        int *counter = threadIdx.x == 0 ? &st->rows_in_order : (threadIdx.x == 1 ? &st->n_wave : &st->n_lds);
        first[threadIdx.x] = t ? atomicAdd(counter, t) : 0;
    }
    __syncthreads();
    int run1 = first[1], run2 = first[2];
    for (long long base = p0; base < p1; base += WG) {               // the same trip count for every thread of the workgroup
        const long long p = base + threadIdx.x;
        const int cls = p < p1 ? row_class(p, crpt, rowflag, &len) : -1;
        const u64 m1 = __ballot(cls == 1), m2 = __ballot(cls == 2);
        if (lane == 0) {
            wcnt[1][wave] = __popcll(m1);
            wcnt[2][wave] = __popcll(m2);
        }
        __syncthreads();
        int before1 = 0, before2 = 0, all1 = 0, all2 = 0;
#pragma unroll
        for (int w = 0; w < WG / 64; ++w) {
            if (w < wave) { before1 += wcnt[1][w]; before2 += wcnt[2][w]; }
            all1 += wcnt[1][w];
            all2 += wcnt[2][w];
        }
        if (cls == 1) wlist[run1 + before1 + __popcll(m1 & below)] = (int)p;
        if (cls == 2) llist[run2 + before2 + __popcll(m2 & below)] = (int)p;
        if (cls == 3) {                                              // few: a row of more than kLdsMax entries
            const int k = atomicAdd(&st->n_long, 1);
            if (k < long_cap) {
                lrows[k] = (int)p;
                llen[k] = len;
            }
            atomicAdd(&st->long_entries, (u64)len);
        }
        run1 += all1;
        run2 += all2;
        __syncthreads();
    }
}

// One wave per listed row of at most 64 entries: lane i holds entry i, a bitonic network over the lanes, the payload fetched from the lane the key names.
__global__ __launch_bounds__(WG) void ex_sort_wave_kernel(int n_rows, const int *__restrict__ wlist, const int32_t *__restrict__ crpt, int32_t *__restrict__ ccol,
                                                          int32_t *__restrict__ src)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WG / 64);
    for (long long i = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6); i < n_rows; i += waves) {   // uniform over the wave
        const int p = wlist[i];
        const long long x0 = crpt[p];
        const int len = min(crpt[p + 1] - crpt[p], kWaveMax);
        const bool live = lane < len;
        u64 key = live ? ((u64)(unsigned)ccol[x0 + lane] << 32 | (unsigned)lane) : ~0ull;
        const int s = live ? src[x0 + lane] : 0;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const u64 other = __shfl_xor(key, j, 64);
                const bool up = (lane & k) == 0, lower = (lane & j) == 0;
                key = (lower == up) ? min(key, other) : max(key, other);
            }
        }
        const int from = (int)(key & 63u);
        const int moved = __shfl(s, from, 64);
        if (live) {                                                  // the len live keys are below every pad: lane i < len holds the i-th of them
            ccol[x0 + lane] = (int)(key >> 32);
            src[x0 + lane] = moved;
        }
    }
}

// One workgroup per listed row of at most kLdsMax entries: keys (q << 32 | position) in LDS, padded with ~0 to the next power of two, a bitonic network.
// Consecutive threads take consecutive pairs: for a compare distance j >= 32 elements a half-wave reads 256 contiguous bytes (no bank conflict), below
// that its 8-byte words are 16 bytes apart (2-way).
__global__ __launch_bounds__(WG) void ex_sort_lds_kernel(int n_rows, const int *__restrict__ llist, const int32_t *__restrict__ crpt, int32_t *__restrict__ ccol,
                                                         int32_t *__restrict__ src)
{
    __shared__ u64 keys[kLdsMax];
    __shared__ int pay[kLdsMax];
    for (int i = blockIdx.x; i < n_rows; i += gridDim.x) {
        const int p = llist[i];
        const long long x0 = crpt[p];
        const int len = min(crpt[p + 1] - crpt[p], kLdsMax);
        int n2 = 128;
        while (n2 < len) n2 <<= 1;
        for (int t = threadIdx.x; t < n2; t += WG) {
            keys[t] = t < len ? ((u64)(unsigned)ccol[x0 + t] << 32 | (unsigned)t) : ~0ull;
            if (t < len) pay[t] = src[x0 + t];
        }
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < (n2 >> 1); t += WG) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const u64 a = keys[lo], b = keys[hi];
                    if ((a > b) == ((lo & k) == 0)) {
                        keys[lo] = b;
                        keys[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        for (int t = threadIdx.x; t < len; t += WG) {
            const u64 key = keys[t];
            ccol[x0 + t] = (int)(key >> 32);
            src[x0 + t] = pay[(int)(key & 0xffffffffu) & (kLdsMax - 1)];
        }
        __syncthreads();
    }
}

// The entries of the k-th long row to the compact list at loff[k]: (k, q, src). One workgroup per row at a time.
__global__ __launch_bounds__(WG) void ex_long_gather_kernel(int n_long, const int *__restrict__ lrows, const int *__restrict__ loff, long long n_entries,
                                                            const int32_t *__restrict__ crpt, const int32_t *__restrict__ ccol, const int32_t *__restrict__ src,
                                                            int32_t *__restrict__ rrow, int32_t *__restrict__ rq, int32_t *__restrict__ rsrc)
{
    for (int k = blockIdx.x; k < n_long; k += gridDim.x) {
        const int p = lrows[k];
        const long long x0 = crpt[p], o0 = loff[k];
        const int len = crpt[p + 1] - crpt[p];
        for (int t = threadIdx.x; t < len && o0 + t < n_entries; t += WG) {
            rrow[o0 + t] = k;
            rq[o0 + t] = ccol[x0 + t];
            rsrc[o0 + t] = src[x0 + t];
        }
    }
}

// perm (of g4s_csr_from_coo_symbolic, G4S_DUP_KEEP): the compact index behind every position of the (rank, q, compact index) order. Row k keeps its
// range [loff[k], loff[k + 1]) in that order, so position x is entry x − loff[k] of row lrows[k].
__global__ __launch_bounds__(WG) void ex_long_apply_kernel(int n_long, long long n_entries, const int *__restrict__ lrows, const int *__restrict__ loff,
                                                           const int32_t *__restrict__ perm, const int32_t *__restrict__ rrow, const int32_t *__restrict__ rq,
                                                           const int32_t *__restrict__ rsrc, const int32_t *__restrict__ crpt, int32_t *__restrict__ ccol,
                                                           int32_t *__restrict__ src)
{
    for (long long x = (long long)blockIdx.x * WG + threadIdx.x; x < n_entries; x += (long long)gridDim.x * WG) {
        const int in = perm[x];
        if ((u64)(unsigned)in >= (u64)n_entries) continue;
        const int k = rrow[in];
        if ((unsigned)k >= (unsigned)n_long) continue;
        const int p = lrows[k];
        const long long t = x - loff[k];
        if (t < 0 || t >= (long long)crpt[p + 1] - crpt[p]) continue;
        ccol[crpt[p] + t] = rq[in];
        src[crpt[p] + t] = rsrc[in];
    }
}

// Behind a clean fill: every src element is an index into val.
__global__ __launch_bounds__(WG) void ex_values_kernel(int ni, long long nc, long long nnz_a, const int32_t *__restrict__ src, const double *__restrict__ val,
                                                       double *__restrict__ cval, const ExState *__restrict__ st)
{
    if (dead(st, ni)) return;
    for (long long x = (long long)blockIdx.x * WG + threadIdx.x; x < nc; x += (long long)gridDim.x * WG) {
        const int e = src[x];
        if ((u64)(unsigned)e < (u64)nnz_a) cval[x] = val[e];
    }
}

// The operands of one call, device arrays.
struct Job {
    const char *fn;
    int rows, cols;
    const int32_t *rpt, *col;
    const double *val;
    int ni;
    const int32_t *I;
    int nj;
    const int32_t *J;
};

int contract_error(const Job &j, int fail)
{
    if (fail & BAD_ROWPTR) return g4s::set_error(G4S_ERR_INVALID, "%s: rpt is not zero-based and non-decreasing", j.fn);
    if (fail & BAD_ID) return g4s::set_error(G4S_ERR_INVALID, "%s: an id of I or J is outside [0, %d) x [0, %d)", j.fn, j.rows, j.cols);
    if (fail & BAD_COL) return g4s::set_error(G4S_ERR_INVALID, "%s: a column id of A is outside [0, %d)", j.fn, j.cols);
    return g4s::set_error(G4S_ERR_INVALID, "%s: crpt is not the row pointer of this extraction: crpt must come from the symbolic call", j.fn);
}

void report(g4s_extract_info *info, const ExState &h, long long units, bool has_j, int waits)
{
    info->nnz_a = h.nnz_a;
    info->nnz_rows = (int64_t)h.nnz_rows;
    info->nnz_c = (int64_t)h.cnnz;
    info->units = units;
    info->unit_entries = kUnit;
    info->j_kind = !has_j ? 0 : (h.j_unsorted ? 2 : 1);
    info->rows_in_order = h.rows_in_order;
    info->rows_sorted_wave = h.n_wave;
    info->rows_sorted_lds = h.n_lds;
    info->rows_sorted_radix = h.n_long;
    info->lds_sort_max = kLdsMax;
    info->host_waits = waits;
}

// The state, the unit table of the output rows and the column map: what both calls start with. Enqueues only.
struct Front {
    Carver work;
    ExState *st = nullptr;
    int *upr = nullptr, *uoff = nullptr, *mult = nullptr, *jptr = nullptr;
    unsigned *cnt = nullptr;                                        // ni + 1 counters, zeroed (the symbolic call's)
    int build(const Job &j, bool with_cnt, hipStream_t s)
    {
        const size_t n1 = 4 * ((size_t)j.ni + 1), c1 = 4 * ((size_t)j.cols + 1);
        work.piece(&st, sizeof(ExState));
        work.piece(&upr, n1);
        work.piece(&uoff, n1);
        if (with_cnt) work.piece(&cnt, n1);
        if (j.J) {
            work.piece(&mult, c1);
            work.piece(&jptr, c1);
        }
        G4S_TRY(work.alloc());
        if (with_cnt) G4S_HIP_TRY(hipMemsetAsync(cnt, 0, n1, s));
        if (j.J) G4S_HIP_TRY(hipMemsetAsync(mult, 0, c1, s));
        G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(ExState), s));
        const long long n = (long long)std::max(j.rows, std::max(j.ni, j.nj)) + 1;
        hipLaunchKernelGGL(ex_check_kernel, dim3(std::min(grid_for<WG>(n, kGridWG), kCheckWG)), dim3(WG), 0, s, j.rows, j.cols, j.rpt, j.ni, j.I, j.nj, j.J, upr, mult, st);
        G4S_HIP_TRY(hipGetLastError());
        G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(upr), uoff, (long long)j.ni + 1, s));
        if (j.J) G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(mult), jptr, (long long)j.cols + 1, s));
        return G4S_OK;
    }
};

#define WALK_ARGS(j, f) (j).rows, (j).cols, (j).rpt, (j).col, (j).ni, (j).I, static_cast<const int *>((f).mult), static_cast<const int *>((f).jptr)

// Device arrays; the stream is synchronised on return. crpt: ni + 1 ints, written. One wait.
int symbolic_device(const Job &j, int32_t *crpt, int64_t *cnnz, g4s_extract_info *info, hipStream_t s)
{
    Front f;
    g4s::ReadScope reads(s);
    ExState h{};
    int units = 0;
    G4S_TRY(f.build(j, true, s));
    hipLaunchKernelGGL(ex_walk_kernel<COUNT_ROWS>, dim3(kGridWG), dim3(WG), 0, s, WALK_ARGS(j, f), (const int *)nullptr, static_cast<const int *>(f.uoff), INT_MAX,
                       f.cnt, (const unsigned *)nullptr, 0LL, (int32_t *)nullptr, (int32_t *)nullptr, f.st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const unsigned *>(f.cnt), reinterpret_cast<unsigned *>(crpt), (long long)j.ni + 1, s));
    G4S_HIP_TRY(reads.note(h, f.st));
    G4S_HIP_TRY(reads.note(units, f.uoff + j.ni));
    G4S_HIP_TRY(reads.wait());
    f.work.idle();                                                 // (an early return above leaves it out: the block is then released behind a device-wide wait)
    if (h.fail) return contract_error(j, h.fail);
    if (too_many_units(j.ni, h.nnz_rows)) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: more than 2^31 work units", j.fn);
    report(info, h, units, j.J != nullptr, 1);
    *cnnz = (int64_t)h.cnnz;
    if (h.cnnz > (u64)INT32_MAX) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: %llu entries exceed the int32 row pointers", j.fn, h.cnnz);
    return G4S_OK;
}

// The rows longer than kLdsMax that are out of order: compacted, sorted by g4s_csr_from_coo_symbolic (its waits are its own), written back.
int sort_long_rows(const Job &j, const ExState &h, const int *lrows, int *llen, const int32_t *crpt, int32_t *ccol, int32_t *src, int *coo_waits, hipStream_t s)
{
    const long long ne = (long long)h.long_entries;
    const int nl = h.n_long;
    const size_t eb = 4 * (size_t)ne, lb = 4 * ((size_t)nl + 1);
    int32_t *rrow, *rq, *rsrc, *perm, *rcrpt;
    int *loff;
    Carver buf;
    buf.piece(&rrow, eb);
    buf.piece(&rq, eb);
    buf.piece(&rsrc, eb);
    buf.piece(&perm, eb);
    buf.piece(&rcrpt, lb);
    buf.piece(&loff, lb);
    G4S_TRY(buf.alloc());
    G4S_HIP_TRY(hipMemsetAsync(llen + nl, 0, 4, s));
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(llen), loff, (long long)nl + 1, s));
    hipLaunchKernelGGL(ex_long_gather_kernel, dim3(std::min(nl, kGridWG)), dim3(WG), 0, s, nl, lrows, static_cast<const int *>(loff), ne, crpt,
                       static_cast<const int32_t *>(ccol), static_cast<const int32_t *>(src), rrow, rq, rsrc);
    G4S_HIP_TRY(hipGetLastError());
    int64_t cn = 0;
    g4s_coo_info ci{};
    G4S_TRY(g4s_csr_from_coo_symbolic(G4S_DUP_KEEP, nl, std::max(j.nj, 1), ne, rrow, rq, rcrpt, perm, &cn, G4S_DEVICE_POINTERS, &ci, s));
    *coo_waits = ci.host_waits;
    hipLaunchKernelGGL(ex_long_apply_kernel, dim3(grid_for<WG>(ne, kGridWG)), dim3(WG), 0, s, nl, ne, lrows, static_cast<const int *>(loff), static_cast<const int32_t *>(perm),
                       static_cast<const int32_t *>(rrow), static_cast<const int32_t *>(rq), static_cast<const int32_t *>(rsrc), crpt, ccol, src);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(hipStreamSynchronize(s));                          // the block goes back idle; the caller's last wait follows at once
    buf.idle();
    return G4S_OK;
}

// Device arrays; the stream is synchronised on return. src may be NULL. h_* (host arrays, or NULL): the copies a caller with host pointers wants,
// enqueued in front of the last wait. Two waits when every row comes out of the fill in order, three when rows are sorted, plus those of
// g4s_csr_from_coo_symbolic and one more when rows longer than kLdsMax are.
int numeric_device(const Job &j, const int32_t *crpt, int32_t *ccol, double *cval, int32_t *src, g4s_extract_info *info, int32_t *h_ccol, double *h_cval,
                   int32_t *h_src, hipStream_t s)
{
    Front f;
    g4s::ReadScope reads(s);
    ExState h{};
    int units = 0, nc32 = 0, waits = 0;
    G4S_TRY(f.build(j, false, s));
    G4S_HIP_TRY(reads.note(h, f.st));
    G4S_HIP_TRY(reads.note(units, f.uoff + j.ni));
    G4S_HIP_TRY(reads.note(nc32, crpt + j.ni));
    G4S_HIP_TRY(reads.wait());
    ++waits;
    auto refuse = [&](int st) { f.work.idle(); return st; };
    if (h.fail) return refuse(contract_error(j, h.fail));
    if (too_many_units(j.ni, h.nnz_rows)) return refuse(g4s::set_error(G4S_ERR_OVERFLOW, "%s: more than 2^31 work units", j.fn));
    if (nc32 < 0 || units < 0) return refuse(g4s::set_error(G4S_ERR_INVALID, "%s: crpt[ni] = %d is not an entry count: crpt must come from the symbolic call", j.fn, nc32));
    const long long nc = nc32, na = h.nnz_a;
    {
        const Span outs[] = {{ccol, 4 * (size_t)nc}, {cval, 8 * (size_t)nc}, {src, 4 * (size_t)nc}},
                   ins[] = {{j.rpt, 4 * ((size_t)j.rows + 1)}, {j.col, 4 * (size_t)na}, {j.val, 8 * (size_t)na}, {j.I, 4 * (size_t)j.ni}, {j.J, 4 * (size_t)j.nj},
                            {crpt, 4 * ((size_t)j.ni + 1)}};
        if (any_overlap(outs, ins)) return refuse(g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input or another output", j.fn));
    }
    const bool jl = j.J && h.j_unsorted;
    const int long_cap = (int)(nc / (kLdsMax + 1)) + 1;
    const size_t ub = 4 * ((size_t)units + 1), nb = 4 * ((size_t)j.ni + 1), cb = 4 * ((size_t)j.cols + 1), lb = 4 * ((size_t)long_cap + 1);
    unsigned *ucnt, *upos;
    int *rowflag, *wlist, *llist, *jlist = nullptr, *cursor = nullptr, *lrows, *llen;
    Carver work;
    work.piece(&ucnt, ub);
    work.piece(&upos, ub);
    work.piece(&rowflag, nb);
    work.piece(&wlist, nb);
    work.piece(&llist, nb);
    if (jl) {
        work.piece(&jlist, 4 * (size_t)j.nj);
        work.piece(&cursor, cb);
    }
    if (!src) work.piece(&src, 4 * (size_t)nc);
    work.piece(&lrows, lb);
    work.piece(&llen, lb);
    G4S_TRY(work.alloc());
    G4S_HIP_TRY(hipMemsetAsync(ucnt, 0, ub, s));
    G4S_HIP_TRY(hipMemsetAsync(rowflag, 0, nb, s));
    if (jl) {
        G4S_HIP_TRY(hipMemsetAsync(cursor, 0, cb, s));
        hipLaunchKernelGGL(ex_jlist_kernel, dim3(grid_for<WG>(j.nj, kGridWG)), dim3(WG), 0, s, j.ni, j.nj, j.J, static_cast<const int *>(f.jptr), cursor, jlist, f.st);
    }
    hipLaunchKernelGGL(ex_walk_kernel<COUNT_UNITS>, dim3(kGridWG), dim3(WG), 0, s, WALK_ARGS(j, f), (const int *)nullptr, static_cast<const int *>(f.uoff), units, ucnt,
                       (const unsigned *)nullptr, 0LL, (int32_t *)nullptr, (int32_t *)nullptr, f.st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const unsigned *>(ucnt), upos, (long long)units + 1, s));
    hipLaunchKernelGGL(ex_crpt_kernel, dim3(grid_for<WG>((long long)j.ni + 1, kGridWG)), dim3(WG), 0, s, j.ni, static_cast<const int *>(f.uoff), units,
                       static_cast<const unsigned *>(upos), crpt, f.st);
    hipLaunchKernelGGL(ex_walk_kernel<FILL>, dim3(kGridWG), dim3(WG), 0, s, WALK_ARGS(j, f), static_cast<const int *>(jlist), static_cast<const int *>(f.uoff), units,
                       (unsigned *)nullptr, static_cast<const unsigned *>(upos), nc, ccol, src, f.st);
    hipLaunchKernelGGL(ex_order_kernel, dim3(grid_for<WG>(nc, kGridWG)), dim3(WG), 0, s, j.ni, nc, crpt, static_cast<const int32_t *>(ccol), rowflag, f.st);
    hipLaunchKernelGGL(ex_classify_kernel, dim3(std::min(grid_for<WG>(j.ni, kGridWG), kClassifyWG)), dim3(WG), 0, s, j.ni, crpt, static_cast<const int *>(rowflag), wlist, llist, lrows, llen, long_cap, f.st);
    G4S_HIP_TRY(hipGetLastError());
    auto finish = [&]() -> int {                                     // the values, the copies for a caller with host arrays; then the state
        if (cval) hipLaunchKernelGGL(ex_values_kernel, dim3(grid_for<WG>(nc, kGridWG)), dim3(WG), 0, s, j.ni, nc, na, static_cast<const int32_t *>(src), j.val, cval, f.st);
        G4S_HIP_TRY(hipGetLastError());
        if (nc > 0) {
            if (h_ccol) G4S_HIP_TRY(hipMemcpyAsync(h_ccol, ccol, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
            if (h_cval) G4S_HIP_TRY(hipMemcpyAsync(h_cval, cval, 8 * (size_t)nc, hipMemcpyDeviceToHost, s));
            if (h_src) G4S_HIP_TRY(hipMemcpyAsync(h_src, src, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
        }
        G4S_HIP_TRY(reads.fetch(h, f.st));
        ++waits;
        return G4S_OK;
    };
    G4S_TRY(finish());                                             // rows in order need nothing more: this is then the last wait
    if (!h.fail && (h.n_wave || h.n_lds || h.n_long)) {
        if (h.n_wave) hipLaunchKernelGGL(ex_sort_wave_kernel, dim3(std::min((h.n_wave + 3) / 4, kGridWG)), dim3(WG), 0, s, h.n_wave, static_cast<const int *>(wlist), crpt, ccol, src);
        if (h.n_lds) hipLaunchKernelGGL(ex_sort_lds_kernel, dim3(std::min(h.n_lds, kGridWG)), dim3(WG), 0, s, h.n_lds, static_cast<const int *>(llist), crpt, ccol, src);
        G4S_HIP_TRY(hipGetLastError());
        if (h.n_long) {
            if (h.n_long > long_cap || h.long_entries > (u64)nc) return g4s::set_error(G4S_ERR_INVALID, "%s: the arrays changed under the call", j.fn);
            int coo_waits = 0;
            G4S_TRY(sort_long_rows(j, h, lrows, llen, crpt, ccol, src, &coo_waits, s));
            waits += coo_waits + 1;
        }
        G4S_TRY(finish());
    }
    f.work.idle();                                                 // (an early return above leaves them out: released behind a device-wide wait)
    work.idle();
    if (h.fail) return contract_error(j, h.fail);
    report(info, h, units, j.J != nullptr, waits);
    return G4S_OK;
}

int symbolic(const Job &j, int32_t *crpt, int64_t *cnnz, unsigned flags, g4s_extract_info *info, hipStream_t s)
{
    const size_t rp = 4 * ((size_t)j.rows + 1), cp = 4 * ((size_t)j.ni + 1);
    const bool dev = flags & G4S_DEVICE_POINTERS;
    long long na = 0;
    if (!dev) {
        na = j.rpt[j.rows];
        if (na < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: a negative entry count", j.fn);
        const Span outs[] = {{crpt, cp}, {cnnz, sizeof(int64_t)}}, ins[] = {{j.rpt, rp}, {j.col, 4 * (size_t)na}, {j.I, 4 * (size_t)j.ni}, {j.J, 4 * (size_t)j.nj}};
        if (any_overlap(outs, ins)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input or another output", j.fn);
    }
    G4S_TRY(not_capturing(j.fn, s));
    g4s_extract_info local{};
    if (!info) info = &local;
    *info = g4s_extract_info{};
    *cnnz = 0;
    if (dev) return symbolic_device(j, crpt, cnnz, info, s);
    Staged stage(s);
    Job d = j;
    d.rpt = stage.in(j.rpt, rp);
    d.col = stage.in(j.col, 4 * (size_t)na);
    d.val = nullptr;
    d.I = stage.in(j.I, 4 * (size_t)j.ni);
    d.J = stage.in(j.J, 4 * (size_t)j.nj);
    int32_t *d_crpt = stage.out<int32_t>(cp);
    int status = stage.error();
    if (status == G4S_OK) status = symbolic_device(d, d_crpt, cnnz, info, s);
    if (status == G4S_OK) status = stage.to_host(crpt, d_crpt, cp);
    if (status == G4S_OK) status = stage.wait();
    return stage.finish(status);
}

int numeric(const Job &j, const int32_t *crpt, int32_t *ccol, double *cval, int32_t *src, unsigned flags, g4s_extract_info *info, hipStream_t s)
{
    const size_t rp = 4 * ((size_t)j.rows + 1), cp = 4 * ((size_t)j.ni + 1);
    const bool dev = flags & G4S_DEVICE_POINTERS;
    long long na = 0, nc = 0;
    if (!dev) {
        na = j.rpt[j.rows];
        nc = crpt[j.ni];
        if (na < 0 || nc < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: a negative entry count", j.fn);
        const Span outs[] = {{ccol, 4 * (size_t)nc}, {cval, 8 * (size_t)nc}, {src, 4 * (size_t)nc}},
                   ins[] = {{j.rpt, rp}, {j.col, 4 * (size_t)na}, {j.val, 8 * (size_t)na}, {j.I, 4 * (size_t)j.ni}, {j.J, 4 * (size_t)j.nj}, {crpt, cp}};
        if (any_overlap(outs, ins)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input or another output", j.fn);
    }
    G4S_TRY(not_capturing(j.fn, s));
    g4s_extract_info local{};
    if (!info) info = &local;
    *info = g4s_extract_info{};
    if (dev) return numeric_device(j, crpt, ccol, cval, src, info, nullptr, nullptr, nullptr, s);
    Staged stage(s);
    Job d = j;
    d.rpt = stage.in(j.rpt, rp);
    d.col = stage.in(j.col, 4 * (size_t)na);
    d.val = stage.in(j.val, 8 * (size_t)na);
    d.I = stage.in(j.I, 4 * (size_t)j.ni);
    d.J = stage.in(j.J, 4 * (size_t)j.nj);
    const int32_t *d_crpt = stage.in(crpt, cp);
    int32_t *d_ccol = stage.out<int32_t>(4 * (size_t)nc);
    double *d_cval = cval ? stage.out<double>(8 * (size_t)nc) : nullptr;
    int32_t *d_src = src ? stage.out<int32_t>(4 * (size_t)nc) : nullptr;
    int status = stage.error();
    if (status == G4S_OK) status = numeric_device(d, d_crpt, d_ccol, d_cval, d_src, info, ccol, cval, src, s);   // the copies to ccol / cval / src: its own
    return stage.finish(status);
}

} // namespace

G4S_API g4s_status g4s_csr_extract_symbolic(int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, int32_t ni, const int32_t *I, int32_t nj,
                                            const int32_t *J, int32_t *crpt, int64_t *cnnz, unsigned flags, g4s_extract_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(rows >= 0 && cols >= 0 && ni >= 0 && nj >= 0, "negative dimension or list length");
    G4S_REQUIRE(rpt && crpt && cnnz, "rpt, crpt or cnnz is NULL");
    G4S_REQUIRE(col || rows == 0, "col is NULL");
    G4S_REQUIRE(I || ni == rows, "I == NULL means every row: ni must equal rows");
    G4S_REQUIRE(J || nj == cols, "J == NULL means every column: nj must equal cols");
    const Job j{__func__, rows, cols, rpt, col, nullptr, ni, I, nj, J};
    return symbolic(j, crpt, cnnz, flags, info, g4s::as_stream(stream));
}

G4S_API g4s_status g4s_csr_extract_numeric(int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, const double *val, int32_t ni, const int32_t *I,
                                           int32_t nj, const int32_t *J, const int32_t *crpt, int32_t *ccol, double *cval, int32_t *src, unsigned flags,
                                           g4s_extract_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(rows >= 0 && cols >= 0 && ni >= 0 && nj >= 0, "negative dimension or list length");
    G4S_REQUIRE(rpt && crpt, "rpt or crpt is NULL");
    G4S_REQUIRE(col || rows == 0, "col is NULL");
    G4S_REQUIRE(ccol || ni == 0 || nj == 0, "ccol is NULL");
    G4S_REQUIRE(I || ni == rows, "I == NULL means every row: ni must equal rows");
    G4S_REQUIRE(J || nj == cols, "J == NULL means every column: nj must equal cols");
    G4S_REQUIRE((val == nullptr) == (cval == nullptr), "val and cval must both be given or both be NULL (pattern-only)");
    const Job j{__func__, rows, cols, rpt, col, val, ni, I, nj, J};
    return numeric(j, crpt, ccol, cval, src, flags, info, g4s::as_stream(stream));
}
