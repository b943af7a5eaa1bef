// spgemm_masked.hip — g4s_spgemm_masked and g4s_triangle_count (include/g4s.h): C⟨M⟩ = A ⊗ B, the product computed only at the positions of a given
// pattern M, over the four semirings of semiring.hpp, with values or pattern-only (every stored value counts as 1.0 and no value array is read).
//
// The pattern of C is M, so there is no symbolic phase, no output allocation and no crpt. Row i walks the products of the full SpGEMM (Gustavson:
// for p in A(i,:), for (j, b) in B(p,:)) and keeps those whose column is found in the sorted mask row M(i,:), which is the accumulator's key set.
//
//   opening pass   mk_open_kernel, 8 lanes per row: nnz(M(i,:)), flop(i) = Σ_{p ∈ A(i,:)} nnz(B(p,:)), the checks of the contract (mask rows strictly
//                  ascending with ids in [0, N), row pointers in range, A's column ids in [0, K)) and the row's class as a sort key. One 4-bit pass of
//                  prims::sort_pairs_descending (stable) turns the keys into the class lists; the host reads the class counts and the error word once.
//                  cval is filled with the semiring's identity beforehand, so rows with an empty mask row or no products are done.
//   wave           nnz(M(i,:)) <= 64 and flop(i) <= 4096: one wavefront per row, four rows per workgroup, no workgroup barrier. The mask row (padded
//                  with INT_MAX) and one value slot per column sit in the wave's LDS slice; 64 entries of A at a time are scanned by their B row lengths
//                  and the lanes walk the concatenated B rows; lookup is a 6-step lower bound.
//   LDS            one workgroup per row, the mask row's columns and value slots in LDS (12 bytes per entry): up to 1024 entries with 256 threads
//                  (17 KiB, eight workgroups per CU), up to 8192 with 1024 threads (116 KiB, one per CU: sixteen waves). Lanes walk the concatenated B
//                  rows of a tile of A entries as traverse.hip's push kernel walks a frontier (degree scan in LDS + monotone search), products outside
//                  [min M(i,:), max M(i,:)] are dropped by two compares, the rest looked up by binary search. One coalesced store of the row at the end.
//   global         a mask row longer than the LDS table: the same walk, the binary search runs over the row of mcol in HBM / L2 and hits go to cval by
//                  S::global_acc.
//   split          flop(i) above 2^20: the row's tiles of A entries are dealt over up to 128 workgroups. A mask row of at most 1024 entries is a private
//                  LDS table per workgroup, folded into cval by S::global_acc (slots still at the identity are skipped); a longer one is the global
//                  class with several workgroups. The grid is rows × ways; a workgroup whose first tile lies behind the row's end returns.
// Kernel boundaries are the only ordering between workgroups; every loop is bounded by a row length or a tile's product count.
// Exactness: min, max and or do not depend on the order of arrival, so the three semirings are exact in every class. Plus-times adds in the order the
// atomics land (LDS or HBM): within 1e-10·Σ|a·b| of the left-to-right sum, and exact whenever all partial sums are representable.
// Environment switches: G4S_MASKED_WAVE_FLOP, G4S_MASKED_LDS_SMALL, G4S_MASKED_LDS_LARGE, G4S_MASKED_SPLIT_FLOP, G4S_MASKED_SPLIT_WAYS
// move the class boundaries (only downwards for the two LDS table sizes); they exist to cross-check one class against another.
#include "common.hpp"
#include "prims.hpp"
#include "readback.hpp"
#include "semiring.hpp"
#include "call_util.hpp"
#include <algorithm>
#include <climits>

namespace {

namespace sr = g4s::semiring;

constexpr int WG = 256;
constexpr int kOpenLpr = 8;                 // lanes per row in the opening pass
constexpr int kWaveMask = 64;               // the wave class keeps one mask column per lane
constexpr int kLdsSmall = 1024, kLdsLarge = 8192;
constexpr int kWgLarge = 1024;              // threads of the workgroup that holds a large table
constexpr long long kWaveFlop = 4096;
constexpr long long kSplitFlop = 1ll << 20;
constexpr int kSplitWays = 128;
constexpr int kSumBlocks = 1024;

enum { C_SKIP = 0, C_WAVE, C_LDS_S, C_LDS_L, C_GLOBAL, C_SPLIT_LDS, C_SPLIT_GLOBAL, C_COUNT };
enum { BAD_MASK = 1, BAD_A = 2, BAD_B = 4 };

struct Cuts {
    long long wave_flop, split_flop;
    int lds_small, lds_large, split_ways;
};

struct OpenState {
    unsigned long long products;
    int invalid;
    int counts[C_COUNT];
};

struct Operands {
    int M, K, N;
    const int *arpt, *acol;
    const double *aval;
    const int *brpt, *bcol;
    const double *bval;
    const int *mrpt, *mcol;
    double *cval;
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(WG) void mk_fill_kernel(long long n, double v, double *__restrict__ out)
{
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < n; k += (long long)gridDim.x * WG) out[k] = v;
}

__global__ __launch_bounds__(WG) void mk_check_b_kernel(long long bnnz, int N, const int *__restrict__ bcol, OpenState *st)
{
    int bad = 0;
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < bnnz; k += (long long)gridDim.x * WG) bad |= (unsigned)bcol[k] >= (unsigned)N;
    if (bad) atomicOr(&st->invalid, BAD_B);
}

// Per row: the length of its mask row, its products, the checks, its class.
__global__ __launch_bounds__(WG) void mk_open_kernel(int M, int K, int N, int annz, int bnnz, int mnnz, const int *__restrict__ arpt, const int *__restrict__ acol,
                                                     const int *__restrict__ brpt, const int *__restrict__ mrpt, const int *__restrict__ mcol,
                                                     int *__restrict__ keys, int *__restrict__ ids, OpenState *st, const Cuts cuts)
{
    __shared__ int s_cnt[C_COUNT];
    __shared__ int s_bad;
    __shared__ unsigned long long s_prod;
    if (threadIdx.x < C_COUNT) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_bad = 0; s_prod = 0ull; }
    __syncthreads();
    const int l = (int)threadIdx.x % kOpenLpr;
    const long long row = (long long)blockIdx.x * (WG / kOpenLpr) + threadIdx.x / kOpenLpr;
    int bad = 0, mlen = 0;
    long long flop = 0;
    if (row < M) {
        const int mb = mrpt[row], me = mrpt[row + 1];
        if (mb < 0 || me < mb || me > mnnz || (row == 0 && mb != 0)) bad |= BAD_MASK;
        else {
            mlen = me - mb;
            for (int k = mb + l; k < me; k += kOpenLpr) {
                const int c = mcol[k];
                if ((unsigned)c >= (unsigned)N) bad |= BAD_MASK;
                if (k > mb && mcol[k - 1] >= c) bad |= BAD_MASK;
            }
        }
        const int ab = arpt[row], ae = arpt[row + 1];
        if (ab < 0 || ae < ab || ae > annz) bad |= BAD_A;
        else {
            for (int k = ab + l; k < ae; k += kOpenLpr) {
                const int p = acol[k];
                if ((unsigned)p >= (unsigned)K) { bad |= BAD_A; continue; }
                const int bs = brpt[p], be = brpt[p + 1];
                if (bs < 0 || be < bs || be > bnnz) { bad |= BAD_B; continue; }
                flop += be - bs;
            }
        }
    }
    for (int o = kOpenLpr / 2; o > 0; o >>= 1) {
        flop += __shfl_xor(flop, o);
        bad |= __shfl_xor(bad, o);
    }
    if (row < M && l == 0) {
        int c = C_SKIP;
        if (!bad && mlen > 0 && flop > 0) {
            if (flop > cuts.split_flop) c = mlen <= cuts.lds_small ? C_SPLIT_LDS : C_SPLIT_GLOBAL;
            else if (mlen <= kWaveMask && flop <= cuts.wave_flop) c = C_WAVE;
            else if (mlen <= cuts.lds_small) c = C_LDS_S;
            else if (mlen <= cuts.lds_large) c = C_LDS_L;
            else c = C_GLOBAL;
            atomicAdd(&s_prod, (unsigned long long)flop);
        }
        keys[row] = c;
        ids[row] = (int)row;
        atomicAdd(&s_cnt[c], 1);
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x < C_COUNT && s_cnt[threadIdx.x]) atomicAdd(&st->counts[threadIdx.x], s_cnt[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (s_prod) atomicAdd(&st->products, s_prod);
        if (s_bad) atomicOr(&st->invalid, s_bad);
    }
}

// The wave class: row list[blockIdx.x · 4 + wave]; everything the wave shares is its own LDS slice, ordered by wave_sync only.
template <typename S, bool VALUES>
__global__ __launch_bounds__(WG) void mk_wave_kernel(const int *__restrict__ list, int nrows, const int *__restrict__ arpt, const int *__restrict__ acol,
                                                     const double *__restrict__ aval, const int *__restrict__ brpt, const int *__restrict__ bcol,
                                                     const double *__restrict__ bval, const int *__restrict__ mrpt, const int *__restrict__ mcol,
                                                     double *__restrict__ cval)
{
    __shared__ double s_val[WG / 64][64], s_av[WG / 64][64];
    __shared__ int s_col[WG / 64][64], s_start[WG / 64][64], s_scan[WG / 64][66];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * (WG / 64) + wave;
    if (idx >= nrows) return;
    const int row = list[idx];
    const int ab = arpt[row], ae = arpt[row + 1], mb = mrpt[row], mlen = mrpt[row + 1] - mb;
    s_col[wave][lane] = lane < mlen ? mcol[mb + lane] : INT_MAX;
    s_val[wave][lane] = S::identity();
    for (int a0 = ab; a0 < ae; a0 += 64) {
        const int i = a0 + lane;
        int start = 0, deg = 0;
        double av = 1.0;
        if (i < ae) {
            const int p = acol[i];
            start = brpt[p];
            deg = brpt[p + 1] - start;
            if constexpr (VALUES) av = aval[i];
        }
        const int x = g4s::prims::wave_inclusive(deg);
        wave_sync();                                               // the walk of the tile before is over
        s_start[wave][lane] = start;
        s_av[wave][lane] = av;
        s_scan[wave][lane + 1] = x;
        if (lane == 0) s_scan[wave][0] = 0;
        wave_sync();
        const int total = s_scan[wave][64];                        // at most the row's products: <= the wave class's cut
        int lo = 0;                                                // the last entry with s_scan[lo] <= e: never decreases as e grows
        for (int e0 = 0; e0 < total; e0 += 64) {
            const int e = e0 + lane;
            if (e < total) {
                int hi = 63;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_scan[wave][mid] <= e) lo = mid;
                    else hi = mid - 1;
                }
                const int k = s_start[wave][lo] + (e - s_scan[wave][lo]);
                const int j = bcol[k];
                int q = 0;                                         // lower bound over the 64 padded columns
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (s_col[wave][q + step - 1] < j) q += step;
                if (s_col[wave][q] == j) {
                    double v;
                    if constexpr (VALUES) v = S::mul(s_av[wave][lo], bval[k]);
                    else v = S::mul(1.0, 1.0);
                    S::lds_acc(&s_val[wave][q], v);
                }
            }
        }
    }
    wave_sync();
    if (lane < mlen) cval[mb + lane] = s_val[wave][lane];
}

constexpr size_t row_kernel_lds(int tpb, int cap) { return 8 * ((size_t)tpb + 2 + tpb / 64 + tpb + cap) + 4 * ((size_t)tpb + cap); }

// The LDS, global and split classes: workgroup blockIdx.x takes row list[blockIdx.x / ways] and, of its tiles of TPB entries of A, every ways-th from
// blockIdx.x % ways on. GLOBAL: the mask row is searched where it lies and hits go to cval (pre-filled with the identity) by global atomics; otherwise
// the row's columns and value slots are an LDS table of `cap` entries, stored at the end (ways == 1) or folded into cval (split).
template <typename S, bool VALUES, int TPB, bool GLOBAL>
__global__ __launch_bounds__(TPB) void mk_row_kernel(const int *__restrict__ list, int ways, int cap, const int *__restrict__ arpt, const int *__restrict__ acol,
                                                     const double *__restrict__ aval, const int *__restrict__ brpt, const int *__restrict__ bcol,
                                                     const double *__restrict__ bval, const int *__restrict__ mrpt, const int *__restrict__ mcol, double *cval)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long *s_scan = reinterpret_cast<long long *>(smem);       // TPB + 1 (+ 1 pad)
    long long *s_wsum = s_scan + TPB + 2;                          // TPB / 64
    double *s_av = reinterpret_cast<double *>(s_wsum + TPB / 64);  // TPB
    double *t_val = s_av + TPB;                                    // cap
    int *s_start = reinterpret_cast<int *>(t_val + cap);           // TPB
    int *t_col = s_start + TPB;                                    // cap
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = list[blockIdx.x / (unsigned)ways], part = (int)(blockIdx.x % (unsigned)ways);
    const int ab = arpt[row], ae = arpt[row + 1], mb = mrpt[row], mlen = mrpt[row + 1] - mb;
    const long long first = (long long)ab + (long long)part * TPB;
    if (first >= ae) return;                                       // the same for every thread of the workgroup
    if constexpr (!GLOBAL) {
        for (int q = t; q < mlen; q += TPB) {                      // (the first tile's barrier orders this before any lookup)
            t_col[q] = mcol[mb + q];
            t_val[q] = S::identity();
        }
    }
    const int cmin = mcol[mb], cmax = mcol[mb + mlen - 1];         // mlen >= 1 in every class that runs
    for (long long a0 = first; a0 < ae; a0 += (long long)ways * TPB) {
        const long long i = a0 + t;
        int start = 0;
        long long x = 0;
        double av = 1.0;
        if (i < ae) {
            const int p = acol[i];
            start = brpt[p];
            x = brpt[p + 1] - start;
            if constexpr (VALUES) av = aval[i];
        }
        for (int o = 1; o < 64; o <<= 1) {                         // inclusive scan of the B row lengths; 64 bits: repeated columns can sum past 2^31
            const long long y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wsum[wave] = x;
        s_start[t] = start;
        if constexpr (VALUES) s_av[t] = av;
        __syncthreads();
        long long off = 0;
        for (int w = 0; w < wave; ++w) off += s_wsum[w];
        s_scan[t + 1] = off + x;
        if (t == 0) s_scan[0] = 0;
        __syncthreads();
        const long long total = s_scan[TPB];
        int lo = 0;                                                // the last entry with s_scan[lo] <= e: never decreases as e grows
        for (long long e = t; e < total; e += TPB) {
            int hi = TPB - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_scan[mid] <= e) lo = mid;
                else hi = mid - 1;
            }
            const int k = s_start[lo] + (int)(e - s_scan[lo]);
            const int j = bcol[k];
            if (j < cmin || j > cmax) continue;
            int q = 0, h = mlen;                                   // the first slot whose column is >= j
            while (q < h) {
                const int mid = (q + h) >> 1;
                int c;
                if constexpr (GLOBAL) c = mcol[mb + mid];
                else c = t_col[mid];
                if (c < j) q = mid + 1;
                else h = mid;
            }
            if (q >= mlen) continue;
            int c;
            if constexpr (GLOBAL) c = mcol[mb + q];
            else c = t_col[q];
            if (c != j) continue;
            double v;
            if constexpr (VALUES) v = S::mul(s_av[lo], bval[k]);
            else v = S::mul(1.0, 1.0);
            if constexpr (GLOBAL) S::global_acc(cval + mb + q, v);
            else S::lds_acc(t_val + q, v);
        }
        __syncthreads();
    }
    if constexpr (!GLOBAL) {
        if (ways == 1) {
            for (int q = t; q < mlen; q += TPB) cval[mb + q] = t_val[q];
        } else {
            for (int q = t; q < mlen; q += TPB) {
                const double v = t_val[q];
                if (v != S::identity()) S::global_acc(cval + mb + q, v);
            }
        }
    }
}

// ---- triangle counting: the strictly lower triangle as a CSR of its own, and the sum of the counts
__global__ __launch_bounds__(WG) void tc_lower_kernel(int n, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colids, int *__restrict__ lcnt,
                                                      OpenState *st)
{
    const int l = (int)threadIdx.x % kOpenLpr;
    const long long row = (long long)blockIdx.x * (WG / kOpenLpr) + threadIdx.x / kOpenLpr;
    int bad = 0, cnt = 0;
    if (row < n) {
        const int rb = rowptr[row], re = rowptr[row + 1];
        if (rb < 0 || re < rb || re > nnz || (row == 0 && rb != 0)) bad = 1;
        else {
            for (int k = rb + l; k < re; k += kOpenLpr) {
                const int c = colids[k];
                if ((unsigned)c >= (unsigned)n) bad = 1;
                if (k > rb && colids[k - 1] >= c) bad = 1;
                cnt += c < row;
            }
        }
    }
    for (int o = kOpenLpr / 2; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        bad |= __shfl_xor(bad, o);
    }
    if (row <= n && l == 0) lcnt[row] = row < n && !bad ? cnt : 0;  // lcnt[n] = 0: the scan's last output is the total
    if (bad) atomicOr(&st->invalid, BAD_MASK);
}

// rows ascend, so the entries below the diagonal are the first lrpt[i + 1] − lrpt[i] of row i
__global__ __launch_bounds__(WG) void tc_copy_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ colids, const int *__restrict__ lrpt,
                                                     int *__restrict__ lcol)
{
    const int l = (int)threadIdx.x % kOpenLpr;
    const long long row = (long long)blockIdx.x * (WG / kOpenLpr) + threadIdx.x / kOpenLpr;
    if (row >= n) return;
    const int rb = rowptr[row], lb = lrpt[row], cnt = lrpt[row + 1] - lb;
    for (int q = l; q < cnt; q += kOpenLpr) lcol[lb + q] = colids[rb + q];
}

// Σ cval as int64 in a fixed order: block b sums the entries b·WG + t + k·kSumBlocks·WG, one block then adds the kSumBlocks partial sums in index order.
__global__ __launch_bounds__(WG) void tc_sum_kernel(long long n, const double *__restrict__ cval, long long *__restrict__ partial)
{
    __shared__ long long s_red[WG / 64];
    long long c = 0;
    for (long long k = (long long)blockIdx.x * WG + threadIdx.x; k < n; k += (long long)gridDim.x * WG) c += (long long)cval[k];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < WG / 64; ++w) sum += s_red[w];
        partial[blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(64) void tc_sum_final_kernel(int nb, const long long *__restrict__ partial, long long *__restrict__ out)
{
    if (threadIdx.x != 0) return;
    long long sum = 0;
    for (int b = 0; b < nb; ++b) sum += partial[b];
    *out = sum;
}

// ------------------------------------------------------------------------------------------------ host side
long long env_ll(const char *name, long long dflt, long long lo, long long hi)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    return std::max(lo, std::min(hi, atoll(e)));
}

Cuts read_cuts()
{
    Cuts c;
    c.wave_flop = env_ll("G4S_MASKED_WAVE_FLOP", kWaveFlop, 0, 1ll << 30);
    c.split_flop = env_ll("G4S_MASKED_SPLIT_FLOP", kSplitFlop, 1, LLONG_MAX);
    c.lds_small = (int)env_ll("G4S_MASKED_LDS_SMALL", kLdsSmall, 0, kLdsSmall);
    c.lds_large = (int)env_ll("G4S_MASKED_LDS_LARGE", kLdsLarge, 0, kLdsLarge);
    c.split_ways = (int)env_ll("G4S_MASKED_SPLIT_WAYS", kSplitWays, 2, 4096);
    return c;
}

template <typename Kernel>
int allow_lds(Kernel k, size_t bytes)
{
    if (bytes > 64 * 1024) G4S_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return G4S_OK;
}

template <typename S, bool VALUES>
int launch_classes(const Operands &o, const int *list, const int *cnt, const Cuts &cuts, hipStream_t s)
{
    int off[C_COUNT];                                              // the list is sorted by descending class
    for (int c = C_COUNT - 1, run = 0; c >= 0; --c) { off[c] = run; run += cnt[c]; }
#define MK_ARGS o.arpt, o.acol, o.aval, o.brpt, o.bcol, o.bval, o.mrpt, o.mcol, o.cval
    if (cnt[C_WAVE])
        hipLaunchKernelGGL((mk_wave_kernel<S, VALUES>), dim3((cnt[C_WAVE] + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, s, list + off[C_WAVE], cnt[C_WAVE], MK_ARGS);
    constexpr size_t lds_s = row_kernel_lds(WG, kLdsSmall), lds_l = row_kernel_lds(kWgLarge, kLdsLarge), lds_g = row_kernel_lds(WG, 0);
    if (cnt[C_LDS_S])
        hipLaunchKernelGGL((mk_row_kernel<S, VALUES, WG, false>), dim3(cnt[C_LDS_S]), dim3(WG), lds_s, s, list + off[C_LDS_S], 1, kLdsSmall, MK_ARGS);
    if (cnt[C_LDS_L]) {
        G4S_TRY(allow_lds(mk_row_kernel<S, VALUES, kWgLarge, false>, lds_l));
        hipLaunchKernelGGL((mk_row_kernel<S, VALUES, kWgLarge, false>), dim3(cnt[C_LDS_L]), dim3(kWgLarge), lds_l, s, list + off[C_LDS_L], 1, kLdsLarge, MK_ARGS);
    }
    if (cnt[C_GLOBAL])
        hipLaunchKernelGGL((mk_row_kernel<S, VALUES, WG, true>), dim3(cnt[C_GLOBAL]), dim3(WG), lds_g, s, list + off[C_GLOBAL], 1, 0, MK_ARGS);
    const long long ways = cuts.split_ways;
    if ((long long)cnt[C_SPLIT_LDS] * ways > INT_MAX || (long long)cnt[C_SPLIT_GLOBAL] * ways > INT_MAX)
        return g4s::set_error(G4S_ERR_OVERFLOW, "g4s_spgemm_masked: %d split rows x %lld workgroups exceed the launch grid", cnt[C_SPLIT_LDS] + cnt[C_SPLIT_GLOBAL], ways);
    if (cnt[C_SPLIT_LDS])
        hipLaunchKernelGGL((mk_row_kernel<S, VALUES, WG, false>), dim3((unsigned)(cnt[C_SPLIT_LDS] * ways)), dim3(WG), lds_s, s, list + off[C_SPLIT_LDS], (int)ways,
                           kLdsSmall, MK_ARGS);
    if (cnt[C_SPLIT_GLOBAL])
        hipLaunchKernelGGL((mk_row_kernel<S, VALUES, WG, true>), dim3((unsigned)(cnt[C_SPLIT_GLOBAL] * ways)), dim3(WG), lds_g, s, list + off[C_SPLIT_GLOBAL], (int)ways,
                           0, MK_ARGS);
#undef MK_ARGS
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

// Everything on device arrays; returns with the stream synchronised (on success and on G4S_ERR_INVALID alike). The caller has ruled out a capture.
int masked_device(const Operands &o, unsigned flags, g4s_masked_info *info, hipStream_t s)
{
    if (info) *info = g4s_masked_info{};
    if (o.M == 0) return G4S_OK;
    g4s::ReadScope reads(s);
    int annz = 0, bnnz = 0, mnnz = 0;
    G4S_HIP_TRY(reads.note(annz, o.arpt + o.M));
    G4S_HIP_TRY(reads.note(mnnz, o.mrpt + o.M));
    if (o.K > 0) G4S_HIP_TRY(reads.note(bnnz, o.brpt + o.K));
    G4S_HIP_TRY(reads.wait());
    if (annz < 0 || bnnz < 0 || mnnz < 0) return g4s::set_error(G4S_ERR_INVALID, "g4s_spgemm_masked: a negative entry count (arpt[M] %d, brpt[K] %d, mrpt[M] %d)", annz, bnnz, mnnz);
    if (info) info->mask_nnz = mnnz;
    if (mnnz == 0) return G4S_OK;
    const size_t cb = sizeof(double) * (size_t)mnnz;
    if (overlap(o.cval, cb, o.arpt, 4 * ((size_t)o.M + 1)) || overlap(o.cval, cb, o.acol, 4 * (size_t)annz) || overlap(o.cval, cb, o.aval, o.aval ? 8 * (size_t)annz : 0) ||
        overlap(o.cval, cb, o.brpt, 4 * ((size_t)o.K + 1)) || overlap(o.cval, cb, o.bcol, 4 * (size_t)bnnz) || overlap(o.cval, cb, o.bval, o.bval ? 8 * (size_t)bnnz : 0) ||
        overlap(o.cval, cb, o.mrpt, 4 * ((size_t)o.M + 1)) || overlap(o.cval, cb, o.mcol, 4 * (size_t)mnnz))
        return g4s::set_error(G4S_ERR_INVALID, "g4s_spgemm_masked: cval overlaps an input array");

    const Cuts cuts = read_cuts();
    const size_t m4 = sizeof(int) * (size_t)o.M;
    OpenState *st;
    int *keys, *ids, *keys_s, *list;                               // four int arrays of M: keys, row ids, and both sorted
    Carver work;
    work.piece(&st, sizeof(OpenState));
    work.piece(&keys, m4);
    work.piece(&ids, m4);
    work.piece(&keys_s, m4);
    work.piece(&list, m4);
    G4S_TRY(work.alloc());
    OpenState h{};
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(OpenState), s));
    const unsigned ring = flags & G4S_SEMIRING_MASK;               // S::identity() on the host
    const double identity = ring == G4S_SEMIRING_MIN_PLUS ? __builtin_inf() : ring == G4S_SEMIRING_MAX_PLUS ? -__builtin_inf() : 0.0;
    hipLaunchKernelGGL(mk_fill_kernel, dim3(grid_for<WG>(mnnz, 8192)), dim3(WG), 0, s, (long long)mnnz, identity, o.cval);
    if (bnnz) hipLaunchKernelGGL(mk_check_b_kernel, dim3(grid_for<WG>(bnnz, 8192)), dim3(WG), 0, s, (long long)bnnz, o.N, o.bcol, st);
    const int rows_per_wg = WG / kOpenLpr;
    hipLaunchKernelGGL(mk_open_kernel, dim3((o.M + rows_per_wg - 1) / rows_per_wg), dim3(WG), 0, s, o.M, o.K, o.N, annz, bnnz, mnnz, o.arpt, o.acol, o.brpt, o.mrpt,
                       o.mcol, keys, ids, st, cuts);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(reads.note(h, st));
    G4S_TRY(g4s::prims::sort_pairs_descending(keys, ids, keys_s, list, keys_s, list, o.M, 3, s));   // one pass: the partners are never written
    G4S_HIP_TRY(reads.wait());
    if (h.invalid) work.idle();                                    // refused: the wait has left the stream idle. (Any other early return leaves it
    if (h.invalid & BAD_MASK)                                      // out, and the block is released behind a device-wide wait.)
        return g4s::set_error(G4S_ERR_INVALID, "g4s_spgemm_masked: the mask is not a CSR pattern with strictly ascending rows and column ids in [0, %d)", o.N);
    if (h.invalid) return g4s::set_error(G4S_ERR_INVALID, "g4s_spgemm_masked: %s", (h.invalid & BAD_A) ? "a row pointer or column id of A is out of range"
                                                                                                      : "a row pointer or column id of B is out of range");
    if (getenv("G4S_DEBUG"))
        fprintf(stderr, "g4s masked classes: skip %d wave %d lds_small %d lds_large %d global %d split_lds %d split_global %d (products %llu)\n", h.counts[C_SKIP],
                h.counts[C_WAVE], h.counts[C_LDS_S], h.counts[C_LDS_L], h.counts[C_GLOBAL], h.counts[C_SPLIT_LDS], h.counts[C_SPLIT_GLOBAL], h.products);
    if (h.counts[C_SKIP] < o.M) {
        G4S_TRY(sr::dispatch(flags, [&](auto p) {
            return o.aval ? launch_classes<decltype(p), true>(o, list, h.counts, cuts, s) : launch_classes<decltype(p), false>(o, list, h.counts, cuts, s);
        }));
    }
    G4S_HIP_TRY(hipStreamSynchronize(s));
    work.idle();
    if (info) {
        info->products = (int64_t)h.products;
        info->rows_wave = h.counts[C_WAVE];
        info->rows_lds = h.counts[C_LDS_S] + h.counts[C_LDS_L] + h.counts[C_SPLIT_LDS];
        info->rows_global = h.counts[C_GLOBAL] + h.counts[C_SPLIT_GLOBAL];
        info->rows_split = h.counts[C_SPLIT_LDS] + h.counts[C_SPLIT_GLOBAL];
    }
    return G4S_OK;
}

// The triangles of the strictly lower triangle L of an n × n pattern on the device: L compacted, Σ (L·L⟨L⟩) in int64.
int triangles_device(int n, int nnz, const int *rowptr, const int *colids, int64_t *triangles, g4s_masked_info *info, hipStream_t s)
{
    BigBuf lcol, cval;
    const size_t n4 = sizeof(int) * ((size_t)n + 1);
    OpenState *st;
    int *lcnt, *lrpt;
    long long *partial;
    Carver small;
    small.piece(&st, sizeof(OpenState));
    small.piece(&lcnt, n4);
    small.piece(&lrpt, n4);
    small.tail(&partial, sizeof(long long) * (kSumBlocks + 1));
    G4S_TRY(small.alloc());
    g4s::ReadScope reads(s);
    int invalid = 0, lnnz = 0;
    long long total = 0;
    const int rows_per_wg = WG / kOpenLpr;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(OpenState), s));
    hipLaunchKernelGGL(tc_lower_kernel, dim3(n / rows_per_wg + 1), dim3(WG), 0, s, n, nnz, rowptr, colids, lcnt, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(lcnt), lrpt, (long long)n + 1, s));
    G4S_HIP_TRY(reads.note(invalid, &st->invalid));
    G4S_HIP_TRY(reads.fetch(lnnz, lrpt + n));
    if (invalid || lnnz == 0) small.idle();                        // nothing more is enqueued, and the wait has left the stream idle (see masked_device)
    if (invalid) return g4s::set_error(G4S_ERR_INVALID, "g4s_triangle_count: rows must be strictly ascending with column ids in [0, %d) and rowptr non-decreasing from 0", n);
    if (lnnz > 0) {
        G4S_TRY(lcol.alloc(sizeof(int) * (size_t)lnnz));
        G4S_TRY(cval.alloc(sizeof(double) * (size_t)lnnz));
        hipLaunchKernelGGL(tc_copy_kernel, dim3(n / rows_per_wg + 1), dim3(WG), 0, s, n, rowptr, colids, lrpt, lcol.as<int>());
        G4S_HIP_TRY(hipGetLastError());
        const Operands o{n, n, n, lrpt, lcol.as<int>(), nullptr, lrpt, lcol.as<int>(), nullptr, lrpt, lcol.as<int>(), cval.as<double>()};
        G4S_TRY(masked_device(o, G4S_SEMIRING_PLUS_TIMES, info, s));
        hipLaunchKernelGGL(tc_sum_kernel, dim3(kSumBlocks), dim3(WG), 0, s, (long long)lnnz, cval.as<double>(), partial);
        hipLaunchKernelGGL(tc_sum_final_kernel, dim3(1), dim3(64), 0, s, kSumBlocks, partial, partial + kSumBlocks);
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(reads.fetch(total, partial + kSumBlocks));
        small.idle();
        lcol.idle = cval.idle = true;
    }
    *triangles = total;
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_spgemm_masked(int32_t M, int32_t K, int32_t N, const int32_t *arpt, const int32_t *acol, const double *aval, const int32_t *brpt,
                                     const int32_t *bcol, const double *bval, const int32_t *mrpt, const int32_t *mcol, double *cval, unsigned flags,
                                     g4s_masked_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~(G4S_DEVICE_POINTERS | G4S_SEMIRING_MASK)) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and one G4S_SEMIRING_* value");
    G4S_REQUIRE(M >= 0 && K >= 0 && N >= 0, "negative dimension");
    G4S_REQUIRE(arpt && acol && brpt && bcol, "a NULL index array of A or B");
    G4S_REQUIRE(mrpt && cval, "mrpt or cval is NULL");
    G4S_REQUIRE(mcol || M == 0, "mcol is NULL");
    G4S_REQUIRE((aval == nullptr) == (bval == nullptr), "aval and bval must both be given or both be NULL (pattern-only)");
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s));
    if (flags & G4S_DEVICE_POINTERS) {
        const Operands o{M, K, N, arpt, acol, aval, brpt, bcol, bval, mrpt, mcol, cval};
        return masked_device(o, flags, info, s);
    }
    // host arrays: device copies of the inputs, the same steps, cval copied back
    if (info) *info = g4s_masked_info{};
    if (M == 0) return G4S_OK;
    const int annz = arpt[M], bnnz = K ? brpt[K] : 0, mnnz = mrpt[M];
    G4S_REQUIRE(annz >= 0 && bnnz >= 0 && mnnz >= 0, "a negative entry count");
    Staged stage(s);
    const Operands o{M, K, N, stage.in(arpt, sizeof(int) * ((size_t)M + 1)), stage.in(acol, sizeof(int) * (size_t)annz), stage.in(aval, sizeof(double) * (size_t)annz),
                     stage.in(brpt, sizeof(int) * ((size_t)K + 1)), stage.in(bcol, sizeof(int) * (size_t)bnnz), stage.in(bval, sizeof(double) * (size_t)bnnz),
                     stage.in(mrpt, sizeof(int) * ((size_t)M + 1)), stage.in(mcol, sizeof(int) * (size_t)mnnz), stage.out<double>(sizeof(double) * (size_t)mnnz)};
    int status = stage.error();
    if (status == G4S_OK) status = masked_device(o, flags, info, s);
    if (status == G4S_OK) status = stage.to_host(cval, o.cval, sizeof(double) * (size_t)mnnz);
    if (status == G4S_OK) status = stage.wait();
    return stage.finish(status);
}

G4S_API g4s_status g4s_triangle_count(int32_t n, const int32_t *rowptr, const int32_t *colids, int64_t *triangles, unsigned flags, g4s_masked_info *info,
                                      void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr && triangles, "rowptr or triangles is NULL");
    G4S_REQUIRE(colids || n == 0, "colids is NULL");
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s));
    *triangles = 0;
    if (info) *info = g4s_masked_info{};
    if (n == 0) return G4S_OK;
    if (flags & G4S_DEVICE_POINTERS) {
        int nnz = 0;
        G4S_HIP_TRY(g4s::ReadScope(s).fetch(nnz, rowptr + n));
        G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
        return triangles_device(n, nnz, rowptr, colids, triangles, info, s);
    }
    const int nnz = rowptr[n];
    G4S_REQUIRE(nnz >= 0, "rowptr[n] is negative");
    Staged stage(s);
    const int *d_rp = stage.in(rowptr, sizeof(int) * ((size_t)n + 1)), *d_ci = stage.in(colids, sizeof(int) * (size_t)nnz);
    int status = stage.error();
    if (status == G4S_OK) status = triangles_device(n, nnz, d_rp, d_ci, triangles, info, s);
    return stage.finish(status);
}
