// pagerank.hip — g4s_pagerank (include/g4s.h): PageRank by power iteration on a CSR handle stored by out-edges, the loop on the device.
//
// One iteration is three launches and nothing is read back in between:
//   product   y := Aᵀ·x through the inner handle of Aᵀ (or A itself under G4S_PAGERANK_SYMMETRIC), on whichever of the four SpMV paths that handle took;
//   epilogue  one grid-stride kernel: r'_v = damping·(y_v + m·p_v) + (1 − damping)·p_v, written over r, the next x_v = r'_v · (1 / s_v), and per
//             workgroup two partial sums: |r' − r| and the r' of the dangling vertices. Its grid is a function of n only;
//   verdict   one workgroup behind the kernel boundary: both partial lists summed in INDEX ORDER (lanes 0 and 1 of the first wave, out of LDS), the
//             residual, the dangling mass m of the next iteration, iter += 1 and `stop` — 1 residual < tol, 2 cap (PrState, pagerank.hpp).
// An epilogue or verdict that finds stop != 0 returns at once, so the host enqueues batches of at least G4S_PAGERANK_BATCH iterations blind, reads the
// 64-byte state once per batch and sizes the next batch from the geometric decay of the last two residuals, as g4s_conj_grad does. Iterations behind
// the stop cost their product and change nothing. The verdict is a kernel of its own rather than the last-ticket workgroup of the epilogue: a kernel
// boundary is the one ordering that needs no argument about what a plain load may see across the XCDs' L2s, the partials are then read
// by ordinary loads, and the price is one launch of a few microseconds per iteration (DESIGN §4.9 has the measurement).
// With a fixed grid and a fixed order of every sum, the residual and the dangling mass are the same bits on every run; the ranks are too wherever the
// product is (paths 0, 3, 4 — the blocked path sums through LDS atomics).
//
// The strength pass (once per reserve and after g4s_csr_update_values) computes s_u = Σ_v a_uv on the forward CSR, 1 / s_u (0 for a dangling u), the
// number of dangling vertices, and validates the values (finite, >= 0): 4, 16 or 64 lanes per row by the average degree, and rows above kLongRow
// entries by a whole workgroup each (strength_long_kernel), so a hub is never one lane's loop. Personalization and warm start are summed and
// validated by the same partial-sum / ordered-sum pair; an invalid input raises stop = 3 on the device and is reported after the first batch's read.
#include "common.hpp"
#include "csr_handle.hpp"
#include "pagerank.hpp"
#include "call_util.hpp"
#include "readback.hpp"
#include "step_batch.hpp"
#include "wave_reduce.hpp"
#include <algorithm>
#include <cmath>
#include <new>

namespace {

using g4s::PrState;

constexpr int kItems = 8;          // entries per thread the epilogue's grid is sized for
constexpr int kMaxGrid = 512;      // workgroups of the epilogue at most: the verdict sums that many partials in order
constexpr int kLongRow = 4096;     // a row with more entries is summed by a whole workgroup
constexpr int kBatch = G4S_PAGERANK_BATCH;
enum { P_RES = 0, P_MASS = 1, P_SUMP = 2, P_SUMR = 3, P_LISTS = 4 };   // the lists of per-workgroup partials, kMaxGrid doubles each

static_assert(sizeof(PrState) == 64, "the host reads PrState as one small block");

inline int epilogue_grid(int n) { return (int)std::max(1LL, std::min(((long long)n + WG * kItems - 1) / (WG * kItems), (long long)kMaxGrid)); }

// The workgroup's sum, in a fixed order: a shuffle tree per wave, then the waves in index order. Every thread gets it.
__device__ __forceinline__ double block_sum(double v, double *s_red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < WG / 64; ++w) s += s_red[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int bad_entry(double a) { return !(a >= 0.0) | !(a < __builtin_inf()); }   // negative, NaN or infinite

// Lists j = 0, 1 of `lists` (G partials each) summed in index order by lanes 0 and 1 of the first wave; the workgroup stages them in LDS, padded
// with zeros to a multiple of 8 so that the chain of additions waits for one LDS read in eight. out[j] is valid for every thread afterwards.
__device__ __forceinline__ void ordered_sums(int G, const double *__restrict__ list0, const double *__restrict__ list1, double *out)
{
    __shared__ double s_part[2][kMaxGrid];
    const int t = (int)threadIdx.x, Gp = (G + 7) & ~7;
    for (int i = t; i < Gp; i += WG) {
        s_part[0][i] = (i < G && list0) ? list0[i] : 0.0;
        s_part[1][i] = (i < G && list1) ? list1[i] : 0.0;
    }
    __syncthreads();
    if (t < 2) {
        double s = 0.0;
        for (int i = 0; i < Gp; i += 8) {
            double a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = s_part[t][i + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += a[j];
        }
        out[t] = s;
    }
    __syncthreads();
}

// One thread: the state of a call from zero. reset_strength: the strength pass runs behind this kernel.
__global__ void begin_kernel(PrState *st, int reset_strength)
{
    if (reset_strength) { st->dangling = 0; st->bad_values = 0; }
    st->residual = 0.0; st->prev_residual = 0.0; st->mass = 0.0; st->sum_p = 0.0; st->sum_r = 0.0;
    st->iter = 0; st->stop = 0; st->bad_vec = 0;
}

__device__ __forceinline__ void strength_store(long long u, double s, double *__restrict__ inv_s, int &bad, long long &dang)
{
    bad |= !(s < __builtin_inf());                                 // a sum that overflowed (or NaN)
    const bool positive = s > 0.0;
    inv_s[u] = positive ? 1.0 / s : 0.0;
    dang += !positive;
}

__device__ __forceinline__ void strength_finish(int bad, long long dang, PrState *st)
{
    dang = wave_sum(dang);
    if ((threadIdx.x & 63) == 0 && dang) atomicAdd((unsigned long long *)&st->dangling, (unsigned long long)dang);
    if (bad) atomicOr(&st->bad_values, 1);
}

// Rows of at most kLongRow entries: LPR lanes per row, the lanes' sums combined by a butterfly (the same order on every run).
template <int LPR>
__global__ __launch_bounds__(WG) void strength_kernel(int n, const int *__restrict__ rowptr, const double *__restrict__ values, double *__restrict__ inv_s, PrState *st)
{
    constexpr int GPB = WG / LPR;
    const int t = (int)threadIdx.x, lig = t % LPR;
    int bad = 0;
    long long dang = 0;
    for (long long r0 = (long long)blockIdx.x * GPB; r0 < n; r0 += (long long)gridDim.x * GPB) {
        const long long u = r0 + t / LPR;
        double s = 0.0;
        bool mine = false;
        if (u < n) {
            const int b = rowptr[u], e = rowptr[u + 1];
            if (e - b <= kLongRow) {
                mine = true;
                for (int k = b + lig; k < e; k += LPR) {
                    const double a = values[k];
                    bad |= bad_entry(a);
                    s += a;
                }
            }
        }
        if constexpr (LPR > 1) {
            for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        }
        if (mine && lig == 0) strength_store(u, s, inv_s, bad, dang);
    }
    strength_finish(bad, dang, st);
}

// Rows above kLongRow entries: a workgroup looks at 256 rows, and walks each long one among them with all its threads.
__global__ __launch_bounds__(WG) void strength_long_kernel(int n, const int *__restrict__ rowptr, const double *__restrict__ values, double *__restrict__ inv_s, PrState *st)
{
    __shared__ unsigned long long s_mask[WG / 64];
    __shared__ double s_red[WG / 64];
    const int t = (int)threadIdx.x;
    int bad = 0;
    long long dang = 0;
    for (long long base = (long long)blockIdx.x * WG; base < n; base += (long long)gridDim.x * WG) {
        const long long u = base + t;
        const bool is_long = u < n && rowptr[u + 1] - rowptr[u] > kLongRow;
        const unsigned long long m = __ballot(is_long);
        if ((t & 63) == 0) s_mask[t >> 6] = m;
        __syncthreads();
        for (int w = 0; w < WG / 64; ++w) {
            unsigned long long mm = s_mask[w];                     // the same word for every thread: the loop below is uniform
            while (mm) {
                const long long v = base + w * 64 + (__ffsll((long long)mm) - 1);
                mm &= mm - 1;
                const int b = rowptr[v], e = rowptr[v + 1];
                double s = 0.0;
                for (int k = b + t; k < e; k += WG) {
                    const double a = values[k];
                    bad |= bad_entry(a);
                    s += a;
                }
                s = block_sum(s, s_red);
                if (t == 0) strength_store(v, s, inv_s, bad, dang);
            }
        }
        __syncthreads();
    }
    strength_finish(bad, dang, st);
}

// Σ v per workgroup into `partials`, and `bit` into bad_vec when an entry is negative or not finite.
__global__ __launch_bounds__(WG) void vec_sum_kernel(int n, const double *__restrict__ v, double *__restrict__ partials, PrState *st, int bit)
{
    __shared__ double s_red[WG / 64];
    double s = 0.0;
    int bad = 0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        const double a = v[i];
        bad |= bad_entry(a);
        s += a;
    }
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
    if (bad) atomicOr(&st->bad_vec, bit);
}

// One workgroup: Σ personalization and Σ start in index order; a sum outside (0, inf) is invalid too.
__global__ __launch_bounds__(WG) void sums_verdict_kernel(int G, const double *__restrict__ part_p, const double *__restrict__ part_r, PrState *st)
{
    __shared__ double s_out[2];
    ordered_sums(G, part_p, part_r, s_out);
    if (threadIdx.x != 0) return;
    int bad = 0;
    if (part_p) { st->sum_p = s_out[0]; bad |= (!(s_out[0] > 0.0) || !(s_out[0] < __builtin_inf())) ? 1 : 0; }
    if (part_r) { st->sum_r = s_out[1]; bad |= (!(s_out[1] > 0.0) || !(s_out[1] < __builtin_inf())) ? 2 : 0; }
    if (bad) st->bad_vec |= bad;
}

// p := personalization / Σ (kept in pn), r_0 := p or rank / Σ rank, x_0 := r_0 · (1 / s), and the dangling mass of r_0 per workgroup.
template <bool PERS>
__global__ __launch_bounds__(WG) void init_kernel(int n, const double *__restrict__ pers, double inv_n, int warm, const double *__restrict__ inv_s, double *__restrict__ pn,
                                                  double *__restrict__ rank, double *__restrict__ x, double *__restrict__ partials, const PrState *st)
{
    __shared__ double s_red[WG / 64];
    if (st->bad_values | st->bad_vec) return;                      // nothing is divided by a sum that is not positive; the verdict raises stop = 3
    const double sum_p = st->sum_p, sum_r = st->sum_r;
    double mass = 0.0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        double pv = inv_n;
        if constexpr (PERS) { pv = pers[i] / sum_p; pn[i] = pv; }
        const double r = warm ? rank[i] / sum_r : pv;
        const double is = inv_s[i];
        rank[i] = r;
        x[i] = r * is;
        if (is == 0.0) mass += r;
    }
    mass = block_sum(mass, s_red);
    if (threadIdx.x == 0) partials[P_MASS * kMaxGrid + blockIdx.x] = mass;
}

template <bool PERS>
__global__ __launch_bounds__(WG) void epilogue_kernel(int n, double damping, double one_minus_damping, double inv_n, const double *__restrict__ y, const double *__restrict__ pn,
                                                      const double *__restrict__ inv_s, double *__restrict__ rank, double *__restrict__ x, double *__restrict__ partials,
                                                      const PrState *st)
{
    __shared__ double s_red[WG / 64];
    if (st->stop != 0) return;                                     // the same word for every workgroup: only a verdict kernel writes it
    const double m = st->mass;
    double res = 0.0, mass = 0.0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) {
        double pv = inv_n;
        if constexpr (PERS) pv = pn[i];
        const double rv = rank[i], is = inv_s[i];
        const double rn = damping * (y[i] + m * pv) + one_minus_damping * pv;
        res += fabs(rn - rv);
        rank[i] = rn;
        x[i] = rn * is;
        if (is == 0.0) mass += rn;
    }
    res = block_sum(res, s_red);
    mass = block_sum(mass, s_red);
    if (threadIdx.x == 0) {
        partials[P_RES * kMaxGrid + blockIdx.x] = res;
        partials[P_MASS * kMaxGrid + blockIdx.x] = mass;
    }
}

// One workgroup behind the epilogue (INIT: behind init_kernel): the partials in index order, the counters and the stop word.
template <bool INIT>
__global__ __launch_bounds__(WG) void verdict_kernel(int G, const double *__restrict__ partials, double tol, int cap, PrState *st)
{
    __shared__ double s_out[2];
    if (!INIT && st->stop != 0) return;
    if (INIT && (st->bad_values | st->bad_vec)) {
        if (threadIdx.x == 0) st->stop = 3;
        return;
    }
    ordered_sums(G, INIT ? nullptr : partials + P_RES * kMaxGrid, partials + P_MASS * kMaxGrid, s_out);
    if (threadIdx.x != 0) return;
    st->mass = s_out[1];
    if (INIT) return;
    const double res = s_out[0];
    const int iter = st->iter + 1;
    st->prev_residual = st->residual;
    st->residual = res;
    st->iter = iter;
    st->stop = res < tol ? 1 : (iter >= cap ? 2 : 0);
}

} // namespace

// ------------------------------------------------------------------------------------------------ the handle's workspace
namespace g4s {

struct PagerankWork {
    double *vec = nullptr;        // inv_s | x | y | pn, n doubles each
    double *partials = nullptr;   // P_LISTS lists of kMaxGrid
    PrState *state = nullptr;
    bool values_dirty = true;     // the strength pass has to run (again)
    int64_t n = 0;
    DevicePieces mem;             // owns the arrays above
};

void pagerank_work_destroy(PagerankWork *w) { delete w; }
long long pagerank_work_bytes(const PagerankWork *w) { return w ? w->mem.bytes : 0; }
void pagerank_values_changed(PagerankWork *w) { if (w) w->values_dirty = true; }

} // namespace g4s

namespace {

constexpr unsigned kAllFlags = G4S_PAGERANK_SYMMETRIC | G4S_PAGERANK_WARM_START;

// The workspace (once) and, unless the caller declares A symmetric or A has no entry, the handle's transpose. Allocates; enqueues nothing.
int reserve(g4s_csr_s *A, unsigned flags)
{
    if (!A->prk) {
        std::unique_ptr<g4s::PagerankWork> w(new (std::nothrow) g4s::PagerankWork());
        if (!w) return g4s::set_error(G4S_ERR_NOMEM, "host allocation failed");
        const size_t n = (size_t)std::max(A->rows, 1);
        w->mem.take(&w->vec, sizeof(double) * 4 * n);
        w->mem.take(&w->partials, sizeof(double) * P_LISTS * kMaxGrid);
        w->mem.take(&w->state, sizeof(PrState));
        if (!w->mem.ok()) return w->mem.report("g4s_csr_pagerank_reserve");
        w->n = (int64_t)n;
        A->prk = w.release();
    }
    if (!(flags & G4S_PAGERANK_SYMMETRIC) && A->nnz > 0 && !A->tr) G4S_TRY(g4s_csr_transpose_reserve(A));
    return G4S_OK;
}

// begin_kernel and, when the values are new, the strength pass, on `s`.
int enqueue_begin(g4s_csr_s *A, hipStream_t s)
{
    g4s::PagerankWork *w = A->prk;
    const int n = A->rows;
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(1), 0, s, w->state, w->values_dirty ? 1 : 0);
    if (w->values_dirty) {
        double *inv_s = w->vec;
        const long long avg = n ? A->nnz / n : 0;
        const int lpr = avg <= 4 ? 4 : avg <= 16 ? 16 : 64;
        const int g = (int)std::max(1LL, std::min(((long long)n * lpr + WG - 1) / WG, 8LL * w->mem.cus));
        if (lpr == 4) hipLaunchKernelGGL(strength_kernel<4>, dim3(g), dim3(WG), 0, s, n, A->d_rowptr, A->d_values, inv_s, w->state);
        else if (lpr == 16) hipLaunchKernelGGL(strength_kernel<16>, dim3(g), dim3(WG), 0, s, n, A->d_rowptr, A->d_values, inv_s, w->state);
        else hipLaunchKernelGGL(strength_kernel<64>, dim3(g), dim3(WG), 0, s, n, A->d_rowptr, A->d_values, inv_s, w->state);
        const int gl = (int)std::max(1LL, std::min(((long long)n + WG - 1) / WG, 4LL * w->mem.cus));
        hipLaunchKernelGGL(strength_long_kernel, dim3(gl), dim3(WG), 0, s, n, A->d_rowptr, A->d_values, inv_s, w->state);
    }
    G4S_HIP_TRY(hipGetLastError());
    w->values_dirty = false;
    return G4S_OK;
}

// The iterations to enqueue behind a read of `h`: what the geometric decay of the last two residuals says is left, at least kBatch.
int next_batch(const PrState &h, double tol)
{
    if (!(tol > 0.0)) return g4s::kBatchMax;
    if (!(h.residual > 0.0) || !(h.prev_residual > h.residual)) return kBatch;
    const double left = std::ceil(std::log(tol / h.residual) / std::log(h.residual / h.prev_residual));
    if (!(left >= (double)kBatch)) return kBatch;
    return left > (double)g4s::kBatchMax ? g4s::kBatchMax : (int)left;
}

int pagerank(g4s_csr_s *A, double damping, double tol, int32_t max_iterations, const double *pers, double *rank, unsigned flags, g4s_pagerank_info *info,
             hipStream_t s)
{
    const char *fn = "g4s_pagerank";
    if (A->rows != A->cols) return g4s::set_error(G4S_ERR_INVALID, "%s: the handle is %d x %d, PageRank needs a square matrix", fn, A->rows, A->cols);
    G4S_TRY(not_capturing(fn, s, "its state"));
    if (info) *info = g4s_pagerank_info{};
    const int n = A->rows;
    if (n == 0) {
        if (info) info->converged = 1;
        return G4S_OK;
    }
    const bool symmetric = (flags & G4S_PAGERANK_SYMMETRIC) != 0, warm = (flags & G4S_PAGERANK_WARM_START) != 0;
    if (!A->prk || (!symmetric && A->nnz > 0 && !A->tr)) G4S_TRY(reserve(A, flags));
    g4s::PagerankWork *w = A->prk;
    g4s_csr_t product_handle = A;
    if (!symmetric && A->nnz > 0) {
        const int32_t *trp, *tci;
        const double *tva;
        g4s::transpose_work_view(A->tr, &trp, &tci, &tva, &product_handle);
    }
    const int cap = max_iterations > 0 ? max_iterations : 100;
    const int G = epilogue_grid(n);
    const double inv_n = 1.0 / (double)n, one_minus_damping = 1.0 - damping;
    double *inv_s = w->vec, *x = w->vec + w->n, *y = w->vec + 2 * w->n, *pn = w->vec + 3 * w->n, *part = w->partials;
    PrState *st = w->state;

    G4S_TRY(enqueue_begin(A, s));
    if (pers) hipLaunchKernelGGL(vec_sum_kernel, dim3(G), dim3(WG), 0, s, n, pers, part + P_SUMP * kMaxGrid, st, 1);
    if (warm) hipLaunchKernelGGL(vec_sum_kernel, dim3(G), dim3(WG), 0, s, n, (const double *)rank, part + P_SUMR * kMaxGrid, st, 2);
    if (pers || warm)
        hipLaunchKernelGGL(sums_verdict_kernel, dim3(1), dim3(WG), 0, s, G, pers ? part + P_SUMP * kMaxGrid : (const double *)nullptr,
                           warm ? part + P_SUMR * kMaxGrid : (const double *)nullptr, st);
    if (pers) hipLaunchKernelGGL(init_kernel<true>, dim3(G), dim3(WG), 0, s, n, pers, inv_n, (int)warm, (const double *)inv_s, pn, rank, x, part, (const PrState *)st);
    else hipLaunchKernelGGL(init_kernel<false>, dim3(G), dim3(WG), 0, s, n, pers, inv_n, (int)warm, (const double *)inv_s, pn, rank, x, part, (const PrState *)st);
    hipLaunchKernelGGL(verdict_kernel<true>, dim3(1), dim3(WG), 0, s, G, (const double *)part, tol, cap, st);
    G4S_HIP_TRY(hipGetLastError());
    if (A->nnz == 0) G4S_HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * (size_t)n, s));   // Aᵀ·x of a matrix without entries, once

    g4s::ReadScope reads(s);
    PrState h{};
    int waits = 0, products = 0, batch = kBatch;
    for (;;) {
        const int nb = std::min(batch, cap - h.iter);              // every iteration enqueued so far has run: stop == 0
        for (int b = 0; b < nb; ++b) {
            if (A->nnz > 0) {
                G4S_TRY(g4s_spmv(product_handle, x, y, 1.0, 0.0, s));
                ++products;
            }
            if (pers) hipLaunchKernelGGL(epilogue_kernel<true>, dim3(G), dim3(WG), 0, s, n, damping, one_minus_damping, inv_n, (const double *)y, (const double *)pn,
                                         (const double *)inv_s, rank, x, part, (const PrState *)st);
            else hipLaunchKernelGGL(epilogue_kernel<false>, dim3(G), dim3(WG), 0, s, n, damping, one_minus_damping, inv_n, (const double *)y, (const double *)pn,
                                    (const double *)inv_s, rank, x, part, (const PrState *)st);
            hipLaunchKernelGGL(verdict_kernel<false>, dim3(1), dim3(WG), 0, s, G, (const double *)part, tol, cap, st);
        }
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(reads.fetch(h, st));
        ++waits;
        if (h.stop != 0) break;
        batch = next_batch(h, tol);
    }
    if (h.stop == 3) {
        if (h.bad_values) {
            w->values_dirty = true;                                // new values get a new verdict
            return g4s::set_error(G4S_ERR_INVALID, "%s: a stored value is negative or not finite (or a row sum overflows)", fn);
        }
        return g4s::set_error(G4S_ERR_INVALID, "%s: %s must be finite and >= 0 with a sum in (0, inf)", fn, (h.bad_vec & 1) ? "personalization" : "the starting vector");
    }
    if (info) {
        info->iterations = h.iter;
        info->converged = h.stop == 1;
        info->host_waits = waits;
        info->products = products;
        info->dangling = h.dangling;
        info->residual = h.residual;
    }
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_csr_pagerank_reserve(g4s_csr_t A, unsigned flags)
{
    G4S_REQUIRE((flags & ~kAllFlags) == 0u, "flags other than G4S_PAGERANK_SYMMETRIC / _WARM_START");
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(A->rows == A->cols, "PageRank needs a square matrix");
    G4S_HIP_TRY(hipDeviceSynchronize());
    G4S_TRY(reserve(A, flags));
    if (A->rows > 0 && A->prk->values_dirty) {                     // the strength pass, now: a call then only iterates
        G4S_TRY(enqueue_begin(A, nullptr));
        G4S_HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return G4S_OK;
}

G4S_API g4s_status g4s_pagerank(g4s_csr_t A, double damping, double tol, int32_t max_iterations, const double *personalization_dev, double *rank_dev,
                                unsigned flags, g4s_pagerank_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~kAllFlags) == 0u, "flags other than G4S_PAGERANK_SYMMETRIC / _WARM_START");
    G4S_REQUIRE(A, "NULL handle");
    G4S_REQUIRE(rank_dev, "rank_dev is NULL");
    G4S_REQUIRE(damping >= 0.0 && damping < 1.0, "damping outside [0, 1)");
    G4S_REQUIRE(tol >= 0.0, "tol is negative or NaN");
    G4S_REQUIRE(max_iterations >= 0, "negative iteration cap");
    return pagerank(A, damping, tol, max_iterations, personalization_dev, rank_dev, flags, info, g4s::as_stream(stream));
}
