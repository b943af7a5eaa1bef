// ilu.hip — g4s_ilu0_* (include/g4s.h): the ILU(0) factorisation of an n × n CSR with canonical rows on the pattern of A itself, level-scheduled, and
// its apply z = U⁻¹ (L⁻¹ r). DESIGN §4.21.
//
// The dependency DAG of the row-wise factorisation — row i waits for every k < i with a stored (i, k) — is the DAG of the strictly lower triangle, the
// one g4s_sptrsv_analyse peels. So the handle is two solve plans made through the public entry points (lower with a unit diagonal, upper) on the
// handle's own (rowptr, colids, f), and the factorisation runs on the lower plan's (level, row) schedule and launch list (trsv_schedule, trsv.hpp):
//   check    ilu_open_rows_kernel: rowptr[0] == 0, non-decreasing; one read of the state. ilu_open_ids_kernel, one wave per row: ids in [0, n),
//            strictly ascending, the diagonal stored, its position to dpos; one read of the state. A refusal ends at either read.
//   factor   per launch of the lower plan ilu_level_kernel (one wide level) or ilu_chain_kernel (one workgroup, a run of narrow levels, a fence and a
//            barrier behind each); then g4s_sptrsv_update_values on both plans.
//   apply    g4s_sptrsv_solve on the lower plan (r → z), then on the upper plan (z → z); for a block of k vectors g4s_sptrsv_solve_multi, likewise.
// The frame — the launch walk, the deal of a tile's rows, the levels of a chain — is the solve's (level_schedule.hpp, level_tile.hpp), and so is the
// memory model of the finished values of earlier rows (ld_prior<kChain>, for_chain_levels). A row's own working values w are shared
// between the lanes that update them inside one kernel, so they live in registers (one lane's row), in LDS (one wave's row, behind a wave barrier per
// step) or — the workgroup's row — in f itself, where every read of them is an agent-scope load (ld_prior<true>, whatever the kernel) behind
// __threadfence() and __syncthreads(). No row reads a value of another row of its own level; no wave waits for another workgroup.
// The arithmetic of g4s.h is factor_tile's three row functions and nothing else: each performs, per k ascending, w_p / u_kk and then w_t − (w_p · u_kj).
#include "common.hpp"
#include "frontier.hpp"
#include "call_util.hpp"
#include "readback.hpp"
#include "trsv.hpp"
#include "ilu.hpp"
#include "level_tile.hpp"
#include <algorithm>
#include <climits>
#include <memory>
#include <new>

struct g4s_ilu0_s {
    int n = 0;                          // first: the refusals of g4s_ilu0_apply_multi read nothing else (tests/test_trsv_multi_cpu.py asks them of a bare n)
    unsigned flags = 0;
    long long nnz = 0;
    g4s::DevBuf head, body;             // rowptr, dpos, the pivot word and the check's state; colids, a, f
    int *rowptr = nullptr, *dpos = nullptr, *colids = nullptr;
    unsigned *bad = nullptr;            // the pivot word of a factorisation whose caller passes none
    double *a = nullptr, *f = nullptr;  // the values last factorised; the factors
    g4s_trsv_t lower = nullptr, upper = nullptr;
    g4s_ilu0_info info{};
    ~g4s_ilu0_s()
    {
        (void)g4s_sptrsv_destroy(lower);
        (void)g4s_sptrsv_destroy(upper);
    }
};

namespace {

using g4s::IluState;

constexpr int kLaneRow = G4S_ILU0_LANE_ROW;
constexpr int kWaveRow = G4S_ILU0_WAVE_ROW;
constexpr size_t kStateBytes = 256;
constexpr unsigned kFlagMask = G4S_DEVICE_POINTERS | G4S_ILU0_NO_CHAINS;
static_assert(sizeof(IluState) <= kStateBytes, "state block");
static_assert((G4S_ILU0_NO_CHAINS & (G4S_DEVICE_POINTERS | G4S_TRSV_UPPER | G4S_TRSV_UNIT_DIAGONAL | G4S_TRSV_NO_CHAINS)) == 0u, "a bit of its own");

// ------------------------------------------------------------------------------------------------------------------------------- the check
__global__ __launch_bounds__(WG) void ilu_open_rows_kernel(int n, const int *__restrict__ rowptr, IluState *st)
{
    open_rows(n, rowptr, &st->invalid, 1, [](long long, int, int) {});
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->bad_id_row = st->bad_order_row = st->bad_diag_row = n;
        st->nnz_in = rowptr[n];                                    // means something only on a valid rowptr, and is used only then
    }
}

// One wave per row, behind a read of the state that found rowptr monotone from 0: [0, rowptr[n]) is the colids array. Ids are compared, never an index.
__global__ __launch_bounds__(WG) void ilu_open_ids_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ colids, int *__restrict__ dpos,
                                                          IluState *st)
{
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6); i < n; i += (long long)gridDim.x * (WG / 64)) {
        const int rb = rowptr[i], re = rowptr[i + 1];
        bool bad_id = false, bad_order = false;
        int at = -1;
        for (int k = rb + lane; k < re; k += 64) {
            const int c = colids[k];
            bad_id |= c < 0 || c >= n;
            if (k > rb) bad_order |= colids[k - 1] >= c;
            if (c == (int)i) at = k;
        }
        bad_id = __any(bad_id);
        bad_order = __any(bad_order);
        at = __shfl(wave_max(at), 0);
        if (lane == 0) {
            if (bad_id) atomicMin(&st->bad_id_row, (int)i);
            else if (bad_order) atomicMin(&st->bad_order_row, (int)i);
            else if (at < 0) atomicMin(&st->bad_diag_row, (int)i);
            dpos[i] = at;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ the factorisation
struct IluView {
    const int *rowptr, *colids, *dpos, *rowid, *loff;
    const double *a;
    double *f;
    unsigned *bad;
};

__device__ __forceinline__ void note_pivot(unsigned *bad, int i, double u)
{
    if (u == 0.0 || !(fabs(u) < __longlong_as_double(0x7FF0000000000000ll))) atomicMin(bad, (unsigned)i);
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Row i of m <= kLaneRow entries at rb, by one lane: columns and w in registers (every index below is a constant once unrolled).
template <bool kChain>
__device__ __forceinline__ void lane_row(const IluView &V, int i, int rb, int m)
{
    int c[kLaneRow];
    double w[kLaneRow];
#pragma unroll
    for (int t = 0; t < kLaneRow; ++t) {
        c[t] = t < m ? V.colids[rb + t] : INT_MAX;
        w[t] = t < m ? V.a[rb + t] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < kLaneRow; ++p) {
        const int k = c[p];
        if (k < i) {                                               // ascending: false from the diagonal on
            const int dk = V.dpos[k], ke = V.rowptr[k + 1];
            const double wp = w[p] / ld_prior<kChain>(V.f + dk);
            w[p] = wp;
            for (int q = dk + 1; q < ke; ++q) {
                const int j = V.colids[q];
                const double prod = wp * ld_prior<kChain>(V.f + q);
#pragma unroll
                for (int t = p + 1; t < kLaneRow; ++t)
                    if (c[t] == j) w[t] = w[t] - prod;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kLaneRow; ++t) {
        if (t < m) {
            const double v = canonical_nan(w[t]);
            V.f[rb + t] = v;
            if (c[t] == i) note_pivot(V.bad, i, v);
        }
    }
}

// The position of column j among cols[lo, hi), ascending; hi when it is not stored.
template <typename Cols>
__device__ __forceinline__ int find_col(Cols cols, int lo, int hi, int j)
{
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols(mid) < j) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && cols(lo) == j ? lo : end;
}

// Row i of kLaneRow < m <= kWaveRow entries at rb, by one wave (every lane calls with the same row): w and the columns in the wave's LDS share.
// Step p is read by every lane before lane 0 stores the quotient; the lanes then update distinct positions (row k's columns are distinct).
template <bool kChain>
__device__ __forceinline__ void wave_row(const IluView &V, int i, int rb, int m, double *sw, int *sc, int lane)
{
    for (int t = lane; t < m; t += 64) {
        sw[t] = V.a[rb + t];
        sc[t] = V.colids[rb + t];
    }
    wave_sync();
    const int nlow = V.dpos[i] - rb;
    for (int p = 0; p < nlow; ++p) {
        const int k = sc[p], dk = V.dpos[k], ke = V.rowptr[k + 1];
        const double wp = sw[p] / ld_prior<kChain>(V.f + dk);
        wave_sync();
        if (lane == 0) sw[p] = wp;
        for (int q = dk + 1 + lane; q < ke; q += 64) {
            const int j = V.colids[q];
            const double u = ld_prior<kChain>(V.f + q);
            const int t = find_col([&](int x) { return sc[x]; }, p + 1, m, j);
            if (t < m) sw[t] = sw[t] - wp * u;
        }
        wave_sync();
    }
    for (int t = lane; t < m; t += 64) {
        const double v = canonical_nan(sw[t]);
        V.f[rb + t] = v;
        if (t == nlow) note_pivot(V.bad, i, v);
    }
    wave_sync();                                                   // the share is free for the wave's next row
}

// Row i of more than kWaveRow entries, by the workgroup (every thread calls): w is the row of f itself. A value of it is stored plainly by one thread
// and read by others only with ld_prior<true> behind the __threadfence() and the __syncthreads() that end every step.
template <bool kChain>
__device__ __forceinline__ void hub_row(const IluView &V, int i, int t, double *s_wp)
{
    const int rb = V.rowptr[i], m = V.rowptr[i + 1] - rb, nlow = V.dpos[i] - rb;
    for (int q = t; q < m; q += WG) V.f[rb + q] = V.a[rb + q];
    __threadfence();
    __syncthreads();
    for (int p = 0; p < nlow; ++p) {
        const int k = V.colids[rb + p], dk = V.dpos[k], ke = V.rowptr[k + 1];
        if (t == 0) {
            const double wp = ld_prior<true>(V.f + rb + p) / ld_prior<kChain>(V.f + dk);
            V.f[rb + p] = wp;
            *s_wp = wp;
        }
        __syncthreads();
        const double wp = *s_wp;
        for (int q = dk + 1 + t; q < ke; q += WG) {
            const int j = V.colids[q];
            const double u = ld_prior<kChain>(V.f + q);
            const int x = find_col([&](int y) { return V.colids[rb + y]; }, p + 1, m, j);
            if (x < m) V.f[rb + x] = ld_prior<true>(V.f + rb + x) - wp * u;
        }
        __threadfence();
        __syncthreads();
    }
    for (int q = t; q < m; q += WG) {
        const double v = ld_prior<true>(V.f + rb + q);
        if (v != v) V.f[rb + q] = canonical_nan(v);
        if (q == nlow) note_pivot(V.bad, i, v);
    }
}

// Rows [lo, hi) of the schedule, all of one level, dealt by deal_tile (level_tile.hpp): a lane's rows first, then each wave its wave rows one after
// another, then the workgroup the longest ones. Who factorises a row never changes a bit of it.
struct IluRow {
    int m, i, rb;                                                  // stored entries, the row, and where they begin
};

template <bool kChain>
__device__ __forceinline__ void factor_tile(const IluView &V, int lo, int hi, int stride, int *s_hub, int *s_nh, double *s_w, int *s_c, double *s_wp)
{
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    deal_tile<kLaneRow, kWaveRow>(lo, hi, stride, s_hub, s_nh,
        [&](int p) {
            const int i = V.rowid[p], rb = V.rowptr[i];
            return IluRow{V.rowptr[i + 1] - rb, i, rb};
        },
        [&](const IluRow &r) { lane_row<kChain>(V, r.i, r.rb, r.m); },
        [&](const IluRow &r, int j) { wave_row<kChain>(V, __shfl(r.i, j), __shfl(r.rb, j), __shfl(r.m, j), s_w + wave * kWaveRow, s_c + wave * kWaveRow, lane); },
        [&](const IluRow &r, int) { hub_row<kChain>(V, r.i, t, s_wp); });
}

// one level that is not in a chain: a tile of WG / stride rows per workgroup
__global__ __launch_bounds__(WG) void ilu_level_kernel(const IluView V, int lo, int hi, int stride)
{
    __shared__ int s_hub[WG], s_nh, s_c[(WG / 64) * kWaveRow];
    __shared__ double s_w[(WG / 64) * kWaveRow], s_wp;
    const int2 tile = level_tile_bounds(lo, hi, stride);
    factor_tile<false>(V, tile.x, tile.y, stride, s_hub, &s_nh, s_w, s_c, &s_wp);
}

// a chain: one workgroup, levels [level_lo, level_hi), each at most WG rows; a later level reads what an earlier one stored (for_chain_levels)
__global__ __launch_bounds__(WG) void ilu_chain_kernel(const IluView V, int level_lo, int level_hi)
{
    __shared__ int s_hub[WG], s_nh, s_c[(WG / 64) * kWaveRow];
    __shared__ double s_w[(WG / 64) * kWaveRow], s_wp;
    for_chain_levels(V.loff, level_lo, level_hi, [&](int lo, int hi, int stride) { factor_tile<true>(V, lo, hi, stride, s_hub, &s_nh, s_w, s_c, &s_wp); });
}

// −1, no bad pivot: the largest unsigned, which every row with one lowers. A kernel, not a memset: a factorisation is captured into graphs.
__global__ void ilu_begin_kernel(unsigned *bad) { *bad = ~0u; }

// The factor launches on the values in P->a, the pivot word in front of them, and both plans refreshed from f. Enqueues only.
int enqueue_factor(g4s_ilu0_s *P, unsigned *bad, hipStream_t s)
{
    const g4s::LevelSchedule &S = g4s::trsv_schedule(P->lower);
    const IluView V{P->rowptr, P->colids, P->dpos, S.rowid, S.loff, P->a, P->f, bad};
    hipLaunchKernelGGL(ilu_begin_kernel, dim3(1), dim3(1), 0, s, bad);
    g4s::for_each_launch(S, g4s::ilu_stride,
        [&](int level_lo, int level_hi) { hipLaunchKernelGGL(ilu_chain_kernel, dim3(1), dim3(WG), 0, s, V, level_lo, level_hi); },
        [&](int lo, int hi, int stride, int grid) { hipLaunchKernelGGL(ilu_level_kernel, dim3((unsigned)grid), dim3(WG), 0, s, V, lo, hi, stride); });
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s_sptrsv_update_values(P->lower, P->f, G4S_DEVICE_POINTERS, s));
    G4S_TRY(g4s_sptrsv_update_values(P->upper, P->f, G4S_DEVICE_POINTERS, s));
    return G4S_OK;
}

// Everything of the analysis that touches the device; P is the caller's to delete on a failure. Returns behind a wait on `s` with nothing in flight,
// whatever the status — after a failure through the hipFree of the handle's blocks.
int analyse(g4s_ilu0_s *P, const int32_t *rowptr, const int32_t *colids, const double *values, bool device, g4s_ilu0_info *info, hipStream_t s)
{
    const int n = P->n;
    const hipMemcpyKind in = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    int cus = 1;
    G4S_HIP_TRY(g4s::device_cus(&cus));
    const size_t ni = sizeof(int) * (size_t)n;
    const size_t o_state = 0, o_bad = o_state + kStateBytes, o_rowptr = o_bad + 256, o_dpos = o_rowptr + pad256(ni + sizeof(int));
    G4S_TRY(P->head.alloc(o_dpos + pad256(ni)));
    char *hb = P->head.as<char>();
    IluState *st = reinterpret_cast<IluState *>(hb + o_state);
    P->bad = reinterpret_cast<unsigned *>(hb + o_bad);
    P->rowptr = reinterpret_cast<int *>(hb + o_rowptr);
    P->dpos = reinterpret_cast<int *>(hb + o_dpos);
    g4s::ReadScope reads(s);
    IluState h{};
    int launches = 0, waits = 0;

    G4S_HIP_TRY(hipMemsetAsync(st, 0, kStateBytes, s));
    G4S_HIP_TRY(hipMemcpyAsync(P->rowptr, rowptr, ni + sizeof(int), in, s));
    hipLaunchKernelGGL(ilu_open_rows_kernel, dim3(grid_rows(n, cus)), dim3(WG), 0, s, n, P->rowptr, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(reads.fetch(h, st));
    launches += 1;
    waits += 1;
    if (h.invalid) return g4s::set_error(G4S_ERR_INVALID, "g4s_ilu0_analyse: %s", csr_invalid_text(h.invalid));

    P->nnz = h.nnz_in;
    const size_t nz = (size_t)P->nnz;
    const size_t o_a = pad256(sizeof(int) * nz), o_f = o_a + pad256(sizeof(double) * nz);
    G4S_TRY(P->body.alloc(o_f + pad256(sizeof(double) * nz)));
    char *bb = P->body.as<char>();
    P->colids = reinterpret_cast<int *>(bb);
    P->a = reinterpret_cast<double *>(bb + o_a);
    P->f = reinterpret_cast<double *>(bb + o_f);
    G4S_HIP_TRY(hipMemcpyAsync(P->colids, colids, sizeof(int) * nz, in, s));
    G4S_HIP_TRY(hipMemcpyAsync(P->a, values, sizeof(double) * nz, in, s));
    G4S_HIP_TRY(hipMemcpyAsync(P->f, P->a, sizeof(double) * nz, hipMemcpyDeviceToDevice, s));   // what the two plans are analysed from: any values do
    hipLaunchKernelGGL(ilu_open_ids_kernel, dim3(grid_for<WG / 64>(n, 16LL * cus)), dim3(WG), 0, s, n, P->rowptr, P->colids, P->dpos, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(reads.fetch(h, st));
    launches += 1;
    waits += 1;
    const int bad_row = std::min(h.bad_id_row, std::min(h.bad_order_row, h.bad_diag_row));
    if (bad_row < n) {
        if (info) info->bad_row = bad_row;
        return g4s::set_error(G4S_ERR_INVALID, "g4s_ilu0_analyse: row %d %s", bad_row,
                              bad_row == h.bad_id_row      ? "stores a column id outside [0, n)"
                              : bad_row == h.bad_order_row ? "is not strictly ascending"
                                                           : "stores no diagonal entry");
    }

    const unsigned chains = (P->flags & G4S_ILU0_NO_CHAINS) ? G4S_TRSV_NO_CHAINS : 0u;
    g4s_trsv_info li{}, ui{};
    G4S_TRY(g4s_sptrsv_analyse(&P->lower, n, P->rowptr, P->colids, P->f, nullptr, G4S_DEVICE_POINTERS | G4S_TRSV_UNIT_DIAGONAL | chains, &li, s));
    G4S_TRY(g4s_sptrsv_analyse(&P->upper, n, P->rowptr, P->colids, P->f, nullptr, G4S_DEVICE_POINTERS | G4S_TRSV_UPPER | chains, &ui, s));

    G4S_TRY(enqueue_factor(P, P->bad, s));
    int bad_pivot = -1;
    G4S_HIP_TRY(reads.fetch(bad_pivot, P->bad));
    waits += 1;
    P->info.nnz = P->nnz;
    P->info.levels = li.levels;
    P->info.widest_level = li.widest_level;
    P->info.launches_per_factor = li.launches_per_solve;
    P->info.chains = li.chains;
    P->info.launches_per_apply = li.launches_per_solve + ui.launches_per_solve;
    P->info.bad_pivot = bad_pivot;
    P->info.launches = li.launches + ui.launches + launches + 1 + li.launches_per_solve + 2;   // the pivot word, the factor kernels, two refreshes
    P->info.host_waits = li.host_waits + ui.host_waits + waits;
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_ilu0_analyse(g4s_ilu0_t *out, int32_t n, const int32_t *rowptr, const int32_t *colids, const double *values, unsigned flags,
                                    g4s_ilu0_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~kFlagMask) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS and G4S_ILU0_NO_CHAINS");
    G4S_REQUIRE(out, "out is NULL");
    G4S_REQUIRE(n >= 0, "negative dimension");
    G4S_REQUIRE(rowptr, "rowptr is NULL");
    G4S_REQUIRE((colids && values) || n == 0, "colids or values is NULL");
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    if (!device) G4S_REQUIRE(rowptr[n] >= 0, "rowptr[n] is negative");
    const hipStream_t s = g4s::as_stream(stream);
    G4S_TRY(not_capturing(__func__, s, "its state"));
    if (info) { *info = g4s_ilu0_info{}; info->n = n; info->bad_row = -1; info->bad_pivot = -1; }
    std::unique_ptr<g4s_ilu0_s> P(new (std::nothrow) g4s_ilu0_s);
    if (!P) return g4s::set_error(G4S_ERR_NOMEM, "g4s_ilu0_analyse: no memory for the handle");
    P->n = n;
    P->flags = flags;
    P->info.n = n;
    P->info.bad_row = -1;
    P->info.bad_pivot = -1;
    if (n > 0) {
        const int status = analyse(P.get(), rowptr, colids, values, device, info, s);
        if (status != G4S_OK) {
            (void)hipStreamSynchronize(s);                         // the caller's arrays and the handle's blocks: nothing in flight touches them
            return status;
        }
    }
    if (info) *info = P->info;
    *out = P.release();
    return G4S_OK;
}

G4S_API g4s_status g4s_ilu0_factor(g4s_ilu0_t P, const double *values, unsigned flags, int32_t *bad_pivot_dev, void *stream)
{
    G4S_REQUIRE(P, "the handle is NULL");
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    const hipStream_t s = g4s::as_stream(stream);
    const bool host = values && !(flags & G4S_DEVICE_POINTERS);
    if (host) G4S_TRY(not_capturing(__func__, s, "nothing back, but copies a host array in and waits for it"));
    if (P->n == 0) {
        if (bad_pivot_dev) {
            hipLaunchKernelGGL(ilu_begin_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<unsigned *>(bad_pivot_dev));
            G4S_HIP_TRY(hipGetLastError());
        }
        return G4S_OK;
    }
    if (values) G4S_HIP_TRY(hipMemcpyAsync(P->a, values, sizeof(double) * (size_t)P->nnz, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    const int status = enqueue_factor(P, bad_pivot_dev ? reinterpret_cast<unsigned *>(bad_pivot_dev) : P->bad, s);
    if (host) {
        const hipError_t e = hipStreamSynchronize(s);              // whatever the status: the caller's array is free behind the call
        if (status == G4S_OK && e != hipSuccess) return g4s::set_error(G4S_ERR_HIP, "g4s_ilu0_factor: the wait failed: %s", hipGetErrorString(e));
    }
    return status;
}

G4S_API g4s_status g4s_ilu0_apply(g4s_ilu0_t P, const double *r_dev, double *z_dev, void *stream)
{
    G4S_REQUIRE(P, "the handle is NULL");
    if (P->n == 0) return G4S_OK;
    G4S_REQUIRE(r_dev && z_dev, "r or z is NULL");
    G4S_TRY(g4s_sptrsv_solve(P->lower, r_dev, z_dev, stream));
    return g4s_sptrsv_solve(P->upper, z_dev, z_dev, stream);
}

G4S_API g4s_status g4s_ilu0_apply_multi(g4s_ilu0_t P, int32_t k, const double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, unsigned flags,
                                        void *stream)
{
    G4S_REQUIRE(P, "the handle is NULL");
    const g4s::BlockCall call = g4s::check_block_call(__func__, P->n, k, "R", R_dev, ldr, "Z", Z_dev, ldz, flags);   // before P->lower is read
    if (!call.go_on) return call.status;
    G4S_TRY(g4s_sptrsv_solve_multi(P->lower, k, R_dev, ldr, Z_dev, ldz, flags, stream));
    return g4s_sptrsv_solve_multi(P->upper, k, Z_dev, ldz, Z_dev, ldz, flags, stream);
}

G4S_API g4s_status g4s_ilu0_get_factors(g4s_ilu0_t P, double *values_out, unsigned flags, void *stream)
{
    G4S_REQUIRE(P, "the handle is NULL");
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    if (P->n == 0 || P->nnz == 0) return G4S_OK;
    G4S_REQUIRE(values_out, "values_out is NULL");
    const hipStream_t s = g4s::as_stream(stream);
    const bool device = (flags & G4S_DEVICE_POINTERS) != 0;
    if (!device) G4S_TRY(not_capturing(__func__, s, "the factors"));
    G4S_HIP_TRY(hipMemcpyAsync(values_out, P->f, sizeof(double) * (size_t)P->nnz, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!device) G4S_HIP_TRY(hipStreamSynchronize(s));
    return G4S_OK;
}

G4S_API g4s_status g4s_ilu0_get_info(g4s_ilu0_t P, g4s_ilu0_info *info)
{
    G4S_REQUIRE(P && info, "the handle or info is NULL");
    *info = P->info;
    return G4S_OK;
}

G4S_API g4s_status g4s_ilu0_destroy(g4s_ilu0_t P)
{
    delete P;                                                      // hipFree waits for whatever still reads the handle
    return G4S_OK;
}
