// ewise.hip — element-wise combination and filtering of CSR matrices on the device (include/g4s.h: g4s_csr_ewise_symbolic / _numeric, g4s_csr_select_symbolic /
// _numeric). The reference has no such call: its reader mirrors a symmetric MatrixMarket file on the host (mm/inc/CSR.h:586-623).
//
// One work unit for every path (unit_walk.hpp: its constants, the row search, the walk of a wave through its run of units, the 16-lane sums; extract.hip
// shares it). The merged sequence of a row — its la entries of A and lb entries of B in ascending column order, A first on a tie, so that a
// matched pair is adjacent — is cut into units of T = kUnit positions; a row of la + lb positions has ceil((la + lb) / T) units and an empty row none. A unit is
// taken by kLanes = 16 adjacent lanes of a wave, kPer = 4 consecutive positions each:
//   ew_rows_kernel      rowptr of A (and B): zero-based and non-decreasing (fail bit 1), units per row, rows cut into more than one unit, the entry counts.
//   prims::exclusive_scan over the rows + 1 unit counts → the first unit of every row; its last element is the number of units.
//   ew_merge_kernel     a fixed grid; wave w owns the units [w·chunk, (w+1)·chunk), its four lane groups take them four at a time. A group finds its row by a
//                       galloping search from its previous row, the unit's first and last merge coordinates by two merge-path searches over the whole row (the
//                       loads are the same for its 16 lanes), every lane its own start by a search inside that window. A lane's end is its neighbour's start,
//                       so the lanes of a unit, and the units of a row, tile the row whatever the data holds: the search is a function of the diagonal alone.
//                       A lane walks at most kPer positions. Whether a position is kept depends on the entry beside it in the OTHER matrix, read from the row
//                       itself — a pair cut by a lane or unit boundary needs nothing else: B's copy looks one entry back in A, A's copy at the current one of B.
//     COUNT_ROWS        (symbolic) checks every entry it walks — id in [0, cols), larger than its predecessor in the row (fail bit 2; a tiling whose ends
//                       run backwards can only come from unsorted data and is the same failure) — and adds the unit's count to its row with one integer atomic.
//     COUNT_UNITS       (numeric) stores the unit's count; a scan gives every unit its first output slot.
//     FILL              (numeric) the same walk; a 16-lane scan of the kept counts, then each lane writes its run. Values: one IEEE operation or a copy.
//   sel_kernel          select: the units are T stored entries of one row, taken 16 at a time in stored order; kept entries are ranked by a ballot.
// No workgroup waits on another, no value goes through an atomic, nothing depends on timing. The host takes no decision between kernels: the symbolic calls wait
// for the device once. The numeric calls keep no state from the symbolic ones (nothing process-wide): they read the three entry counts (one wait, which sizes
// the per-unit arrays and the overlap check), recompute the unit table and the unit counts — one more read of the column ids — and wait once at the end.
//
// Memory safety rests on the row pointers alone: column ids are compared, never used as an index. Every kernel behind ew_rows_kernel returns at once when
// fail bit 1 is set, and FILL also when the counts it recomputed do not add up to crpt[rows] (fail bit 4: crpt is not what the symbolic call wrote).
#include "common.hpp"
#include "prims.hpp"
#include "readback.hpp"
#include "call_util.hpp"
#include "unit_walk.hpp"
#include <algorithm>

namespace {

constexpr int BAD_ROWPTR = 1, BAD_ENTRY = 2, BAD_CRPT = 4;

struct EwState {
    int fail, nnz_a, nnz_b, rows_split;
    unsigned long long cnnz;
};

// b may be NULL (select): its rows are empty. cnt (may be NULL): zeroed for COUNT_ROWS.
__global__ __launch_bounds__(WG) void ew_rows_kernel(int rows, const int32_t *__restrict__ arpt, const int32_t *__restrict__ brpt, int *__restrict__ upr,
                                                     int *__restrict__ cnt, EwState *__restrict__ st)
{
    for (long long r = (long long)blockIdx.x * WG + threadIdx.x; r <= rows; r += (long long)gridDim.x * WG) {
        const int a0 = arpt[r], b0 = brpt ? brpt[r] : 0;
        int units = 0;
        bool bad = r == 0 && (a0 != 0 || b0 != 0);
        if (r < rows) {
            const int a1 = arpt[r + 1], b1 = brpt ? brpt[r + 1] : 0;
            if (a1 < a0 || b1 < b0 || a0 < 0 || b0 < 0) bad = true;
            else units = (int)(((long long)(a1 - a0) + (b1 - b0) + kUnit - 1) / kUnit);
            if (units > 1) atomicAdd(&st->rows_split, 1);
        } else {
            st->nnz_a = a0;
            st->nnz_b = b0;
        }
        upr[r] = units;
        if (cnt) cnt[r] = 0;
        if (bad) atomicOr(&st->fail, BAD_ROWPTR);
    }
}

// The number of A's entries among the first d positions of the merged row: the least ia in [lo, hi] with a[ia] > b[d − 1 − ia]. The caller keeps
// max(0, d − lb) <= lo and hi <= min(d, la), so every index read lies inside the two rows whatever they hold.
__device__ __forceinline__ int merge_path(const int32_t *__restrict__ a, const int32_t *__restrict__ b, long long d, int lo, int hi)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// out: COUNT_ROWS → cnt[rows + 1] (zeroed), COUNT_UNITS → cnt[units], FILL → upos[units + 1] is read, ccol / cval are written.
template <int MODE, bool VALUES>
__global__ __launch_bounds__(WG) void ew_merge_kernel(int op, int combine, int rows, int cols, const int32_t *__restrict__ arpt, const int32_t *__restrict__ acol,
                                                      const double *__restrict__ aval, const int32_t *__restrict__ brpt, const int32_t *__restrict__ bcol,
                                                      const double *__restrict__ bval, const int *__restrict__ uoff, int units_cap, int *__restrict__ cnt,
                                                      const int *__restrict__ upos, const int32_t *__restrict__ crpt, int32_t *__restrict__ ccol,
                                                      double *__restrict__ cval, EwState *__restrict__ st)
{
    if (st->fail & BAD_ROWPTR) return;
    const int units = uoff[rows];
    if (units > units_cap) {                                       // the counts changed under the call
        if (threadIdx.x == 0) atomicOr(&st->fail, BAD_ROWPTR);
        return;
    }
    if (MODE == FILL && (st->fail || upos[units] != crpt[rows])) {
        if (threadIdx.x == 0 && !st->fail) atomicOr(&st->fail, BAD_CRPT);
        return;
    }
    UnitWalk w(units);
    const int lane = w.lane;
    int r = -1;
    unsigned long long total = 0;
    for (long long it = 0; it < w.chunk; it += kGroups) {          // the same trip count for every lane of the wave: the shuffles below are never divergent
        const long long ul = w.unit(it);
        const bool live = w.live(ul);
        int ia_s = 0, ia_e = 0, ib_s = 0, ib_e = 0, la = 0, lb = 0, last = 0;
        const int32_t *a = acol, *b = bcol;
        long long ka = 0, kb = 0;
        bool bad = false;
        if (live) {
            const int u = (int)ul;
            r = row_after(uoff, rows, r, u);
            ka = arpt[r];
            kb = brpt[r];
            la = arpt[r + 1] - (int)ka;
            lb = brpt[r + 1] - (int)kb;
            a = acol + ka;
            b = bcol + kb;
            const long long len = (long long)la + lb, u0 = (long long)(u - uoff[r]) * kUnit, u1 = min(u0 + kUnit, len);
            const int f0 = merge_path(a, b, u0, (int)max(0LL, u0 - lb), (int)min(u0, (long long)la));
            const int f1 = merge_path(a, b, u1, (int)max(0LL, u1 - lb), (int)min(u1, (long long)la));
            const long long d = min(u0 + (long long)lane * kPer, u1);
            ia_s = lane == 0 ? f0 : merge_path(a, b, d, (int)max((long long)f0, d - lb), (int)min(min((long long)f1, d), (long long)la));
            ib_s = (int)(d - ia_s);
            last = f1;
            ib_e = (int)(u1 - f1);
        }
        const int nia = __shfl_down(ia_s, 1, kLanes), nib = __shfl_down(ib_s, 1, kLanes);
        if (lane < kLanes - 1) { ia_e = nia; ib_e = nib; }
        else ia_e = last;
        if (ia_e < ia_s || ib_e < ib_s) {                          // only unsorted rows give a tiling that runs backwards
            bad = true;
            ia_e = ia_s;
            ib_e = ib_s;
        }
        int i = ia_s, j = ib_s, kept = 0;
        unsigned mask = 0;
        int32_t oc[kPer];
        double ov[kPer];
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            oc[t] = 0;
            ov[t] = 0.0;
            if (i < ia_e || j < ib_e) {
                const bool take_a = j >= ib_e || (i < ia_e && a[i] <= b[j]);
                int c;
                bool matched, keep;
                if (take_a) {
                    c = a[i];
                    if (MODE == COUNT_ROWS) bad |= (unsigned)c >= (unsigned)cols || (i > 0 && a[i - 1] >= c);
                    matched = j < lb && b[j] == c;
                    keep = op == G4S_EWISE_UNION || (op == G4S_EWISE_INTERSECT) == matched;
                    if (MODE == FILL && VALUES && keep) ov[t] = matched ? combine_values(combine, aval[ka + i], bval[kb + j]) : aval[ka + i];
                    ++i;
                } else {
                    c = b[j];
                    if (MODE == COUNT_ROWS) bad |= (unsigned)c >= (unsigned)cols || (j > 0 && b[j - 1] >= c);
                    matched = i > 0 && a[i - 1] == c;
                    keep = op == G4S_EWISE_UNION && !matched;
                    if (MODE == FILL && VALUES && keep) ov[t] = bval[kb + j];
                    ++j;
                }
                oc[t] = c;
                if (keep) {
                    mask |= 1u << t;
                    ++kept;
                }
            }
        }
        if (MODE == FILL) {
            const int incl = group_inclusive(kept, lane);
            if (live) {
                long long pos = (long long)upos[(int)ul] + incl - kept;
#pragma unroll
                for (int t = 0; t < kPer; ++t)
                    if (mask >> t & 1u) {
                        ccol[pos] = oc[t];
                        if (VALUES) cval[pos] = ov[t];
                        ++pos;
                    }
            }
        } else {
            const int sum = group_sum(kept);
            if (live && lane == 0) {
                if (MODE == COUNT_ROWS) {
                    if (sum) atomicAdd(&cnt[r], sum);
                    total += (unsigned long long)sum;
                } else {
                    cnt[(int)ul] = sum;
                }
            }
            if (bad) atomicOr(&st->fail, BAD_ENTRY);
        }
    }
    if (MODE == COUNT_ROWS && total) atomicAdd(&st->cnnz, total);
}

__device__ __forceinline__ bool select_keep(int pred, long long k, double thr, int row, int col, double v)
{
    const long long d = (long long)col - row;
    switch (pred) {
    case G4S_SELECT_TRIL: return d <= k;
    case G4S_SELECT_TRIU: return d >= k;
    case G4S_SELECT_OFFDIAG: return d != 0;
    case G4S_SELECT_DIAG: return d == 0;
    case G4S_SELECT_NONZERO: return v != 0.0;
    case G4S_SELECT_GT: return v > thr;
    case G4S_SELECT_GE: return v >= thr;
    case G4S_SELECT_LT: return v < thr;
    default: return v <= thr;
    }
}

// USE_VAL: the predicate reads values. VALUES (FILL): values are copied.
template <int MODE, bool USE_VAL, bool VALUES>
__global__ __launch_bounds__(WG) void sel_kernel(int pred, long long k, double thr, int rows, const int32_t *__restrict__ rpt, const int32_t *__restrict__ col,
                                                 const double *__restrict__ val, const int *__restrict__ uoff, int units_cap, int *__restrict__ cnt,
                                                 const int *__restrict__ upos, const int32_t *__restrict__ crpt, int32_t *__restrict__ ccol,
                                                 double *__restrict__ cval, EwState *__restrict__ st)
{
    if (st->fail & BAD_ROWPTR) return;
    const int units = uoff[rows];
    if (units > units_cap) {
        if (threadIdx.x == 0) atomicOr(&st->fail, BAD_ROWPTR);
        return;
    }
    if (MODE == FILL && (st->fail || upos[units] != crpt[rows])) {
        if (threadIdx.x == 0 && !st->fail) atomicOr(&st->fail, BAD_CRPT);
        return;
    }
    UnitWalk w(units);
    const int lane = w.lane, group = w.group;
    const unsigned below = (1u << lane) - 1u;
    int r = -1;
    unsigned long long total = 0;
    for (long long it = 0; it < w.chunk; it += kGroups) {          // uniform over the wave: the ballots see all four groups
        const long long ul = w.unit(it);
        const bool live = w.live(ul);
        long long k0 = 0, k1 = 0, pos = 0;
        if (live) {
            const int u = (int)ul;
            r = row_after(uoff, rows, r, u);
            k0 = rpt[r] + (long long)(u - uoff[r]) * kUnit;
            k1 = min(k0 + kUnit, (long long)rpt[r + 1]);
            if (MODE == FILL) pos = upos[u];
        }
        int kept = 0;
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const long long e = k0 + t * kLanes + lane;
            bool keep = false;
            int c = 0;
            double v = 0.0;
            if (e < k1) {
                c = col[e];
                if (USE_VAL || (MODE == FILL && VALUES)) v = val[e];
                keep = select_keep(pred, k, thr, r, c, v);
            }
            const unsigned gm = (unsigned)(__ballot(keep) >> (group * kLanes)) & 0xffffu;
            if (MODE == FILL) {
                if (keep) {
                    const long long p = pos + __popc(gm & below);
                    ccol[p] = c;
                    if (VALUES) cval[p] = v;
                }
                pos += __popc(gm);
            } else {
                kept += __popc(gm);
            }
        }
        if (MODE != FILL && live && lane == 0) {
            if (MODE == COUNT_ROWS) {
                if (kept) atomicAdd(&cnt[r], kept);
                total += (unsigned long long)kept;
            } else {
                cnt[(int)ul] = kept;
            }
        }
    }
    if (MODE == COUNT_ROWS && total) atomicAdd(&st->cnnz, total);
}

// The operands of one call, device arrays. b* are NULL for select; op / combine are then pred and unused.
struct Job {
    const char *fn;
    bool select;
    int op, combine;
    long long k;
    double thr;
    int rows, cols;
    const int32_t *arpt, *acol;
    const double *aval;
    const int32_t *brpt, *bcol;
    const double *bval;
    bool use_val() const { return select && op >= G4S_SELECT_NONZERO; }
};

template <int MODE>
void launch(const Job &j, bool values, const int *uoff, int units_cap, int *cnt, const int *upos, const int32_t *crpt, int32_t *ccol, double *cval, EwState *st,
            hipStream_t s)
{
    const dim3 g(kGridWG), b(WG);
    if (j.select) {
#define SEL_ARGS j.op, j.k, j.thr, j.rows, j.arpt, j.acol, j.aval, uoff, units_cap, cnt, upos, crpt, ccol, cval, st
        if (j.use_val()) {
            if (values) hipLaunchKernelGGL((sel_kernel<MODE, true, true>), g, b, 0, s, SEL_ARGS);
            else hipLaunchKernelGGL((sel_kernel<MODE, true, false>), g, b, 0, s, SEL_ARGS);
        } else {
            if (values) hipLaunchKernelGGL((sel_kernel<MODE, false, true>), g, b, 0, s, SEL_ARGS);
            else hipLaunchKernelGGL((sel_kernel<MODE, false, false>), g, b, 0, s, SEL_ARGS);
        }
#undef SEL_ARGS
    } else {
#define EW_ARGS j.op, j.combine, j.rows, j.cols, j.arpt, j.acol, j.aval, j.brpt, j.bcol, j.bval, uoff, units_cap, cnt, upos, crpt, ccol, cval, st
        if (values) hipLaunchKernelGGL((ew_merge_kernel<MODE, true>), g, b, 0, s, EW_ARGS);
        else hipLaunchKernelGGL((ew_merge_kernel<MODE, false>), g, b, 0, s, EW_ARGS);
#undef EW_ARGS
    }
}

int contract_error(const Job &j, int fail)
{
    if (fail & BAD_ROWPTR) return g4s::set_error(G4S_ERR_INVALID, "%s: a rowptr is not zero-based and non-decreasing", j.fn);
    if (fail & BAD_CRPT) return g4s::set_error(G4S_ERR_INVALID, "%s: crpt[rows] is not the entry count of this operation: crpt must come from the symbolic call", j.fn);
    return g4s::set_error(G4S_ERR_INVALID, "%s: the rows of A and B must be strictly ascending with column ids in [0, %d)", j.fn, j.cols);
}

// Device arrays; the stream is synchronised on return. crpt: rows + 1 ints, written. One wait.
int symbolic_device(const Job &j, int32_t *crpt, int64_t *cnnz, g4s_ewise_info *info, hipStream_t s)
{
    const size_t n1 = sizeof(int) * ((size_t)j.rows + 1);
    EwState *st;
    int *upr, *uoff, *cnt;
    Carver work;
    work.piece(&st, sizeof(EwState));
    work.piece(&upr, n1);
    work.piece(&uoff, n1);
    work.piece(&cnt, n1);
    G4S_TRY(work.alloc());
    g4s::ReadScope reads(s);
    EwState h{};
    int units = 0;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(EwState), s));
    hipLaunchKernelGGL(ew_rows_kernel, dim3(grid_for<WG>((long long)j.rows + 1, kGridWG)), dim3(WG), 0, s, j.rows, j.arpt, j.brpt, upr, cnt, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(upr), uoff, (long long)j.rows + 1, s));
    if (j.rows > 0) launch<COUNT_ROWS>(j, false, uoff, INT_MAX, cnt, nullptr, nullptr, nullptr, nullptr, st, s);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(cnt), crpt, (long long)j.rows + 1, s));
    G4S_HIP_TRY(reads.note(h, st));
    G4S_HIP_TRY(reads.fetch(units, uoff + j.rows));
    work.idle();                                                   // (an early return above leaves it out: the block is then released behind a device-wide wait)
    if (h.fail) return contract_error(j, h.fail);
    {
        info->nnz_a = h.nnz_a;
        info->nnz_b = h.nnz_b;
        info->nnz_c = (int64_t)h.cnnz;
        info->units = units;
        info->unit_entries = kUnit;
        info->rows_split = h.rows_split;
        info->host_waits = 1;
    }
    *cnnz = (int64_t)h.cnnz;
    if (h.cnnz > (unsigned long long)INT32_MAX) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: %llu entries exceed the int32 row pointers", j.fn, h.cnnz);
    return G4S_OK;
}

// Device arrays, the three entry counts already read (and checked >= 0); the stream is synchronised on return.
int numeric_device(const Job &j, long long nnz_a, long long nnz_b, long long nnz_c, const int32_t *crpt, int32_t *ccol, double *cval, hipStream_t s)
{
    if (nnz_c == 0) return G4S_OK;
    if (too_many_units(j.rows, (unsigned long long)(nnz_a + nnz_b))) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: more than 2^31 work units", j.fn);
    const long long cap = unit_cap(j.rows, (unsigned long long)(nnz_a + nnz_b));
    const size_t n1 = sizeof(int) * ((size_t)j.rows + 1), u1 = sizeof(int) * ((size_t)cap + 1);
    EwState *st;
    int *upr, *uoff, *ucnt, *upos;
    Carver work;
    work.piece(&st, sizeof(EwState));
    work.piece(&upr, n1);
    work.piece(&uoff, n1);
    work.piece(&ucnt, u1);
    work.piece(&upos, u1);
    G4S_TRY(work.alloc());
    int fail = 0;
    G4S_HIP_TRY(hipMemsetAsync(st, 0, sizeof(EwState), s));
    G4S_HIP_TRY(hipMemsetAsync(ucnt, 0, u1, s));
    hipLaunchKernelGGL(ew_rows_kernel, dim3(grid_for<WG>((long long)j.rows + 1, kGridWG)), dim3(WG), 0, s, j.rows, j.arpt, j.brpt, upr, (int *)nullptr, st);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(upr), uoff, (long long)j.rows + 1, s));
    launch<COUNT_UNITS>(j, false, uoff, (int)cap, ucnt, nullptr, nullptr, nullptr, nullptr, st, s);
    G4S_HIP_TRY(hipGetLastError());
    G4S_TRY(g4s::prims::exclusive_scan(static_cast<const int *>(ucnt), upos, cap + 1, s));
    launch<FILL>(j, cval != nullptr, uoff, (int)cap, nullptr, upos, crpt, ccol, cval, st, s);
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(g4s::ReadScope(s).fetch(fail, &st->fail));
    work.idle();                                                   // (as in symbolic_device)
    if (fail) return contract_error(j, fail);
    return G4S_OK;
}

// arpt[rows], brpt[rows] (brpt may be NULL) and crpt[rows] (may be NULL) of device arrays: one wait
int read_counts(const Job &j, const int32_t *crpt, long long *na, long long *nb, long long *nc, hipStream_t s)
{
    g4s::ReadScope reads(s);
    int a = 0, b = 0, c = 0;
    G4S_HIP_TRY(reads.note(a, j.arpt + j.rows));
    if (j.brpt) G4S_HIP_TRY(reads.note(b, j.brpt + j.rows));
    if (crpt) G4S_HIP_TRY(reads.note(c, crpt + j.rows));
    G4S_HIP_TRY(reads.wait());
    if (a < 0 || b < 0 || c < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: a negative entry count (rowptr[rows] %d, %d, crpt[rows] %d)", j.fn, a, b, c);
    *na = a; *nb = b; *nc = c;
    return G4S_OK;
}

// The input arrays of a job with the given entry counts, as spans for the overlap check.
struct Inputs {
    Span s[6];
};
Inputs input_spans(const Job &j, long long na, long long nb)
{
    const size_t rp = 4 * ((size_t)j.rows + 1);
    return Inputs{{{j.arpt, rp}, {j.acol, 4 * (size_t)na}, {j.aval, 8 * (size_t)na}, {j.brpt, j.brpt ? rp : 0}, {j.bcol, 4 * (size_t)nb}, {j.bval, 8 * (size_t)nb}}};
}

int symbolic(Job j, int32_t *crpt, int64_t *cnnz, unsigned flags, g4s_ewise_info *info, hipStream_t s)
{
    const size_t rp = 4 * ((size_t)j.rows + 1);
    const bool dev = flags & G4S_DEVICE_POINTERS;
    if (j.rows > INT_MAX - (1 << 27)) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: too many rows for the int32 unit table", j.fn);
    // what can be known without the device: with host arrays everything, with device arrays the row pointers (the column arrays after the one wait)
    const long long na = dev ? 0 : j.arpt[j.rows], nb = dev || !j.brpt ? 0 : j.brpt[j.rows];
    if (na < 0 || nb < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: a negative entry count", j.fn);
    {
        const Span outs[] = {{crpt, rp}, {cnnz, sizeof(int64_t)}};
        if (any_overlap(outs, input_spans(j, na, nb).s)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input array", j.fn);
    }
    G4S_TRY(not_capturing(j.fn, s));
    if (info) *info = g4s_ewise_info{};
    *cnnz = 0;
    g4s_ewise_info local{};
    if (!info) info = &local;
    if (dev) {
        const int st = symbolic_device(j, crpt, cnnz, info, s);
        if (st != G4S_OK && st != G4S_ERR_OVERFLOW) return st;
        const Span outs[] = {{crpt, rp}};                          // the column arrays' lengths are known only now
        if (any_overlap(outs, input_spans(j, info->nnz_a, info->nnz_b).s))
            return g4s::set_error(G4S_ERR_INVALID, "%s: crpt overlaps a column or value array", j.fn);
        return st;
    }
    Staged stage(s);
    Job d = j;
    d.arpt = stage.in(j.arpt, rp);
    d.acol = stage.in(j.acol, 4 * (size_t)na);
    d.aval = j.use_val() ? stage.in(j.aval, 8 * (size_t)na) : nullptr;
    d.brpt = stage.in(j.brpt, rp);                                   // (NULL for select)
    d.bcol = stage.in(j.bcol, 4 * (size_t)nb);
    d.bval = nullptr;
    int32_t *d_crpt = stage.out<int32_t>(rp);
    int status = stage.error();
    if (status == G4S_OK) status = symbolic_device(d, d_crpt, cnnz, info, s);
    if (status == G4S_OK || status == G4S_ERR_OVERFLOW) {          // crpt comes back with the overflow too
        int back = stage.to_host(crpt, d_crpt, rp);
        if (back == G4S_OK) back = stage.wait();
        if (back != G4S_OK) status = back;
    }
    return stage.finish(status);
}

int numeric(Job j, const int32_t *crpt, int32_t *ccol, double *cval, unsigned flags, hipStream_t s)
{
    const size_t rp = 4 * ((size_t)j.rows + 1);
    const bool dev = flags & G4S_DEVICE_POINTERS;
    if (j.rows > INT_MAX - (1 << 27)) return g4s::set_error(G4S_ERR_OVERFLOW, "%s: too many rows for the int32 unit table", j.fn);
    long long na = 0, nb = 0, nc = 0;
    auto check_overlap = [&]() -> int {
        const Span outs[] = {{ccol, 4 * (size_t)nc}, {cval, 8 * (size_t)nc}};
        Inputs in = input_spans(j, na, nb);
        const Span ins[] = {in.s[0], in.s[1], in.s[2], in.s[3], in.s[4], in.s[5], {crpt, rp}};
        if (any_overlap(outs, ins)) return g4s::set_error(G4S_ERR_INVALID, "%s: an output overlaps an input array", j.fn);
        return G4S_OK;
    };
    if (!dev) {
        na = j.arpt[j.rows]; nb = j.brpt ? j.brpt[j.rows] : 0; nc = crpt[j.rows];
        if (na < 0 || nb < 0 || nc < 0) return g4s::set_error(G4S_ERR_INVALID, "%s: a negative entry count", j.fn);
        G4S_TRY(check_overlap());
    }
    G4S_TRY(not_capturing(j.fn, s));
    if (dev) {
        G4S_TRY(read_counts(j, crpt, &na, &nb, &nc, s));
        G4S_TRY(check_overlap());
        return numeric_device(j, na, nb, nc, crpt, ccol, cval, s);
    }
    if (nc == 0) return G4S_OK;
    Staged stage(s);
    Job d = j;
    d.arpt = stage.in(j.arpt, rp);
    d.acol = stage.in(j.acol, 4 * (size_t)na);
    d.aval = stage.in(j.aval, 8 * (size_t)na);
    d.brpt = stage.in(j.brpt, rp);                                   // (NULL for select)
    d.bcol = stage.in(j.bcol, 4 * (size_t)nb);
    d.bval = stage.in(j.bval, 8 * (size_t)nb);
    const int32_t *d_crpt = stage.in(crpt, rp);
    int32_t *d_ccol = stage.out<int32_t>(4 * (size_t)nc);
    double *d_cval = cval ? stage.out<double>(8 * (size_t)nc) : nullptr;
    int status = stage.error();
    if (status == G4S_OK) status = numeric_device(d, na, nb, nc, d_crpt, d_ccol, d_cval, s);
    if (status == G4S_OK) status = stage.to_host(ccol, d_ccol, 4 * (size_t)nc);
    if (status == G4S_OK && cval) status = stage.to_host(cval, d_cval, 8 * (size_t)nc);
    if (status == G4S_OK) status = stage.wait();
    return stage.finish(status);
}

bool valid_op(int op) { return op >= G4S_EWISE_UNION && op <= G4S_EWISE_DIFFERENCE; }
bool valid_combine(int c) { return c >= G4S_COMBINE_PLUS && c <= G4S_COMBINE_SECOND; }
bool valid_pred(int p) { return p >= G4S_SELECT_TRIL && p <= G4S_SELECT_LE; }

} // namespace

G4S_API g4s_status g4s_csr_ewise_symbolic(int op, int32_t rows, int32_t cols, const int32_t *arpt, const int32_t *acol, const int32_t *brpt, const int32_t *bcol,
                                          int32_t *crpt, int64_t *cnnz, unsigned flags, g4s_ewise_info *info, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_op(op), "op is not a G4S_EWISE_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(arpt && brpt && crpt && cnnz, "arpt, brpt, crpt or cnnz is NULL");
    G4S_REQUIRE((acol && bcol) || rows == 0, "acol or bcol is NULL");
    const Job j{__func__, false, op, G4S_COMBINE_PLUS, 0, 0.0, rows, cols, arpt, acol, nullptr, brpt, bcol, nullptr};
    return symbolic(j, crpt, cnnz, flags, info, g4s::as_stream(stream));
}

G4S_API g4s_status g4s_csr_ewise_numeric(int op, int combine, int32_t rows, int32_t cols, const int32_t *arpt, const int32_t *acol, const double *aval,
                                         const int32_t *brpt, const int32_t *bcol, const double *bval, const int32_t *crpt, int32_t *ccol, double *cval,
                                         unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_op(op), "op is not a G4S_EWISE_* value");
    G4S_REQUIRE(valid_combine(combine), "combine is not a G4S_COMBINE_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(arpt && brpt && crpt, "arpt, brpt or crpt is NULL");
    G4S_REQUIRE((acol && bcol && ccol) || rows == 0, "acol, bcol or ccol is NULL");
    G4S_REQUIRE((aval == nullptr) == (bval == nullptr) && (aval == nullptr) == (cval == nullptr),
                "aval, bval and cval must all be given or all be NULL (pattern-only)");
    const Job j{__func__, false, op, combine, 0, 0.0, rows, cols, arpt, acol, aval, brpt, bcol, bval};
    return numeric(j, crpt, ccol, cval, flags, g4s::as_stream(stream));
}

G4S_API g4s_status g4s_csr_select_symbolic(int pred, int64_t k, double thr, int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, const double *val,
                                           int32_t *crpt, int64_t *cnnz, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_pred(pred), "pred is not a G4S_SELECT_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(rpt && crpt && cnnz, "rpt, crpt or cnnz is NULL");
    G4S_REQUIRE(col || rows == 0, "col is NULL");
    G4S_REQUIRE(val || pred < G4S_SELECT_NONZERO, "a value predicate without val");
    const Job j{__func__, true, pred, 0, (long long)k, thr, rows, cols, rpt, col, val, nullptr, nullptr, nullptr};
    return symbolic(j, crpt, cnnz, flags, nullptr, g4s::as_stream(stream));
}

G4S_API g4s_status g4s_csr_select_numeric(int pred, int64_t k, double thr, int32_t rows, int32_t cols, const int32_t *rpt, const int32_t *col, const double *val,
                                          const int32_t *crpt, int32_t *ccol, double *cval, unsigned flags, void *stream)
{
    G4S_REQUIRE((flags & ~G4S_DEVICE_POINTERS) == 0u, "flags other than G4S_HOST_POINTERS / G4S_DEVICE_POINTERS");
    G4S_REQUIRE(valid_pred(pred), "pred is not a G4S_SELECT_* value");
    G4S_REQUIRE(rows >= 0 && cols >= 0, "negative dimension");
    G4S_REQUIRE(rpt && crpt, "rpt or crpt is NULL");
    G4S_REQUIRE((col && ccol) || rows == 0, "col or ccol is NULL");
    G4S_REQUIRE(val || pred < G4S_SELECT_NONZERO, "a value predicate without val");
    G4S_REQUIRE(val || !cval, "cval without val");
    const Job j{__func__, true, pred, 0, (long long)k, thr, rows, cols, rpt, col, val, nullptr, nullptr, nullptr};
    return numeric(j, crpt, ccol, cval, flags, g4s::as_stream(stream));
}
