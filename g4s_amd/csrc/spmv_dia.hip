// spmv_dia.hip — the diagonal-form SpMV path of a CSR handle (csr.hip): plan, builder, value refresh and kernels.
#include "common.hpp"
#include "spmv_dia.hpp"
#include "spmv_device.hpp"
#include "semiring.hpp"
#include <algorithm>
#include <memory>
#include <vector>

namespace g4s {
namespace {

constexpr int WG = 256;

// ---- diagonal-structured matrices (stencils, banded): the index-free path.
// When every entry's offset col − row comes from a small set (≤ 32 distinct values: 5 for the 5-point, 7 for the 7-point Laplacian, 2·hb+1 for
// a band) the column indices carry no information: the values are stored by diagonal, dia[d·ld + row] = A(row, row + off[d]) (0 where the
// diagonal has no entry in that row — a boundary row), plus one 32-bit presence mask per row. One lane per row: all nd value loads and all nd
// (unit-stride, shifted) loads of x go out together, then the present products are added in ascending offset = ascending column order —
// the order of the CSR row, so the result is bit-identical to the oracle. 8·nd + 4 + 8 bytes per row instead of 12·nd + 4 + 8, and the
// x loads are coalesced instead of gathered (what north_star calls the dense-tile fallback, in the form that pays for a mat-vec: drop the
// indices — a 2-flop-per-entry product gains nothing from the matrix cores).
constexpr int kMaxDiags = 32;
struct DiaOffsets { int off[kMaxDiags]; };
// Which rows an XCD walks. Blocks of one XCD walk a contiguous eighth of the rows, so that the shifted reads of x of neighbouring row blocks go through one L2.
// A 3-D stencil has two diagonals one PLANE away (±431² for the 431³ Laplacian) and x[row + plane] is needed again one and two planes later; with contiguous
// eighths that reuse distance is three planes of x plus the streams in between, more than a 4 MiB L2, so x crosses the fabric three times (PMC: 6.72 GB fetched
// for 5.44 GB of own reads). Round 3 built a plane-sliced walk (XCD j takes the j-th eighth of EVERY plane, plane after plane: 5.65 GB fetched, L2 hit 0.36
// instead of 0.20) and a variant with staggered starting planes; on one handle in one process they ran 1 % and 5–8 % SLOWER on four boxes (DESIGN §4.1:
// profiles/r03_ab_lap7_walks.txt) — the kernel is not bound by the bytes that cross the fabric — and were removed in round 4. Likewise the switch back to one
// row per lane (two rows per lane: −4 % / −10 %, profiles/r03, tools history).

template <int ND, bool NT, class S>
__global__ __launch_bounds__(WG) void spmv_dia_kernel(int rows, int cols, int nd, DiaOffsets offs, long long ld, const double *__restrict__ dia,
                                                       const unsigned *__restrict__ mask, const double *__restrict__ x, double *__restrict__ y,
                                                       double alpha, double beta, int blocks_per_xcd, int row0 /* first row of this launch */)
{
    // blocks of one XCD walk a contiguous range of rows: neighbouring row blocks read neighbouring parts of x through the same L2
    const int b = (int)blockIdx.x;
    const int lb = (b % g4s::kXcds) * blocks_per_xcd + b / g4s::kXcds;
    const int row = row0 + lb * WG + (int)threadIdx.x;
    if (row >= rows) return;
    const unsigned m = mask[row];
    double v[ND], xv[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < nd) {
            v[d] = NT ? __builtin_nontemporal_load(dia + (long long)d * ld + row) : dia[(long long)d * ld + row];   // G4S_SPMV_NO_NT is honoured here too
            const int c = min(max(row + offs.off[d], 0), cols - 1);       // absent entries read a clamped (unused) position
            xv[d] = x[c];
        }
    double s = S::identity();
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < nd && ((m >> d) & 1u)) s = S::combine(s, S::mul(v[d], xv[d]));
    store_y<S>(y, row, s, alpha, beta);
}

// Two consecutive rows per lane: the diagonal values, the masks and y move as 16-byte / 8-byte accesses per lane instead of 8 / 4 (the memory pipeline's
// preferred width); the arithmetic of a row is unchanged (same products, same order: bit-identical). Launched when y is 16-byte aligned and the matrix
// has at most 16 diagonals (registers); the last lane of an odd row count takes the one-row path above through `rows2`.
typedef double dia_double2 __attribute__((ext_vector_type(2)));
typedef unsigned dia_uint2 __attribute__((ext_vector_type(2)));
template <int ND, bool NT, class S>
__global__ __launch_bounds__(WG) void spmv_dia2_kernel(int rows2 /* even part of the row count */, int cols, int nd, DiaOffsets offs, long long ld, const double *__restrict__ dia,
                                                        const unsigned *__restrict__ mask, const double *__restrict__ x, double *__restrict__ y,
                                                        double alpha, double beta, int blocks_per_xcd)
{
    const int b = (int)blockIdx.x;
    const int lb = (b % g4s::kXcds) * blocks_per_xcd + b / g4s::kXcds;
    const int row = 2 * (lb * WG + (int)threadIdx.x);
    if (row >= rows2) return;
    const dia_uint2 m = *reinterpret_cast<const dia_uint2 *>(mask + row);
    dia_double2 v[ND];
    double x0[ND], x1[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < nd) {
            const dia_double2 *p = reinterpret_cast<const dia_double2 *>(dia + (long long)d * ld + row);
            v[d] = NT ? __builtin_nontemporal_load(p) : *p;
            const int c = row + offs.off[d];
            x0[d] = x[min(max(c, 0), cols - 1)];
            x1[d] = x[min(max(c + 1, 0), cols - 1)];
        }
    double s0 = S::identity(), s1 = S::identity();
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < nd) {
            if ((m[0] >> d) & 1u) s0 = S::combine(s0, S::mul(v[d][0], x0[d]));
            if ((m[1] >> d) & 1u) s1 = S::combine(s1, S::mul(v[d][1], x1[d]));
        }
    dia_double2 out;
    if constexpr (!g4s::semiring::is_plus_times<S>) {
        if (beta == 0.0) { out[0] = s0; out[1] = s1; }
        else {
            const dia_double2 old = *reinterpret_cast<const dia_double2 *>(y + row);
            out[0] = S::combine(s0, S::normalize(old[0])); out[1] = S::combine(s1, S::normalize(old[1]));
        }
    } else if (beta == 0.0) { out[0] = alpha * s0; out[1] = alpha * s1; }
    else {
        const dia_double2 old = *reinterpret_cast<const dia_double2 *>(y + row);
        out[0] = alpha * s0 + beta * old[0]; out[1] = alpha * s1 + beta * old[1];
    }
    *reinterpret_cast<dia_double2 *>(y + row) = out;
}

// One thread per row scatters the row's entries into their diagonals; fail |= 1 when an offset is not in the candidate set, a row holds
// the same column twice (a diagonal has one slot per row), or a row's columns are not ascending — the kernel adds the products in offset
// order, which is the oracle's (stored) order only for sorted rows, and "bit-identical" is what this path promises.
__global__ void dia_fill_kernel(int rows, int nd, DiaOffsets offs, long long ld, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colids,
                                const double *__restrict__ values, double *__restrict__ dia, unsigned *__restrict__ mask, int *__restrict__ fail)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    unsigned m = 0;
    int prev = -1;
    for (int k = rowptr[row]; k < rowptr[row + 1]; ++k) {
        const int o = colids[k] - row;
        int lo = 0, hi = nd;                                       // offs.off is ascending
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (offs.off[mid] < o) lo = mid + 1; else hi = mid; }
        if (lo >= nd || offs.off[lo] != o || lo <= prev) { atomicOr(fail, 1); return; }   // lo <= prev: a repeated or a descending column
        prev = lo;
        m |= 1u << lo;
        dia[(long long)lo * ld + row] = values[k];
    }
    mask[row] = m;
}

// new values into the diagonals. The pattern is the plan's: row r's entries are its present diagonals in ascending offset order (dia_fill_kernel checked
// that at create), so entry j of the row belongs to the j-th set bit of its mask — no column ids, no search; one lane per row, the loads of a row's values in
// flight together, the stores unit-stride per diagonal.
template <int ND>
__global__ __launch_bounds__(256) void dia_refill_kernel(int rows, int nd, long long ld, const int32_t *__restrict__ rowptr, const unsigned *__restrict__ mask,
                                                         const double *__restrict__ values, double *__restrict__ dia)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const unsigned m = mask[row];
    if (!m) return;                                                // an empty row stores nothing, and its k0 may be nnz: one past the caller's array
    const int k0 = rowptr[row], last = rowptr[row + 1] - 1;        // m != 0: the row has an entry, so k0 <= last <= nnz − 1
    double v[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) v[d] = values[min(k0 + (int)__popc(m & ((1u << d) - 1u)), last)];   // (absent diagonals read a neighbour: not stored)
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < nd && ((m >> d) & 1u)) dia[(long long)d * ld + row] = v[d];
}

// The nontemporal or the plain instantiation of a kernel, same grid and arguments.
template <class... P, class... Args>
void launch_pair(bool nt, void (*k_nt)(P...), void (*k_plain)(P...), dim3 grid, hipStream_t s, Args... args)
{
    void (*const kernel)(P...) = nt ? k_nt : k_plain;
    hipLaunchKernelGGL(kernel, grid, dim3(WG), 0, s, args...);
}

} // namespace

struct DiaPlan {
    int rows = 0, cols = 0, nd = 0;
    long long ld = 0;
    bool use_nt = true;
    const int32_t *d_rowptr = nullptr;   // borrowed from the CSR handle
    DiaOffsets offs{};
    DevBuf dia;                          // nd·ld values by diagonal
    DevBuf mask;                         // presence bits per row
};

// Try the diagonal-structured form: candidate offsets from a sample of rows (first, middle, last 2048), then one pass over the matrix that
// either fills the diagonals or reports an entry outside the candidate set. Kept when the diagonals are at least 60 % full.
// *out stays NULL (status OK) when the matrix does not have that form, or when there is no room for it.
int dia_try_build(DiaPlan **out, int rows, int cols, long long nnz, const int32_t *d_rowptr, const int32_t *d_colids, const double *d_values, bool use_nt)
{
    *out = nullptr;
    if (rows < 1024 || nnz < 4096) return G4S_OK;
    std::vector<int> offs;
    const int S = 2048;
    std::vector<int32_t> cbuf;
    for (int part = 0; part < 3; ++part) {
        const int32_t ra = part == 0 ? 0 : (part == 1 ? std::max(0, rows / 2 - S / 2) : std::max(0, rows - S)), rb = std::min(rows, ra + S);
        std::vector<int32_t> rp_slice((size_t)(rb - ra) + 1);     // the sampled rows' pointers, from the device copy
        G4S_HIP_TRY(hipMemcpy(rp_slice.data(), d_rowptr + ra, sizeof(int32_t) * rp_slice.size(), hipMemcpyDeviceToHost));
        const int32_t *h_rowptr = rp_slice.data() - ra;
        const int64_t k0 = h_rowptr[ra], k1 = h_rowptr[rb];
        if (k1 - k0 > 64ll * S) return G4S_OK;                     // rows this long are not a stencil
        cbuf.resize((size_t)(k1 - k0));
        if (k1 > k0) G4S_HIP_TRY(hipMemcpy(cbuf.data(), d_colids + k0, sizeof(int32_t) * (size_t)(k1 - k0), hipMemcpyDeviceToHost));
        for (int32_t r = ra; r < rb; ++r)
            for (int64_t k = h_rowptr[r]; k < h_rowptr[r + 1]; ++k) offs.push_back(cbuf[(size_t)(k - k0)] - r);
        std::sort(offs.begin(), offs.end());
        offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
        if ((int)offs.size() > kMaxDiags) return G4S_OK;
    }
    const int nd = (int)offs.size();
    if (nd == 0 || (double)nnz < 0.6 * (double)nd * rows) return G4S_OK;
    auto P = std::make_unique<DiaPlan>();
    P->rows = rows; P->cols = cols; P->nd = nd; P->use_nt = use_nt; P->d_rowptr = d_rowptr;
    for (int d = 0; d < nd; ++d) P->offs.off[d] = offs[d];
    P->ld = ((long long)rows + 63) / 64 * 64;
    DevBuf fail;
    if (P->dia.alloc(sizeof(double) * (size_t)(P->ld * nd)) != G4S_OK || P->mask.alloc(sizeof(unsigned) * (size_t)rows) != G4S_OK || fail.alloc(sizeof(int)) != G4S_OK) {
        (void)hipGetLastError();                                    // no room: stay on CSR
        return G4S_OK;
    }
    hipError_t e = hipMemset(P->dia.p, 0, P->dia.bytes);
    if (e == hipSuccess) e = hipMemset(fail.p, 0, sizeof(int));
    if (e != hipSuccess) return set_error(G4S_ERR_HIP, "diagonal form: hipMemset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(dia_fill_kernel, dim3((rows + 255) / 256), dim3(256), 0, nullptr, rows, nd, P->offs, P->ld, d_rowptr, d_colids, d_values, P->dia.as<double>(),
                       P->mask.as<unsigned>(), fail.as<int>());
    int h_fail = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(&h_fail, fail.p, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_error(G4S_ERR_HIP, "diagonal fill failed: %s", hipGetErrorString(e));
    if (!h_fail) *out = P.release();
    return G4S_OK;
}

int dia_update_values(DiaPlan *P, const double *d_values, hipStream_t s)
{
    const dim3 grid((P->rows + 255) / 256), block(256);
    if (P->nd <= 8) hipLaunchKernelGGL(dia_refill_kernel<8>, grid, block, 0, s, P->rows, P->nd, P->ld, P->d_rowptr, P->mask.as<unsigned>(), d_values, P->dia.as<double>());
    else if (P->nd <= 16) hipLaunchKernelGGL(dia_refill_kernel<16>, grid, block, 0, s, P->rows, P->nd, P->ld, P->d_rowptr, P->mask.as<unsigned>(), d_values, P->dia.as<double>());
    else hipLaunchKernelGGL(dia_refill_kernel<32>, grid, block, 0, s, P->rows, P->nd, P->ld, P->d_rowptr, P->mask.as<unsigned>(), d_values, P->dia.as<double>());
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

void dia_destroy(DiaPlan *P) { delete P; }
long long dia_bytes(const DiaPlan *P) { return P ? (long long)(P->dia.bytes + P->mask.bytes) : 0; }

template <class S>
static int dia_launch(DiaPlan *P, const double *x, double *y, double alpha, double beta, hipStream_t s)
{
    // two rows per lane where it applies (≤ 16 diagonals, y 16-byte aligned): the even part of the rows; an odd last row by the one-row kernel
    const bool two = P->nd <= 16 && (reinterpret_cast<uintptr_t>(y) & 15u) == 0 && P->rows >= 2;
    const int rows2 = two ? (P->rows & ~1) : 0;
    const double *dia = P->dia.as<double>();
    const unsigned *mask = P->mask.as<unsigned>();
    if (rows2) {
        const int nblocks = (rows2 / 2 + WG - 1) / WG, per_xcd = (nblocks + kXcds - 1) / kXcds;
        const dim3 grid((unsigned)(per_xcd * kXcds));
        if (P->nd <= 8) launch_pair(P->use_nt, spmv_dia2_kernel<8, true, S>, spmv_dia2_kernel<8, false, S>, grid, s, rows2, P->cols, P->nd, P->offs, P->ld, dia, mask, x, y, alpha, beta, per_xcd);
        else launch_pair(P->use_nt, spmv_dia2_kernel<16, true, S>, spmv_dia2_kernel<16, false, S>, grid, s, rows2, P->cols, P->nd, P->offs, P->ld, dia, mask, x, y, alpha, beta, per_xcd);
    }
    const int tail0 = rows2;                                       // rows [tail0, rows) by the one-row kernel: all of them, or the odd last one
    if (tail0 < P->rows) {
        const int n_tail = P->rows - tail0;
        const int nblocks = (n_tail + WG - 1) / WG, per_xcd = (nblocks + kXcds - 1) / kXcds;
        const dim3 grid((unsigned)(per_xcd * kXcds));
        if (P->nd <= 8) launch_pair(P->use_nt, spmv_dia_kernel<8, true, S>, spmv_dia_kernel<8, false, S>, grid, s, P->rows, P->cols, P->nd, P->offs, P->ld, dia, mask, x, y, alpha, beta, per_xcd, tail0);
        else if (P->nd <= 16) launch_pair(P->use_nt, spmv_dia_kernel<16, true, S>, spmv_dia_kernel<16, false, S>, grid, s, P->rows, P->cols, P->nd, P->offs, P->ld, dia, mask, x, y, alpha, beta, per_xcd, tail0);
        else launch_pair(P->use_nt, spmv_dia_kernel<32, true, S>, spmv_dia_kernel<32, false, S>, grid, s, P->rows, P->cols, P->nd, P->offs, P->ld, dia, mask, x, y, alpha, beta, per_xcd, tail0);
    }
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

int dia_spmv(DiaPlan *P, const double *x, double *y, unsigned sr_flag, double alpha, double beta, hipStream_t s)
{
    return semiring::dispatch(sr_flag, [&](auto policy) { return dia_launch<decltype(policy)>(P, x, y, alpha, beta, s); });
}

} // namespace g4s
