// g4s/csr.hpp — header-only C++ host side over the C-ABI (include/g4s.h), keeping the reference's spelling:
//   CSR<IT,NT>                         mm/inc/CSR.h:22-113   (rows, cols, nnz, rowptr, colids, values, zerobased; owns its arrays)
//   HashSpGEMM<vectorProbing,sortOutput>(a,b,c,multop,addop)   mm/inc/hash_mult.h:1028-1057, short forms :1103-1113
//   mkl(a,b,c,timing)                  mm/inc/mkl_mult.h:113-124 (the call the shipped benchmark times)
//   Timings                            mm/inc/Timings.h:4-23, mm/src/Timings.cpp:36-65
//   SpMV(a,x,y,alpha,beta)             the CSR mat-vec this build defines for mv/ 
//   SpMVSemiring(a,x,y,multop,addop)   the same over min-plus, max-plus or or-and (y := A ⊗ x, or y ⊕ (A ⊗ x))
//   MaskedSpGEMM(a,b,mask,c,multop,addop)   C⟨M⟩ = A ⊗ B at the positions of the pattern `mask` only; TriangleCount(a): Σ (L·L⟨L⟩) of the lower triangle
//   ConnectedComponents(a,labels,symmetric)   labels[v] = the smallest vertex id of v's weakly connected component (every stored entry an edge)
//   StronglyConnectedComponents(a,labels)  labels[v] = the smallest vertex id of v's strongly connected component of the directed pattern `a` (g4s_strongly_connected_components)
//   MinimumSpanningForest(a,edges,labels), MaximumSpanningForest(…)   the positions of the entries of the minimum / maximum spanning forest of the weighted undirected graph `a` (g4s_minimum_spanning_forest)
//   KCore(a,core,round,max_k)        core[v] = v's core number in the symmetric pattern `a`, round[v] = the peel frontier that removed it (g4s_kcore)
//   TriangularSolve(a,lower,unit)    an RAII plan of the level-scheduled solve T x = b on the lower / upper triangle of `a`: solve (a vector or a block of k), update_values (g4s_sptrsv_*)
//   ILU0<IT,NT>(a)                   an RAII handle of the ILU(0) factorisation of `a` (canonical rows): apply z = U⁻¹ L⁻¹ r (a vector or a block of k), factor, factors (g4s_ilu0_*)
//   KTruss(a,truss,round,support,max_k)   per stored entry: the truss number of its edge in the symmetric pattern `a`, the peel frontier that removed it, its triangles (g4s_ktruss)
//   GreedyColor(a,color,key,seed,round), MaximalIndependentSet(a,in_set,key,seed)   first-fit colouring in decreasing priority (key, hash), and its colour class 0 (g4s_color)
//   Transpose(a,at)                  Aᵀ as a CSR, stable (the role of CSR(const CSC&, bool transpose), mm/inc/CSR.h:171-230, and mm/inc/convert.h)
//   EWiseAdd / EWiseMult / EWiseDifference(a,b,c), Select(a,c,pred,k,thr), Symmetrise(a,c)   A ∪ B, A ∩ B, A ∖ B, a filter, A ∪ Aᵀ (g4s_csr_ewise_*, g4s_csr_select_*)
//   graph, FromGraph(g,c,dup), FromCOO(…), ToCOO(a,row_out), SortAndMerge(a,c,dup)   an edge list to a CSR with repeats merged and back (CSR(graph&), mm/inc/CSR.h:255-329)
//   Extract(a,ri,ci), SpRef / SpRef2, Permute(a,perm), SubMatrix(a,M_,N_,M_start,N_start)   A[I, J] for id lists in any order, with repeats (CSC::SpRef, mm/inc/CSC.h:513-690; the block constructor, mm/inc/CSR.h:691-733)
// Only IT = int32_t, NT = double exist in the reference (mm/inc/define.h:14-15) and on the device. Arrays handed back by the
// library are allocated with g4s_malloc and released with g4s_free (the my_malloc/my_free pairing of mm/inc/utility.h:126-153).
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>
#include "../g4s.h"

namespace g4s {

inline void check(g4s_status st, const char *what)
{
    if (st != G4S_OK) throw std::runtime_error(std::string(what) + ": " + g4s_last_error());
}

struct Timings : g4s_timings {
    Timings() { reset(); }
    void reset() { create = spmm = convert = order = export_csr = destroy = total = 0.0; }
    void operator+=(const Timings &b)
    {
        create += b.create; spmm += b.spmm; convert += b.convert; order += b.order;
        export_csr += b.export_csr; destroy += b.destroy; total += b.total;
    }
    void operator/=(double x)
    {
        create /= x; spmm /= x; convert /= x; order /= x; export_csr /= x; destroy /= x; total /= x;
    }
    // Timings::print, byte for byte (mm/src/Timings.cpp:36-60). The reference keeps seconds and prints 1000·t; g4s_timings holds
    // milliseconds, so t below is field/1000. Called with total_flop = 2·flop (mm/src/mkl_spgemm.cpp:82). Percentages are of `total`,
    // the wall time around the whole call, not of the sum of the stages; perf lines divide flop/1e9 by seconds (inf for a zero stage,
    // as in the reference).
    bool measure_separate = true, measure_total = true;   // mm/inc/Timings.h:6-7
    void print(double total_flop) const
    {
        const double total_flop_G = total_flop / 1000000000;
        std::printf("total flop %lf\n", total_flop);
        const double c = create / 1000, s = spmm / 1000, v = convert / 1000, o = order / 1000, e = export_csr / 1000, d = destroy / 1000, t = total / 1000;
        const double sum_total = c + s + v + o + e + d;
        if (measure_separate) {
            std::printf("time(ms):\n");
            std::printf("    create             %8.3lfms %6.2lf%%\n", 1000 * c, c / t * 100);
            std::printf("    spmm               %8.3lfms %6.2lf%%\n", 1000 * s, s / t * 100);
            std::printf("    convert            %8.3lfms %6.2lf%%\n", 1000 * v, v / t * 100);
            std::printf("    order              %8.3lfms %6.2lf%%\n", 1000 * o, o / t * 100);
            std::printf("    export_csr         %8.3lfms %6.2lf%%\n", 1000 * e, e / t * 100);
            std::printf("    destroy            %8.3lfms %6.2lf%%\n", 1000 * d, d / t * 100);
            std::printf("    sum_total          %8.3lfms %6.2lf%%\n", 1000 * sum_total, sum_total / t * 100);
            std::printf("perf(Gflops):\n");
            std::printf("    create             %6.2lf\n", total_flop_G / c);
            std::printf("    spmm               %6.2lf\n", total_flop_G / s);
            std::printf("    convert            %6.2lf\n", total_flop_G / v);
            std::printf("    order              %6.2lf\n", total_flop_G / o);
            std::printf("    export_csr         %6.2lf\n", total_flop_G / e);
            std::printf("    destroy            %6.2lf\n", total_flop_G / d);
            std::printf("    total              %6.2lf\n", total_flop_G / t);
        }
    }
    void reg_print(double total_flop) const                // mm/src/Timings.cpp:62-65
    {
        const double total_flop_G = total_flop / 1000000000;
        std::printf("%le\n", total_flop_G / (total / 1000));
    }
};

template <class IT = int32_t, class NT = double>
class CSR {
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the reference and the device use int32 / fp64 only");
public:
    CSR() : rows(0), cols(0), nnz(0), rowptr(nullptr), colids(nullptr), values(nullptr), zerobased(true) {}
    // raw-array constructor: copies, like mm/inc/CSR.h:102-113
    CSR(const IT *rp, const IT *ci, const NT *va, IT M, IT N, IT nz) : rows(M), cols(N), nnz(nz), zerobased(true)
    {
        rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)M + 1));
        colids = (IT *)g4s_malloc(sizeof(IT) * (size_t)nz);
        values = (NT *)g4s_malloc(sizeof(NT) * (size_t)nz);
        std::memcpy(rowptr, rp, sizeof(IT) * ((size_t)M + 1));
        std::memcpy(colids, ci, sizeof(IT) * (size_t)nz);
        std::memcpy(values, va, sizeof(NT) * (size_t)nz);
    }
    CSR(const CSR &o) : CSR(o.rowptr, o.colids, o.values, o.rows, o.cols, o.nnz) {}
    CSR &operator=(const CSR &o) { if (this != &o) { CSR t(o); swap(t); } return *this; }
    CSR(CSR &&o) noexcept : CSR() { swap(o); }
    CSR &operator=(CSR &&o) noexcept { swap(o); return *this; }
    ~CSR() { make_empty(); }
    void make_empty()                                   // mm/inc/CSR.h:50-62
    {
        g4s_free(rowptr); g4s_free(colids); g4s_free(values);
        rowptr = colids = nullptr; values = nullptr; rows = cols = nnz = 0;
    }
    void swap(CSR &o) noexcept
    {
        std::swap(rows, o.rows); std::swap(cols, o.cols); std::swap(nnz, o.nnz); std::swap(rowptr, o.rowptr);
        std::swap(colids, o.colids); std::swap(values, o.values); std::swap(zerobased, o.zerobased);
    }
    IT rows, cols, nnz;
    IT *rowptr, *colids;
    NT *values;
    bool zerobased;
};

// The add operations of the tropical semirings, as ordinary callables (they keep their meaning in host code).
template <class NT>
struct min_op {
    NT operator()(const NT &x, const NT &y) const { return y < x ? y : x; }
};
template <class NT>
struct max_op {
    NT operator()(const NT &x, const NT &y) const { return x < y ? y : x; }
};

// (multiply, add) functor pair → the device semiring flag (include/g4s.h, G4S_SEMIRING_*). Only these four pairs exist on the device.
template <class Mul, class Add, class NT>
struct semiring_flag { static constexpr bool supported = false; };
template <class NT>
struct semiring_flag<std::multiplies<NT>, std::plus<NT>, NT> { static constexpr bool supported = true; static constexpr unsigned value = G4S_SEMIRING_PLUS_TIMES; };
template <class NT>
struct semiring_flag<std::plus<NT>, min_op<NT>, NT> { static constexpr bool supported = true; static constexpr unsigned value = G4S_SEMIRING_MIN_PLUS; };
template <class NT>
struct semiring_flag<std::plus<NT>, max_op<NT>, NT> { static constexpr bool supported = true; static constexpr unsigned value = G4S_SEMIRING_MAX_PLUS; };
template <class NT>
struct semiring_flag<std::logical_and<NT>, std::logical_or<NT>, NT> { static constexpr bool supported = true; static constexpr unsigned value = G4S_SEMIRING_OR_AND; };

// C = A·B on the device, result adopted by `c`. The (multop, addop) pair must be one of the four device semirings (semiring_flag); any other
// functor is refused at compile time — there is no host loop.
template <bool vectorProbing = false, bool sortOutput = true, typename IT, typename NT, typename Mul, typename Add>
void HashSpGEMM(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, Mul, Add, Timings *timing = nullptr)
{
    static_assert(semiring_flag<Mul, Add, NT>::supported,
                  "device SpGEMM implements four (multop, addop) pairs only: (std::multiplies, std::plus), (std::plus, g4s::min_op), "
                  "(std::plus, g4s::max_op), (std::logical_and, std::logical_or)");
    c.make_empty();
    int64_t cnnz = 0;
    check(g4s_spgemm_csr_i32_f64(a.rowptr, a.colids, a.values, b.rowptr, b.colids, b.values, &c.rowptr, &c.colids, &c.values,
                                 a.rows, a.cols, b.cols, &cnnz, timing, (sortOutput ? G4S_SORT_OUTPUT : 0u) | semiring_flag<Mul, Add, NT>::value),
          "HashSpGEMM");
    c.rows = a.rows; c.cols = b.cols; c.nnz = (IT)cnnz; c.zerobased = true;
}
template <typename IT, typename NT>
void HashSpGEMM(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c) { HashSpGEMM<false, true>(a, b, c, std::multiplies<NT>(), std::plus<NT>()); }

// c = the product A ⊗ B at the positions of mask's pattern only (g4s_spgemm_masked, host arrays): c receives a copy of the mask's pattern and the new
// values — the full product's value where it has an entry, the semiring's identity elsewhere. mask's rows must be strictly ascending; its values are
// not read. The functor pair is checked like HashSpGEMM's. c must not be a, b or mask.
template <typename IT, typename NT, typename Mul, typename Add>
void MaskedSpGEMM(const CSR<IT, NT> &a, const CSR<IT, NT> &b, const CSR<IT, NT> &mask, CSR<IT, NT> &c, Mul, Add, g4s_masked_info *info = nullptr)
{
    static_assert(semiring_flag<Mul, Add, NT>::supported,
                  "device SpGEMM implements four (multop, addop) pairs only: (std::multiplies, std::plus), (std::plus, g4s::min_op), "
                  "(std::plus, g4s::max_op), (std::logical_and, std::logical_or)");
    c.make_empty();
    c.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)mask.rows + 1));
    c.colids = (IT *)g4s_malloc(sizeof(IT) * ((size_t)mask.nnz + 1));
    c.values = (NT *)g4s_malloc(sizeof(NT) * ((size_t)mask.nnz + 1));
    if (!c.rowptr || !c.colids || !c.values) { c.make_empty(); throw std::runtime_error("MaskedSpGEMM: host allocation failed"); }
    if (mask.rowptr) std::memcpy(c.rowptr, mask.rowptr, sizeof(IT) * ((size_t)mask.rows + 1));
    else c.rowptr[0] = 0;
    if (mask.nnz) std::memcpy(c.colids, mask.colids, sizeof(IT) * (size_t)mask.nnz);
    c.rows = a.rows; c.cols = b.cols; c.nnz = mask.nnz; c.zerobased = true;
    check(g4s_spgemm_masked(a.rows, a.cols, b.cols, a.rowptr, a.colids, a.values, b.rowptr, b.colids, b.values, c.rowptr, c.colids, c.values,
                            G4S_HOST_POINTERS | semiring_flag<Mul, Add, NT>::value, info, nullptr), "MaskedSpGEMM");
}
template <typename IT, typename NT>
void MaskedSpGEMM(const CSR<IT, NT> &a, const CSR<IT, NT> &b, const CSR<IT, NT> &mask, CSR<IT, NT> &c) { MaskedSpGEMM(a, b, mask, c, std::multiplies<NT>(), std::plus<NT>()); }

// The triangles of the graph whose symmetric pattern (or lower triangle alone) `a` stores, rows strictly ascending (g4s_triangle_count, host arrays).
template <typename IT, typename NT>
int64_t TriangleCount(const CSR<IT, NT> &a, g4s_masked_info *info = nullptr)
{
    int64_t count = 0;
    check(g4s_triangle_count(a.rows, a.rowptr, a.colids, &count, G4S_HOST_POINTERS, info, nullptr), "TriangleCount");
    return count;
}

// labels[v] (a.rows values) = the smallest vertex id in v's weakly connected component of the square pattern `a` — every stored entry an undirected
// edge, whatever its value (g4s_connected_components, host arrays). symmetric: the caller declares the pattern symmetric (G4S_CC_SYMMETRIC).
template <typename IT, typename NT>
void ConnectedComponents(const CSR<IT, NT> &a, int32_t *labels, bool symmetric = false, g4s_cc_info *info = nullptr)
{
    if (a.rows != a.cols) throw std::runtime_error("ConnectedComponents: the pattern is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    int32_t none = 0;
    check(g4s_connected_components(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, a.rows ? labels : &none,
                                   G4S_HOST_POINTERS | (symmetric ? G4S_CC_SYMMETRIC : 0u), info, nullptr), "ConnectedComponents");
}

// labels[v] (a.rows values) = the smallest vertex id in v's STRONGLY connected component of the square pattern `a` — every stored entry (u, v) a directed
// edge u → v, whatever its value (g4s_strongly_connected_components, host arrays; the call builds the transpose it needs).
template <typename IT, typename NT>
void StronglyConnectedComponents(const CSR<IT, NT> &a, int32_t *labels, g4s_scc_info *info = nullptr)
{
    if (a.rows != a.cols) throw std::runtime_error("StronglyConnectedComponents: the pattern is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    int32_t none = 0;
    check(g4s_strongly_connected_components(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, nullptr, nullptr, a.rows ? labels : &none, G4S_HOST_POINTERS, info,
                                            nullptr), "StronglyConnectedComponents");
}

// edges[0 … info->edges) = the ascending positions, in a.colids / a.values, of the entries of the minimum spanning forest of the undirected graph whose
// edges are the stored off-diagonal entries of the square matrix `a`, weights = values, under the strict order (w, min, max, position) — the forest
// Kruskal builds in that order (g4s_minimum_spanning_forest, host arrays). edges has room for max(a.rows − 1, 0) values. labels (a.rows values, may be
// NULL): the canonical component labels. weighted = false reads no values: all weights equal, a spanning forest. Returns the number of positions.
// MaximumSpanningForest is the same call with G4S_MSF_MAXIMUM: only the weight is reversed.
template <typename IT, typename NT>
int64_t MinimumSpanningForest(const CSR<IT, NT> &a, int32_t *edges, int32_t *labels = nullptr, g4s_msf_info *info = nullptr, bool weighted = true, unsigned flags = 0u)
{
    if (a.rows != a.cols) throw std::runtime_error("MinimumSpanningForest: the matrix is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    g4s_msf_info mine = {};
    check(g4s_minimum_spanning_forest(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, weighted ? a.values : nullptr, edges, a.rows ? labels : nullptr,
                                      G4S_HOST_POINTERS | flags, &mine, nullptr), "MinimumSpanningForest");
    if (info) *info = mine;
    return mine.edges;
}

template <typename IT, typename NT>
int64_t MaximumSpanningForest(const CSR<IT, NT> &a, int32_t *edges, int32_t *labels = nullptr, g4s_msf_info *info = nullptr, bool weighted = true)
{
    return MinimumSpanningForest(a, edges, labels, info, weighted, G4S_MSF_MAXIMUM);
}

// core[v] (a.rows values) = the largest k such that v belongs to a subgraph of the simple undirected graph `a` in which every vertex has at least k
// neighbours (g4s_kcore, host arrays): `a` holds the graph's symmetric pattern with ascending rows (Symmetrise gives one), a stored diagonal entry is
// ignored. round (may be NULL): the index of the peel frontier that removed v; sorted by (round, id) the vertices are in a degeneracy ordering. max_k:
// only the levels below it are peeled, what is left gets core = max_k and round = −1 (info->capped).
template <typename IT, typename NT>
void KCore(const CSR<IT, NT> &a, int32_t *core, int32_t *round = nullptr, int32_t max_k = INT32_MAX, g4s_kcore_info *info = nullptr)
{
    if (a.rows != a.cols) throw std::runtime_error("KCore: the pattern is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    int32_t none = 0;
    check(g4s_kcore(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, max_k, a.rows ? core : &none, a.rows ? round : nullptr, G4S_HOST_POINTERS, info, nullptr),
          "KCore");
}

// A device allocation that lives for one call: the block a host-side block solve or apply copies through.
struct DeviceBlock {
    void *p = nullptr;
    DeviceBlock(size_t bytes, const char *what) { check(g4s_dev_alloc(&p, bytes), what); }
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { (void)g4s_dev_free(p); }
};

// The plan of the solve T x = b with the lower (lower = false: upper) triangle T of the square matrix `a` (g4s_sptrsv_analyse): only the entries of
// that triangle are read, so the (D + L) of a general matrix is solved from the matrix itself. The plan keeps its own copy of the triangle on the
// device; `a` need not outlive the constructor. unit_diagonal: stored diagonal entries are ignored; without it a row that stores none throws.
// level (may be NULL): a.rows ints, the depth of every row in the dependency DAG. solve(b, x): host arrays of a.rows doubles, x may be b; copied
// through a device buffer of the plan, synchronous. solve_device: device arrays, enqueued on `stream`, asynchronous. update_values: new values in
// the layout of a.values, all a.nnz of them. solve(B, X, k): host blocks of a.rows × k, row-major with ld = k, X may be B, all k columns on the launches
// of one solve, synchronous. solve_device_multi: device blocks with their leading dimensions and G4S_TRSV_COL_MAJOR or 0 (g4s_sptrsv_solve_multi).
class TriangularSolve {
public:
    template <typename IT, typename NT>
    explicit TriangularSolve(const CSR<IT, NT> &a, bool lower = true, bool unit_diagonal = false, int32_t *level = nullptr) : n_(a.rows)
    {
        if (a.rows != a.cols) throw std::runtime_error("TriangularSolve: the matrix is not square");
        const unsigned flags = G4S_HOST_POINTERS | (lower ? 0u : G4S_TRSV_UPPER) | (unit_diagonal ? G4S_TRSV_UNIT_DIAGONAL : 0u);
        const IT zero = 0;                                  // an empty CSR holds no arrays: nothing is read for rows == 0 or nnz == 0
        const NT none = 0;
        check(g4s_sptrsv_analyse(&plan_, a.rows, a.rowptr ? a.rowptr : &zero, a.nnz ? a.colids : &zero, a.nnz ? a.values : &none, level, flags, &info_, nullptr),
              "TriangularSolve");
    }
    TriangularSolve(const TriangularSolve &) = delete;
    TriangularSolve &operator=(const TriangularSolve &) = delete;
    TriangularSolve(TriangularSolve &&o) noexcept : plan_(o.plan_), buf_(o.buf_), n_(o.n_), info_(o.info_) { o.plan_ = nullptr; o.buf_ = nullptr; }
    ~TriangularSolve()
    {
        if (buf_) (void)g4s_dev_free(buf_);
        if (plan_) (void)g4s_sptrsv_destroy(plan_);
    }
    void solve(const double *b, double *x)
    {
        if (n_ == 0) return;
        if (!buf_) check(g4s_dev_alloc(&buf_, sizeof(double) * (size_t)n_), "TriangularSolve::solve");
        check(g4s_memcpy_h2d(buf_, b, sizeof(double) * (size_t)n_), "TriangularSolve::solve");
        solve_device(static_cast<const double *>(buf_), static_cast<double *>(buf_));
        check(g4s_device_synchronize(), "TriangularSolve::solve");
        check(g4s_memcpy_d2h(x, buf_, sizeof(double) * (size_t)n_), "TriangularSolve::solve");
    }
    void solve_device(const double *b_dev, double *x_dev, void *stream = nullptr) { check(g4s_sptrsv_solve(plan_, b_dev, x_dev, stream), "TriangularSolve::solve"); }
    void solve(const double *B, double *X, int k)           // n × k host blocks, row-major with ld = k
    {
        if (k < 0 || k > G4S_TRSV_MAX_RHS) throw std::runtime_error("TriangularSolve::solve: k is negative or above G4S_TRSV_MAX_RHS");
        if (n_ == 0 || k == 0) return;
        const size_t bytes = sizeof(double) * (size_t)n_ * (size_t)k;
        DeviceBlock blk(bytes, "TriangularSolve::solve");
        check(g4s_memcpy_h2d(blk.p, B, bytes), "TriangularSolve::solve");
        solve_device_multi(k, static_cast<const double *>(blk.p), k, static_cast<double *>(blk.p), k);
        check(g4s_device_synchronize(), "TriangularSolve::solve");
        check(g4s_memcpy_d2h(X, blk.p, bytes), "TriangularSolve::solve");
    }
    void solve_device_multi(int32_t k, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx, unsigned flags = 0, void *stream = nullptr)
    {
        check(g4s_sptrsv_solve_multi(plan_, k, B_dev, ldb, X_dev, ldx, flags, stream), "TriangularSolve::solve");
    }
    void update_values(const double *values) { check(g4s_sptrsv_update_values(plan_, values, G4S_HOST_POINTERS, nullptr), "TriangularSolve::update_values"); }
    const g4s_trsv_info &info() const { return info_; }

private:
    g4s_trsv_t plan_ = nullptr;
    void *buf_ = nullptr;
    int32_t n_;
    g4s_trsv_info info_ = {};
};

// The ILU(0) factorisation of the square matrix `a` (g4s_ilu0_analyse): a ≈ L U on a's own pattern. The rows of `a` must be canonical — columns
// strictly ascending, every diagonal entry stored (SortAndMerge gives such rows) —, anything else throws. The handle keeps its own copy on the
// device; `a` need not outlive the constructor. apply(r, z): z = U⁻¹ (L⁻¹ r), host arrays of a.rows doubles, z may be r; copied through a device
// buffer of the object, synchronous. apply_device: device arrays, enqueued on `stream`, asynchronous. factor(values): refactorise with new values
// in the layout of a.values (all a.nnz of them; NULL: the values held); returns the smallest row whose pivot is zero or not finite, −1 when there
// is none — which is no error. factors(out): a.nnz values in the layout of a.values, L strictly below the diagonal, U on and above it.
// apply(R, Z, k) and apply_device_multi: the apply of a block of a.rows × k vectors, as TriangularSolve's block solve (g4s_ilu0_apply_multi).
template <typename IT, typename NT>
class ILU0 {
public:
    explicit ILU0(const CSR<IT, NT> &a) : n_(a.rows)
    {
        if (a.rows != a.cols) throw std::runtime_error("ILU0: the matrix is not square");
        const IT zero = 0;                                  // an empty CSR holds no arrays: nothing is read for rows == 0 or nnz == 0
        const NT none = 0;
        check(g4s_ilu0_analyse(&h_, a.rows, a.rowptr ? a.rowptr : &zero, a.nnz ? a.colids : &zero, a.nnz ? a.values : &none, G4S_HOST_POINTERS, &info_, nullptr),
              "ILU0");
    }
    ILU0(const ILU0 &) = delete;
    ILU0 &operator=(const ILU0 &) = delete;
    ILU0(ILU0 &&o) noexcept : h_(o.h_), buf_(o.buf_), n_(o.n_), info_(o.info_) { o.h_ = nullptr; o.buf_ = nullptr; }
    ~ILU0()
    {
        if (buf_) (void)g4s_dev_free(buf_);
        if (h_) (void)g4s_ilu0_destroy(h_);
    }
    void apply(const double *r, double *z)
    {
        if (n_ == 0) return;
        double *buf = buffer("ILU0::apply");
        check(g4s_memcpy_h2d(buf, r, sizeof(double) * (size_t)n_), "ILU0::apply");
        apply_device(buf, buf);
        check(g4s_device_synchronize(), "ILU0::apply");
        check(g4s_memcpy_d2h(z, buf, sizeof(double) * (size_t)n_), "ILU0::apply");
    }
    void apply_device(const double *r_dev, double *z_dev, void *stream = nullptr) { check(g4s_ilu0_apply(h_, r_dev, z_dev, stream), "ILU0::apply"); }
    void apply(const double *R, double *Z, int k)           // n × k host blocks, row-major with ld = k
    {
        if (k < 0 || k > G4S_TRSV_MAX_RHS) throw std::runtime_error("ILU0::apply: k is negative or above G4S_TRSV_MAX_RHS");
        if (n_ == 0 || k == 0) return;
        const size_t bytes = sizeof(double) * (size_t)n_ * (size_t)k;
        DeviceBlock blk(bytes, "ILU0::apply");
        check(g4s_memcpy_h2d(blk.p, R, bytes), "ILU0::apply");
        apply_device_multi(k, static_cast<const double *>(blk.p), k, static_cast<double *>(blk.p), k);
        check(g4s_device_synchronize(), "ILU0::apply");
        check(g4s_memcpy_d2h(Z, blk.p, bytes), "ILU0::apply");
    }
    void apply_device_multi(int32_t k, const double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, unsigned flags = 0, void *stream = nullptr)
    {
        check(g4s_ilu0_apply_multi(h_, k, R_dev, ldr, Z_dev, ldz, flags, stream), "ILU0::apply");
    }
    int32_t factor(const double *values = nullptr)
    {
        if (n_ == 0) return -1;
        int32_t bad = -1;
        int32_t *word = reinterpret_cast<int32_t *>(buffer("ILU0::factor") + n_);
        check(g4s_ilu0_factor(h_, values, G4S_HOST_POINTERS, word, nullptr), "ILU0::factor");
        check(g4s_device_synchronize(), "ILU0::factor");
        check(g4s_memcpy_d2h(&bad, word, sizeof(bad)), "ILU0::factor");
        return bad;
    }
    void factors(double *out) { check(g4s_ilu0_get_factors(h_, out, G4S_HOST_POINTERS, nullptr), "ILU0::factors"); }
    const g4s_ilu0_info &info() const { return info_; }

private:
    double *buffer(const char *what)                        // n doubles for r / z and, behind them, the pivot word
    {
        if (!buf_) check(g4s_dev_alloc(&buf_, sizeof(double) * ((size_t)n_ + 1)), what);
        return static_cast<double *>(buf_);
    }
    g4s_ilu0_t h_ = nullptr;
    void *buf_ = nullptr;
    int32_t n_;
    g4s_ilu0_info info_ = {};
};

// truss[p] (a.nnz values, one per stored entry) = the largest k such that the edge stored at entry p belongs to a subgraph of the simple undirected graph
// `a` in which every edge lies in at least k − 2 triangles (g4s_ktruss, host arrays): `a` holds the graph's symmetric pattern with ascending rows
// (Symmetrise gives one); both copies of an edge get the same values, a stored diagonal entry gets truss 0, round −1, support 0. round (may be NULL): the
// index of the peel frontier that removed the edge. support (may be NULL): the triangles through the edge in `a`. max_k (>= 2): only the levels below it
// are peeled, what is left — the max_k-truss — gets truss = max_k and round = −1 (info->capped).
template <typename IT, typename NT>
void KTruss(const CSR<IT, NT> &a, int32_t *truss, int32_t *round = nullptr, int32_t *support = nullptr, int32_t max_k = INT32_MAX, g4s_ktruss_info *info = nullptr)
{
    if (a.rows != a.cols) throw std::runtime_error("KTruss: the pattern is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    int32_t none = 0;
    check(g4s_ktruss(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, max_k, a.rows ? truss : &none, a.rows ? round : nullptr, a.rows ? support : nullptr,
                     G4S_HOST_POINTERS, info, nullptr), "KTruss");
}

// color[v] (a.rows values) = the first-fit colour of v in the simple undirected graph `a`: the smallest colour not held by a neighbour of higher
// priority, the priority being the pair (key[v], fmix32(v ^ seed)), larger first (g4s_color, host arrays). `a` holds the graph's symmetric pattern
// with ascending rows (Symmetrise gives one), a stored diagonal entry is ignored. key (may be NULL: a pure hash order): the round of KCore gives
// smallest-last, at most degeneracy + 1 colours; largest_first takes the degree as the key (key must then be NULL). round (may be NULL): the depth
// of v in the priority DAG.
template <typename IT, typename NT>
void GreedyColor(const CSR<IT, NT> &a, int32_t *color, const int32_t *key = nullptr, uint32_t seed = 0, int32_t *round = nullptr, bool largest_first = false,
                 g4s_color_info *info = nullptr)
{
    if (a.rows != a.cols) throw std::runtime_error("GreedyColor: the pattern is not square");
    const IT zero = 0;                                      // an empty CSR holds no arrays: nothing is read or written for rows == 0
    int32_t none = 0;
    check(g4s_color(a.rows, a.rowptr ? a.rowptr : &zero, a.colids, a.rows ? key : nullptr, seed, a.rows ? color : &none, a.rows ? round : nullptr,
                    G4S_HOST_POINTERS | (largest_first ? G4S_COLOR_LARGEST_FIRST : 0u), info, nullptr), "GreedyColor");
}

// in_set[v] = 1 for the vertices of the greedy maximal independent set in priority order — colour class 0 of GreedyColor(a, …, key, seed) —, else 0.
template <typename IT, typename NT>
void MaximalIndependentSet(const CSR<IT, NT> &a, std::vector<char> &in_set, const int32_t *key = nullptr, uint32_t seed = 0)
{
    std::vector<int32_t> color((size_t)(a.rows > 0 ? a.rows : 0));
    GreedyColor(a, color.data(), key, seed);
    in_set.resize(color.size());
    for (size_t v = 0; v < color.size(); ++v) in_set[v] = color[v] == 0;
}

// The wrapper the shipped benchmark calls: mkl(A,B,C,timing) (mm/inc/mkl_mult.h:113-124 ← mm/src/mkl_spgemm.cpp:67,74).
template <typename IT, typename NT>
void mkl(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, Timings &timing) { HashSpGEMM<false, true>(a, b, c, std::multiplies<NT>(), std::plus<NT>(), &timing); }

template <typename IT, typename NT>
long long get_flop(const CSR<IT, NT> &a, const CSR<IT, NT> &b)   // mm/inc/hash_mult.h:46-62
{
    int64_t flop = 0;
    check(g4s_spgemm_flop(a.rows, a.rowptr, a.colids, b.rowptr, &flop, nullptr, G4S_HOST_POINTERS), "get_flop");
    return flop;
}

template <typename IT, typename NT>
void SpMV(const CSR<IT, NT> &a, const NT *x, NT *y, NT alpha = 1.0, NT beta = 0.0)
{
    check(g4s_spmv_csr_i32_f64(a.rows, a.cols, a.rowptr, a.colids, a.values, x, y, alpha, beta, G4S_HOST_POINTERS), "SpMV");
}

// y := A ⊗ x, or y := y ⊕ (A ⊗ x) with accumulate, over the semiring of a (multop, addop) pair (semiring_flag: the pairs of HashSpGEMM), host arrays.
// Its own name, not an overload of SpMV: SpMV(a, x, y, alpha, beta) keeps its one meaning whatever the argument types.
template <typename IT, typename NT, typename Mul, typename Add>
void SpMVSemiring(const CSR<IT, NT> &a, const NT *x, NT *y, Mul, Add, bool accumulate = false)
{
    static_assert(semiring_flag<Mul, Add, NT>::supported,
                  "device SpMV implements four (multop, addop) pairs only: (std::multiplies, std::plus), (std::plus, g4s::min_op), "
                  "(std::plus, g4s::max_op), (std::logical_and, std::logical_or)");
    check(g4s_spmv_semiring_csr_i32_f64(a.rows, a.cols, a.rowptr, a.colids, a.values, x, y,
                                        G4S_HOST_POINTERS | semiring_flag<Mul, Add, NT>::value | (accumulate ? G4S_SPMV_ACCUMULATE : 0u)), "SpMVSemiring");
}

// at = Aᵀ (a.cols × a.rows) on the device through g4s_csr_transpose, host arrays. Stable: row j of at lists the entries of column j of a in their
// stored order (duplicates kept), so at is also the CSC form of a. at's old arrays are released first.
template <typename IT, typename NT>
void Transpose(const CSR<IT, NT> &a, CSR<IT, NT> &at)
{
    at.make_empty();
    at.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)a.cols + 1));
    at.colids = (IT *)g4s_malloc(sizeof(IT) * ((size_t)a.nnz + 1));
    at.values = (NT *)g4s_malloc(sizeof(NT) * ((size_t)a.nnz + 1));
    if (!at.rowptr || !at.colids || !at.values) { at.make_empty(); throw std::runtime_error("Transpose: host allocation failed"); }
    check(g4s_csr_transpose(a.rows, a.cols, a.nnz, a.rowptr, a.colids, a.values, at.rowptr, at.colids, a.values ? at.values : nullptr, nullptr, G4S_HOST_POINTERS, nullptr),
          "Transpose");
    at.rows = a.cols; at.cols = a.rows; at.nnz = a.nnz; at.zerobased = true;
}

// Element-wise combination and filtering on the device (g4s_csr_ewise_* / g4s_csr_select_*, host arrays; include/g4s.h has the contract): rows of a
// and b strictly ascending, the result's too; a stored position is an entry whatever its value. c's old arrays are released first; c must not be a or b.
//   EWiseAdd(a, b, c, combine)     every position of a or b; combine (G4S_COMBINE_*, default PLUS) where both store it, a copy elsewhere
//   EWiseMult(a, b, c, combine)    the positions both store (default TIMES)
//   EWiseDifference(a, b, c)       the entries of a whose position b does not store
//   Select(a, c, pred, k, thr)     the entries of a that satisfy G4S_SELECT_* pred, in stored order (rows in any order)
//   Symmetrise(a, c, combine, drop_diagonal)   a ∪ aᵀ of a square matrix (default MAX), optionally without its diagonal
namespace detail {
template <typename IT, typename NT>
void adopt(CSR<IT, NT> &c, IT rows, IT cols, int64_t nnz, const char *what)
{
    c.colids = (IT *)g4s_malloc(sizeof(IT) * ((size_t)nnz + 1));
    c.values = (NT *)g4s_malloc(sizeof(NT) * ((size_t)nnz + 1));
    if (!c.colids || !c.values) { c.make_empty(); throw std::runtime_error(std::string(what) + ": host allocation failed"); }
    c.rows = rows; c.cols = cols; c.nnz = (IT)nnz; c.zerobased = true;
}
template <typename IT, typename NT>
void ewise(int op, int combine, const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, g4s_ewise_info *info, const char *what)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device works on CSR<int32_t, double>");
    if (a.rows != b.rows || a.cols != b.cols) throw std::runtime_error(std::string(what) + ": the shapes differ");
    c.make_empty();
    const IT zero = 0;                                      // an empty CSR holds no arrays
    const IT *arp = a.rowptr ? a.rowptr : &zero, *brp = b.rowptr ? b.rowptr : &zero;
    const IT rows = a.rowptr && b.rowptr ? a.rows : 0;
    c.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)a.rows + 1));
    if (!c.rowptr) throw std::runtime_error(std::string(what) + ": host allocation failed");
    int64_t cnnz = 0;
    g4s_status st = g4s_csr_ewise_symbolic(op, rows, a.cols, arp, a.colids, brp, b.colids, c.rowptr, &cnnz, G4S_HOST_POINTERS, info, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, what); }
    for (IT r = rows; r < a.rows; ++r) c.rowptr[r + 1] = 0;
    adopt(c, a.rows, a.cols, cnnz, what);
    st = g4s_csr_ewise_numeric(op, combine, rows, a.cols, arp, a.colids, a.values, brp, b.colids, b.values, c.rowptr, c.colids, c.values, G4S_HOST_POINTERS, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, what); }
}
} // namespace detail
template <typename IT, typename NT>
void EWiseAdd(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, int combine = G4S_COMBINE_PLUS, g4s_ewise_info *info = nullptr)
{
    detail::ewise(G4S_EWISE_UNION, combine, a, b, c, info, "EWiseAdd");
}
template <typename IT, typename NT>
void EWiseMult(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, int combine = G4S_COMBINE_TIMES, g4s_ewise_info *info = nullptr)
{
    detail::ewise(G4S_EWISE_INTERSECT, combine, a, b, c, info, "EWiseMult");
}
template <typename IT, typename NT>
void EWiseDifference(const CSR<IT, NT> &a, const CSR<IT, NT> &b, CSR<IT, NT> &c, g4s_ewise_info *info = nullptr)
{
    detail::ewise(G4S_EWISE_DIFFERENCE, G4S_COMBINE_FIRST, a, b, c, info, "EWiseDifference");
}
template <typename IT, typename NT>
void Select(const CSR<IT, NT> &a, CSR<IT, NT> &c, int pred, int64_t k = 0, double thr = 0.0)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device works on CSR<int32_t, double>");
    c.make_empty();
    const IT zero = 0;
    const IT *rp = a.rowptr ? a.rowptr : &zero;
    const IT rows = a.rowptr ? a.rows : 0;
    c.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)a.rows + 1));
    if (!c.rowptr) throw std::runtime_error("Select: host allocation failed");
    int64_t cnnz = 0;
    g4s_status st = g4s_csr_select_symbolic(pred, k, thr, rows, a.cols, rp, a.colids, a.values, c.rowptr, &cnnz, G4S_HOST_POINTERS, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, "Select"); }
    for (IT r = rows; r < a.rows; ++r) c.rowptr[r + 1] = 0;
    detail::adopt(c, a.rows, a.cols, cnnz, "Select");
    st = g4s_csr_select_numeric(pred, k, thr, rows, a.cols, rp, a.colids, a.values, c.rowptr, c.colids, c.values, G4S_HOST_POINTERS, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, "Select"); }
}
template <typename IT, typename NT>
void Symmetrise(const CSR<IT, NT> &a, CSR<IT, NT> &c, int combine = G4S_COMBINE_MAX, bool drop_diagonal = false)
{
    if (a.rows != a.cols) throw std::runtime_error("Symmetrise: the matrix is not square");
    CSR<IT, NT> at;
    Transpose(a, at);
    if (!drop_diagonal) { EWiseAdd(a, at, c, combine); return; }
    CSR<IT, NT> u;
    EWiseAdd(a, at, u, combine);
    Select(u, c, G4S_SELECT_OFFDIAG);
}

// A CSR from an edge list on the device (g4s_csr_from_coo_symbolic / _numeric, g4s_csr_row_indices, host arrays; include/g4s.h has the contract). c's old
// arrays are released first; c must not be a.
//   graph                          the reference's edge list (mm/inc/graph.h): m edges e from start[e] to end[e] with weight w[e], n vertices; borrowed arrays
//   FromGraph(g, c, dup)           the n × n matrix of g, what CSR(graph&) builds (mm/inc/CSR.h:255-329); throws on an id that does not fit int32
//   FromCOO(rows, cols, nnz, row, col, val, c, dup)   the same from int32 triples; val may be NULL (values 1.0)
//   ToCOO(a, row_out)              the row of every stored entry of a (a.nnz values): with a.colids and a.values, a as a COO
//   SortAndMerge(a, c, dup)        a with sorted rows and merged repeats: ToCOO followed by FromCOO (CSC::MergeDuplicates, mm/inc/CSC.h:297-342)
// dup is G4S_DUP_KEEP or a G4S_COMBINE_* value (default PLUS). Summation order: the reference's constructor sorts each source's edges by (col, value)
// before it sums, so it adds repeats in ascending value; this library adds them in input order. The two agree bit for bit wherever the sums are exact,
// which covers the integer weights graph.h describes.
struct graph {
    long m, n;
    long *start, *end;
    double *w;
};
template <typename IT, typename NT>
void FromCOO(IT rows, IT cols, int64_t nnz, const IT *row, const IT *col, const NT *val, CSR<IT, NT> &c, int dup = G4S_COMBINE_PLUS, g4s_coo_info *info = nullptr)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device works on CSR<int32_t, double>");
    c.make_empty();
    if (rows < 0 || cols < 0 || nnz < 0) throw std::runtime_error("FromCOO: negative size");
    c.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)rows + 1));
    IT *perm = (IT *)g4s_malloc(sizeof(IT) * ((size_t)nnz + 1));
    if (!c.rowptr || !perm) { g4s_free(perm); c.make_empty(); throw std::runtime_error("FromCOO: host allocation failed"); }
    int64_t cnnz = 0;
    g4s_status st = g4s_csr_from_coo_symbolic(dup, rows, cols, nnz, row, col, c.rowptr, perm, &cnnz, G4S_HOST_POINTERS, info, nullptr);
    if (st == G4S_OK) {
        try { detail::adopt(c, rows, cols, cnnz, "FromCOO"); } catch (...) { g4s_free(perm); throw; }
        st = g4s_csr_from_coo_numeric(dup, rows, cols, nnz, row, col, val, c.rowptr, perm, c.colids, val ? c.values : nullptr, G4S_HOST_POINTERS, nullptr);
        if (st == G4S_OK && !val) for (int64_t k = 0; k < cnnz; ++k) c.values[k] = 1.0;
    }
    g4s_free(perm);
    if (st != G4S_OK) { c.make_empty(); check(st, "FromCOO"); }
}
template <typename IT, typename NT>
void FromGraph(const graph &g, CSR<IT, NT> &c, int dup = G4S_COMBINE_PLUS, g4s_coo_info *info = nullptr)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device works on CSR<int32_t, double>");
    if (g.m < 0 || g.n < 0 || g.n > INT32_MAX) throw std::runtime_error("FromGraph: the vertex count does not fit int32");
    IT *row = (IT *)g4s_malloc(sizeof(IT) * ((size_t)g.m + 1)), *col = (IT *)g4s_malloc(sizeof(IT) * ((size_t)g.m + 1));
    auto release = [&] { g4s_free(row); g4s_free(col); };
    if (!row || !col) { release(); throw std::runtime_error("FromGraph: host allocation failed"); }
    for (long e = 0; e < g.m; ++e) {
        if (g.start[e] < INT32_MIN || g.start[e] > INT32_MAX || g.end[e] < INT32_MIN || g.end[e] > INT32_MAX) {
            release();
            throw std::runtime_error("FromGraph: a vertex id does not fit int32");
        }
        row[e] = (IT)g.start[e];
        col[e] = (IT)g.end[e];
    }
    try { FromCOO((IT)g.n, (IT)g.n, (int64_t)g.m, row, col, g.w, c, dup, info); } catch (...) { release(); throw; }
    release();
}
template <typename IT, typename NT>
void ToCOO(const CSR<IT, NT> &a, IT *row_out)
{
    static_assert(std::is_same<IT, int32_t>::value, "the device works on CSR<int32_t, double>");
    const IT zero = 0;
    check(g4s_csr_row_indices(a.rowptr ? a.rows : 0, a.nnz, a.rowptr ? a.rowptr : &zero, row_out, G4S_HOST_POINTERS, nullptr), "ToCOO");
}
template <typename IT, typename NT>
void SortAndMerge(const CSR<IT, NT> &a, CSR<IT, NT> &c, int dup = G4S_COMBINE_PLUS, g4s_coo_info *info = nullptr)
{
    IT *row = (IT *)g4s_malloc(sizeof(IT) * ((size_t)a.nnz + 1));
    if (!row) throw std::runtime_error("SortAndMerge: host allocation failed");
    try {
        ToCOO(a, row);
        FromCOO(a.rows, a.cols, (int64_t)a.nnz, row, a.colids, a.values, c, dup, info);
    } catch (...) { g4s_free(row); throw; }
    g4s_free(row);
}

// C = A[I, J] on the device (g4s_csr_extract_symbolic / _numeric, host arrays; include/g4s.h has the contract): C(p, q) is stored exactly where
// A(ri[p], ci[q]) is — MATLAB's A(I, J). The lists may be in any order and may repeat ids; every row of the result is ordered by (q, stored position).
//   Extract(a, ri, ci, src, info)  the ri.size() × ci.size() result; src (optional) receives the index into a.colids / a.values behind every entry
//   SpRef(a, ri, ci), SpRef2(a, ri, rilen, ci, cilen)   the reference's spelling (CSC::SpRef / SpRef2, mm/inc/CSC.h:513-690). The reference wants sorted lists
//                                  and keeps the original row ids in the result; this is the MATLAB meaning its comment states: rows are renumbered 0 … rilen − 1
//   Permute(a, perm)               a[perm, perm] of a square matrix: vertex perm[p] becomes vertex p
//   SubMatrix(a, M_, N_, M_start, N_start)   the M_ × N_ block at (M_start, N_start): CSR(const CSR&, M_, N_, M_start, N_start), mm/inc/CSR.h:691-733
// (leading_submatrix of g4s/mtx.hpp stays the host loop it is.)
namespace detail {
// src_vec (or NULL) is sized between the two calls, when the entry count is known; src_raw (or NULL) is the caller's array of that many ids.
template <typename IT, typename NT>
CSR<IT, NT> extract(const CSR<IT, NT> &a, const IT *ri, IT rilen, const IT *ci, IT cilen, IT *src_raw, std::vector<IT> *src_vec, g4s_extract_info *info)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device works on CSR<int32_t, double>");
    if (rilen < 0 || cilen < 0) throw std::runtime_error("Extract: negative list length");
    CSR<IT, NT> c;
    const IT zero = 0, none = 0;                           // an empty CSR holds no arrays; an empty list is still a list, not "every row"
    const IT *rp = a.rowptr ? a.rowptr : &zero;
    const IT rows = a.rowptr ? a.rows : 0;
    if (!a.rowptr && rilen > 0) throw std::runtime_error("Extract: a row id of an empty matrix");
    if (!ri) ri = &none;
    if (!ci) ci = &none;
    c.rowptr = (IT *)g4s_malloc(sizeof(IT) * ((size_t)rilen + 1));
    if (!c.rowptr) throw std::runtime_error("Extract: host allocation failed");
    int64_t cnnz = 0;
    g4s_status st = g4s_csr_extract_symbolic(rows, a.cols, rp, a.colids, rilen, ri, cilen, ci, c.rowptr, &cnnz, G4S_HOST_POINTERS, info, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, "Extract"); }
    adopt(c, rilen, cilen, cnnz, "Extract");
    if (src_vec) {
        src_vec->assign((size_t)cnnz + 1, 0);
        src_raw = src_vec->data();
    }
    st = g4s_csr_extract_numeric(rows, a.cols, rp, a.colids, a.values, rilen, ri, cilen, ci, c.rowptr, c.colids, a.values ? c.values : nullptr, src_raw,
                                 G4S_HOST_POINTERS, info, nullptr);
    if (st != G4S_OK) { c.make_empty(); check(st, "Extract"); }
    if (src_vec) src_vec->resize((size_t)cnnz);
    if (!a.values) for (int64_t k = 0; k < cnnz; ++k) c.values[k] = 1.0;
    return c;
}
} // namespace detail
template <typename IT, typename NT>
CSR<IT, NT> SpRef2(const CSR<IT, NT> &a, const IT *ri, IT rilen, const IT *ci, IT cilen, IT *src = nullptr, g4s_extract_info *info = nullptr)
{
    return detail::extract(a, ri, rilen, ci, cilen, src, (std::vector<IT> *)nullptr, info);
}
template <typename IT, typename NT>
CSR<IT, NT> Extract(const CSR<IT, NT> &a, const std::vector<IT> &ri, const std::vector<IT> &ci, std::vector<IT> *src = nullptr, g4s_extract_info *info = nullptr)
{
    if (ri.size() > (size_t)INT32_MAX || ci.size() > (size_t)INT32_MAX) throw std::runtime_error("Extract: a list does not fit int32");
    return detail::extract(a, ri.data(), (IT)ri.size(), ci.data(), (IT)ci.size(), (IT *)nullptr, src, info);
}
template <typename IT, typename NT>
CSR<IT, NT> SpRef(const CSR<IT, NT> &a, const std::vector<IT> &ri, const std::vector<IT> &ci) { return Extract(a, ri, ci); }
template <typename IT, typename NT>
CSR<IT, NT> Permute(const CSR<IT, NT> &a, const std::vector<IT> &perm)
{
    if (a.rows != a.cols) throw std::runtime_error("Permute: the matrix is not square");
    if (perm.size() != (size_t)a.rows) throw std::runtime_error("Permute: perm must hold one id per vertex");
    return Extract(a, perm, perm);
}
template <typename IT, typename NT>
CSR<IT, NT> SubMatrix(const CSR<IT, NT> &a, IT M_, IT N_, IT M_start = 0, IT N_start = 0)
{
    if (M_ < 0 || N_ < 0 || M_start < 0 || N_start < 0 || (int64_t)M_start + M_ > a.rows || (int64_t)N_start + N_ > a.cols)
        throw std::runtime_error("SubMatrix: the block leaves the matrix");
    std::vector<IT> ri((size_t)M_), ci((size_t)N_);
    for (IT p = 0; p < M_; ++p) ri[(size_t)p] = M_start + p;
    for (IT q = 0; q < N_; ++q) ci[(size_t)q] = N_start + q;
    return Extract(a, ri, ci);
}

// Shortest-path distances (dist: a.rows values, +inf where unreached) and BFS levels (level: a.rows values, −1 where unreached) from the nearest of
// n_sources vertices on the graph `a` stores by out-edges (row i: the edges i → j, weight a_ij), host arrays, synchronous: a handle, one g4s_sssp /
// g4s_bfs (include/g4s.h has the contract: exact min-plus fixed point; an entry is a BFS edge when it is != 0), the handle destroyed.
namespace detail {
template <typename IT, typename NT, typename Out, typename Run>
void traverse(const CSR<IT, NT> &a, Out *out, const char *what, Run run)
{
    static_assert(std::is_same<IT, int32_t>::value && std::is_same<NT, double>::value, "the device traversals work on CSR<int32_t, double>");
    g4s_csr_t h = nullptr;
    check(g4s_csr_create(&h, a.rows, a.cols, a.nnz, a.rowptr, a.colids, a.values, G4S_HOST_POINTERS | G4S_SPMV_STREAM), what);
    void *dev = nullptr;
    g4s_status st = g4s_dev_alloc(&dev, sizeof(Out) * ((size_t)a.rows + 1));
    if (st == G4S_OK) st = run(h, (Out *)dev);
    if (st == G4S_OK) st = g4s_memcpy_d2h(out, dev, sizeof(Out) * (size_t)a.rows);
    if (dev) g4s_dev_free(dev);
    g4s_csr_destroy(h);
    check(st, what);
}
} // namespace detail
template <typename IT, typename NT>
void SSSP(const CSR<IT, NT> &a, const IT *sources, IT n_sources, NT *dist, g4s_traverse_info *info = nullptr)
{
    detail::traverse(a, dist, "SSSP", [&](g4s_csr_t h, NT *d) { return g4s_sssp(h, sources, n_sources, d, 0, 0u, info, nullptr); });
}
template <typename IT, typename NT>
void SSSP(const CSR<IT, NT> &a, IT source, NT *dist) { SSSP(a, &source, (IT)1, dist); }
template <typename IT, typename NT>
void BFS(const CSR<IT, NT> &a, const IT *sources, IT n_sources, int32_t *level, g4s_traverse_info *info = nullptr)
{
    detail::traverse(a, level, "BFS", [&](g4s_csr_t h, int32_t *l) { return g4s_bfs(h, sources, n_sources, l, 0, 0u, info, nullptr); });
}
template <typename IT, typename NT>
void BFS(const CSR<IT, NT> &a, IT source, int32_t *level) { BFS(a, &source, (IT)1, level); }

// PageRank of the graph `a` stores by out-edges (g4s_pagerank; include/g4s.h has the contract: networkx's pagerank with dangling = personalization,
// weights finite and >= 0), host arrays, synchronous: rank receives a.rows values; personalization (a.rows values, or nullptr for the uniform
// teleport vector) is staged on the device; max_iterations == 0 means 100. A handle, one call, the handle destroyed.
template <typename IT, typename NT>
void PageRank(const CSR<IT, NT> &a, NT *rank, double damping = 0.85, double tol = 1e-10, int32_t max_iterations = 0, const NT *personalization = nullptr,
              g4s_pagerank_info *info = nullptr)
{
    detail::traverse(a, rank, "PageRank", [&](g4s_csr_t h, NT *r) {
        void *p = nullptr;
        g4s_status st = G4S_OK;
        if (personalization) {
            st = g4s_dev_alloc(&p, sizeof(NT) * ((size_t)a.rows + 1));
            if (st == G4S_OK) st = g4s_memcpy_h2d(p, personalization, sizeof(NT) * (size_t)a.rows);
        }
        if (st == G4S_OK) st = g4s_pagerank(h, damping, tol, max_iterations, (const NT *)p, r, 0u, info, nullptr);
        if (p) g4s_dev_free(p);
        return st;
    });
}

// Betweenness centrality of the graph `a` stores by out-edges, from n_sources vertices (g4s_betweenness; include/g4s.h has the contract: Brandes'
// dependencies summed over the listed sources, an entry is an edge when it is != 0, repeated columns are parallel edges), host arrays, synchronous:
// bc receives a.rows values, scale · Σ_s δ_s. A handle, one call, the handle destroyed.
template <typename IT, typename NT>
void BetweennessCentrality(const CSR<IT, NT> &a, NT *bc, const IT *sources, IT n_sources, double scale = 1.0, g4s_bc_info *info = nullptr)
{
    detail::traverse(a, bc, "BetweennessCentrality", [&](g4s_csr_t h, NT *b) { return g4s_betweenness(h, sources, n_sources, scale, b, 0u, info, nullptr); });
}

// Y = alpha·A·X + beta·Y with host blocks X (cols × k) and Y (rows × k): row-major by default (ld >= k), column-major as in cblas_dxxmm.c's
// B and C (ld >= cols / rows) with col_major = true.
template <typename IT, typename NT>
void SpMM(const CSR<IT, NT> &a, int32_t k, const NT *X, int64_t ldx, NT *Y, int64_t ldy, NT alpha = 1.0, NT beta = 0.0, bool col_major = false)
{
    check(g4s_spmm_csr_i32_f64(a.rows, a.cols, k, a.rowptr, a.colids, a.values, X, ldx, Y, ldy, alpha, beta,
                               G4S_HOST_POINTERS | (col_major ? G4S_SPMM_COL_MAJOR : 0u)), "SpMM");
}

} // namespace g4s
