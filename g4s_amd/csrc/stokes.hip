// stokes.hip — the incompressibility (Uzawa / Schur-complement CG) iteration of CitcomS around the velocity solve.
//
// Follows solve_Ahat_p_fhat_CG, citcoms/lib/Stokes_flow_Incomp.c:188-452, in its update order, for the incompressible case
// (inv_gruneisen == 0, so initial_vel_residual :839-881 runs) with solve_del2_u's conjugate-gradient branch
// (General_matrix_functions.c:89-94) as the velocity solve — the loop of g4s_conj_grad (cg.hip), held as a CgSolve (cg_async.hpp) on the element-by-element
// operator, the assembled matrix or a row-partitioned one. The iteration is written once (uzawa_loop) for g4s_stokes_uzawa_cg and g4s_stokes_uzawa_cg_dist.
// Operators: assemble_div_u / assemble_grad_p (Element_calculations.c:701-779) on the per-element gradient vectors
// g[e][p] = elt_del[e].g[p][0]; norms: global_v_norm2 / global_p_norm2 / global_div_norm2 / global_pdot
// (Global_operations.c:565-656), one process. Every vector stays in HBM; the host owns the outer loop's scalar logic
// (keep_iterating :150-162, the "two consecutive converging iterations" rule); δ, α and the norms are computed on the device and
// nine doubles come back once per outer iteration.
#include "common.hpp"
#include "readback.hpp"
#include "cg_async.hpp"
#include "block_sum.hpp"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace {

constexpr int kBlocks = 256, kThreads = 256;

using g4s::block_sum;

// A reduction of K sums at once. f(i) does the element-wise work of index i and returns its K terms; the sums have a fixed two-level shape (grid-stride
// partials per workgroup → one workgroup adds the kBlocks partials of each sum): reproducible, on one device and on every rank alike. K = 6 carries
// everything an outer iteration can sum once its new V, P and r are known in one pass (and, partitioned, in ONE all-reduce message: Global_operations.c:534-656
// reduces each norm on its own).
template <int K> struct Sums { double v[K]; };

template <int K, typename F>
__global__ __launch_bounds__(kThreads) void map_sum_kernel(int n, F f, double *__restrict__ part)
{
    __shared__ double sh[4];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += kBlocks * kThreads) {
        const Sums<K> v = f(i);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += v.v[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double t = block_sum(acc[k], sh);
        if (threadIdx.x == 0) part[k * kBlocks + blockIdx.x] = t;
    }
}

// One workgroup closes the reduction on one device: the K sums, then the epilogue ep(r) on one thread — the scalar algebra of the outer loop (δ, α, the
// norms) stays on the device, in the slots of a small scalar array the following kernels read.
template <int K, typename E>
__global__ __launch_bounds__(kThreads) void finish_sums_kernel(const double *__restrict__ part, E ep)
{
    __shared__ double sh[4];
    static_assert(kBlocks == kThreads, "one partial per thread");
    double r[K];
    for (int k = 0; k < K; ++k) r[k] = block_sum(part[k * kBlocks + threadIdx.x], sh);
    if (threadIdx.x == 0) ep(r);
}

// On a partitioned operator it closes in three steps: the rank's own K sums go to raw, the caller all-reduces raw, and one thread runs the same epilogue on it.
template <int K>
__global__ __launch_bounds__(kThreads) void finish_raw_kernel(const double *__restrict__ part, double *__restrict__ raw)
{
    __shared__ double sh[4];
    static_assert(kBlocks == kThreads, "one partial per thread");
    for (int k = 0; k < K; ++k) {
        const double r = block_sum(part[k * kBlocks + threadIdx.x], sh);
        if (threadIdx.x == 0) raw[k] = r;
    }
}
template <typename E>
__global__ void scalar_kernel(E ep, const double *r) { if (threadIdx.x == 0 && blockIdx.x == 0) ep(r); }

template <typename F>
__global__ __launch_bounds__(kThreads) void map_kernel(int n, F f)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) f(i);
}

// divU[e] = Σ_a (g0·U[j1] + g1·U[j2] + g2·U[j3]) in a order — the per-element sequence of assemble_div_u (bit-identical).
// Eight lanes per element: lane a forms the term of local node a (its gathers of U are independent of the other lanes'), then the
// terms are added in a = 0, 1, 2, … order through shuffles, as the source's loop adds them. One thread per element was a chain of
// 24 dependent gathers (11 µs for 8192 elements).
__global__ __launch_bounds__(kThreads) void div_u_kernel(int nel, int npe, int dof, const int *__restrict__ elem_eq, const double *__restrict__ g,
                                                          const double *__restrict__ U, double *__restrict__ divU)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    const int e = idx >> 3, sub = idx & 7;
    const int n = npe * dof;
    const bool ok = e < nel;
    double s = 0.0;
    for (int a0 = 0; a0 < npe; a0 += 8) {                          // npe = 8 in CitcomS: one round
        const int a = a0 + sub;
        double t = 0.0;
        if (ok && a < npe)
            for (int d = 0; d < dof; ++d) {
                const double q = g[(size_t)e * n + a * dof + d] * U[elem_eq[(size_t)e * n + a * dof + d]];
                t = d == 0 ? q : t + q;
            }
        for (int k = 0; k < 8 && a0 + k < npe; ++k) s = s + __shfl(t, (threadIdx.x & ~7) + k, 64);   // every lane of the group keeps the same running sum
    }
    if (ok && sub == 0) divU[e] = s;
}

// gradP[eq(node, d)] = Σ over the node's (element, local node) terms, ascending element, of g·P[e], elements with P == 0 skipped:
// the sequence of additions assemble_grad_p makes into that equation (bit-identical). A gather: no atomics.
__global__ __launch_bounds__(kThreads) void grad_p_kernel(int nno, int npe, int dof, const int *__restrict__ node_ptr,
                                                           const int *__restrict__ node_terms, const int *__restrict__ node_eq,
                                                           const double *__restrict__ g, const double *__restrict__ P, double *__restrict__ gradP)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= nno * dof) return;
    const int node = idx / dof, d = idx - node * dof, n = npe * dof;
    double s = 0.0;
    for (int t = node_ptr[node]; t < node_ptr[node + 1]; ++t) {
        const int term = node_terms[t], e = term / npe, a = term - e * npe;
        const double pe = P[e];
        if (pe == 0.0) continue;
        const double q = g[(size_t)e * n + a * dof + d] * pe;
        s = s + q;
    }
    gradP[node_eq[idx]] = s;
}

__global__ __launch_bounds__(kThreads) void zero_rows_kernel(int n_zero, const int *__restrict__ rows, double *__restrict__ v)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_zero) v[rows[i]] = 0.0;
}

// BPI[e] = 1 / Σ_p g[e][p]·(BI[eq(e,p)]·g[e][p])  (assemble_dAhatp_entry + build_diagonal_of_Ahat)
__global__ __launch_bounds__(kThreads) void pressure_precond_kernel(int nel, int n, const int *__restrict__ elem_eq, const double *__restrict__ g,
                                                                     const double *__restrict__ BI, double *__restrict__ BPI)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nel) return;
    double divU = 0.0;
    for (int p = 0; p < n; ++p) {
        const double ge = g[(size_t)e * n + p];
        const double gradP = BI[elem_eq[(size_t)e * n + p]] * ge;
        const double q = ge * gradP;
        divU = divU + q;
    }
    BPI[e] = divU != 0.0 ? 1.0 / divU : 1.0;
}

inline int grid_for(int n) { return (n + kThreads - 1) / kThreads; }

inline void strip_rows(int n_zero, const int32_t *rows, double *x, hipStream_t s)
{
    if (n_zero) hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for(n_zero)), dim3(kThreads), 0, s, n_zero, rows, x);
}

// A block of the stream-ordered scratch pool, given back when its owner goes; take() hands out its pieces in order (sizes in bytes, multiples of 256).
struct Scratch {
    explicit Scratch(hipStream_t s) : s(s) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { g4s::scratch_free(p, s); }
    int alloc(size_t bytes) { return g4s::scratch_alloc(&p, bytes, s); }
    double *take(size_t bytes) { double *r = reinterpret_cast<double *>(static_cast<char *>(p) + used); used += bytes; return r; }
    void *p = nullptr;
    size_t used = 0;
    const hipStream_t s;
};

} // namespace

G4S_API g4s_status g4s_elem_op_div_u(g4s_elem_op_t op, const double *g_dev, const double *U_dev, double *divU_dev, void *stream)
{
    g4s::ElemOpView v;
    G4S_TRY(g4s_elem_op_view(op, &v));
    G4S_REQUIRE(v.nel == 0 || (g_dev && U_dev && divU_dev), "NULL argument");
    if (v.nel) hipLaunchKernelGGL(div_u_kernel, dim3(grid_for(v.nel * 8)), dim3(kThreads), 0, g4s::as_stream(stream), v.nel, v.npe, v.dof, v.elem_eq, g_dev, U_dev, divU_dev);
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

G4S_API g4s_status g4s_elem_op_grad_p(g4s_elem_op_t op, const double *g_dev, const double *P_dev, double *gradP_dev,
                                      const int32_t *zero_resid_dev, int32_t n_zero, void *stream)
{
    g4s::ElemOpView v;
    G4S_TRY(g4s_elem_op_view(op, &v));
    G4S_REQUIRE(v.neq == 0 || gradP_dev, "NULL argument");
    G4S_REQUIRE(v.nel == 0 || (g_dev && P_dev), "NULL argument");
    G4S_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero_resid_dev), "zero_resid is NULL");
    hipStream_t s = g4s::as_stream(stream);
    // equations no node owns receive nothing and must read 0 (the source zeroes gradP first)
    if (v.neq && (int64_t)v.nno * v.dof != v.neq) G4S_HIP_TRY(hipMemsetAsync(gradP_dev, 0, sizeof(double) * (size_t)v.neq, s));
    if (v.nno) hipLaunchKernelGGL(grad_p_kernel, dim3(grid_for(v.nno * v.dof)), dim3(kThreads), 0, s, v.nno, v.npe, v.dof, v.node_ptr, v.node_terms, v.node_eq, g_dev, P_dev, gradP_dev);
    if (n_zero) hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for(n_zero)), dim3(kThreads), 0, s, n_zero, zero_resid_dev, gradP_dev);
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

G4S_API g4s_status g4s_elem_op_pressure_preconditioner(g4s_elem_op_t op, const double *g_dev, const double *BI_dev, double *BPI_dev, void *stream)
{
    g4s::ElemOpView v;
    G4S_TRY(g4s_elem_op_view(op, &v));
    G4S_REQUIRE(v.nel == 0 || (g_dev && BI_dev && BPI_dev), "NULL argument");
    if (v.nel) hipLaunchKernelGGL(pressure_precond_kernel, dim3(grid_for(v.nel)), dim3(kThreads), 0, g4s::as_stream(stream), v.nel, v.npe * v.dof, v.elem_eq, g_dev, BI_dev, BPI_dev);
    G4S_HIP_TRY(hipGetLastError());
    return G4S_OK;
}

// ------------------------------------------------------------------------------------------------ the outer iteration, once for both operators
namespace g4s { int dist_product(g4s_spmv_dist_t A, const g4s_transport *tr, const double *x, double *y, void *stream); }   // cg.hip

namespace {

// What uzawa_loop asks of an operator (a policy object, passed by reference on the host; device code gets only `vnorm`, by value):
//   grad_p(in, out)   assemble_grad_p + strip_bcs;   div_u(in, out)   assemble_div_u;   apply_K(in, out)   the stiffness product, not stripped
//   vnorm(X, i), n_vnorm   the i-th summand of global_v_norm2 of X and how many there are
//   solve(BI, acc, steps)  the velocity solves of the call (cg_async.hpp)
//   close<K>(part, raw, ep, s)   the end of a reduction: the K sums of the partials in `part` reach ep(r) on one device thread
struct LocalOps {                                                  // one device: the element operator, K through it or through g4s_spmv
    g4s_elem_op_t op; g4s_csr_t K_csr; const double *g; const int32_t *zero_resid; int n_zero; void *stream;
    struct VNorm {                                                 // (Σ_d X[eq(i,d)]²)·NMass[i] over the nodes
        const int *node_eq; const double *nmass; int dof;
        __device__ double operator()(const double *X, int i) const
        {
            double t = 0.0;
            for (int d = 0; d < dof; ++d) { const double x = X[node_eq[i * dof + d]]; const double q = x * x; t = d == 0 ? q : t + q; }
            return t * nmass[i];
        }
    } vnorm;
    int n_vnorm, neq;
    int grad_p(const double *in, double *out) const { return g4s_elem_op_grad_p(op, g, in, out, zero_resid, n_zero, stream); }
    int div_u(const double *in, double *out) const { return g4s_elem_op_div_u(op, g, in, out, stream); }
    int apply_K(const double *in, double *out) const { return K_csr ? g4s_spmv(K_csr, in, out, 1.0, 0.0, stream) : g4s_elem_op_apply(op, in, out, stream); }
    g4s::LocalCgSolve solve(const double *BI, double acc, int steps) const   // General_matrix_functions.c:48-146, CG branch
    {
        return g4s::LocalCgSolve(K_csr ? nullptr : op, K_csr, neq, BI, zero_resid, n_zero, acc, steps, stream);
    }
    template <int K, typename E> int close(const double *part, double *, E ep, hipStream_t s) const   // one launch: the sums and the epilogue
    {
        hipLaunchKernelGGL((finish_sums_kernel<K, E>), dim3(1), dim3(kThreads), 0, s, part, ep);
        return G4S_OK;
    }
};

struct DistOps {                                                   // row-partitioned K, D, Dt; every sum goes over the ranks
    g4s_spmv_dist_t K, D, Dt; const g4s_transport *tr; const int32_t *zero_resid; int n_zero; void *stream;
    struct VNorm {                                                 // X[i]²·vmass[i] over this rank's equations
        const double *vmass;
        __device__ double operator()(const double *X, int i) const { return X[i] * X[i] * vmass[i]; }
    } vnorm;
    int n_vnorm, neq;
    int grad_p(const double *in, double *out) const
    {
        G4S_TRY(g4s::dist_product(Dt, tr, in, out, stream));
        strip_rows(n_zero, zero_resid, out, g4s::as_stream(stream));
        return G4S_OK;
    }
    int div_u(const double *in, double *out) const { return g4s::dist_product(D, tr, in, out, stream); }
    int apply_K(const double *in, double *out) const { return g4s::dist_product(K, tr, in, out, stream); }
    g4s::DistCgSolve solve(const double *BI, double acc, int steps) const { return g4s::DistCgSolve(K, tr, neq, BI, zero_resid, n_zero, acc, steps, stream); }
    template <int K_, typename E> int close(const double *part, double *raw, E ep, hipStream_t s) const   // raw local sums → summed over the ranks → the epilogue
    {
        hipLaunchKernelGGL((finish_raw_kernel<K_>), dim3(1), dim3(kThreads), 0, s, part, raw);
        G4S_TRY(tr->allreduce_sum_f64(tr->ctx, raw, K_, stream));
        hipLaunchKernelGGL((scalar_kernel<E>), dim3(1), dim3(64), 0, s, ep, raw);
        return G4S_OK;
    }
};

// solve_Ahat_p_fhat_CG from the workspace to *res. `entry` names the caller in the loop's one error message; the entry points have checked the arguments.
template <typename Ops>
int uzawa_loop(const char *entry, const Ops &ops, int neq, int nel, const double *BI, const double *BPI, const double *area, double volume, const int32_t *zero_resid,
               int n_zero, const double *FF, double *V, double *P, const g4s_stokes_params *prm, g4s_stokes_result *res, double *hist, int hist_lines, hipStream_t s)
{
    // sc: device scalars of the loop. A reduction = map_sum over the vectors + ops.close, whose epilogue writes the derived scalars; nothing comes to the
    // host until fetch() at the end of an outer iteration. <r1, z1> of the NEXT outer iteration is formed in the closing reduction of the current one (r2 is
    // final there; round 5): the two slots of R1Z1 / DELTA alternate by the iteration's parity — the closing step may run twice (a speculation that did not
    // hold) and must find the current pair untouched.
    enum { R1Z1_0, R1Z1_1, DELTA_0, DELTA_1, ALPHA, VDOTV, U1DOTU1, PDOTP, S2S2, DIVN, NSC };
    static_assert(NSC <= 16, "scalar slots");
    const size_t nq = ((size_t)neq * 8 + 255) / 256 * 256, np = ((size_t)nel * 8 + 255) / 256 * 256;
    Scratch scr(s), scr2(s);
    G4S_TRY(scr.alloc(3 * nq + 6 * np + sizeof(double) * (6 * kBlocks + 32)));
    double *F = scr.take(nq), *u1 = scr.take(nq), *tmp = scr.take(nq);
    double *r1 = scr.take(np), *r2 = scr.take(np), *z1 = scr.take(np), *s1 = scr.take(np), *s2 = scr.take(np), *Fp = scr.take(np);
    double *part = scr.take(sizeof(double) * 6 * kBlocks), *sc = scr.take(sizeof(double) * 16), *raw = scr.take(sizeof(double) * 16);   // raw: sums on their way through an all-reduce
    // V and P of the NEXT outer iteration are written beside the current ones (ping-pong): an iteration that was enqueued behind a velocity solve whose
    // first batch turns out not to have met its test can then simply be enqueued again, from unchanged inputs
    G4S_TRY(scr2.alloc(nq + np));
    double *Vc = V, *Vn = scr2.take(nq), *Pc = P, *Pn = scr2.take(np);
    // G4S_STOKES_SYNC=1: wait for every velocity solve before enqueuing what follows it (the round-2 behaviour, for A/B)
    const bool speculate = !(getenv("G4S_STOKES_SYNC") && atoi(getenv("G4S_STOKES_SYNC")) != 0);

    double hsc[NSC] = {0};
    auto reduce = [&](auto k, int n, auto f, auto ep) -> int {     // k: the number of sums, as a std::integral_constant
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL((map_sum_kernel<K, decltype(f)>), dim3(kBlocks), dim3(kThreads), 0, s, n, f, part);
        return ops.template close<K>(part, raw, ep, s);
    };
    constexpr std::integral_constant<int, 1> one{};
    constexpr std::integral_constant<int, 6> six{};
    auto fetch = [&]() -> int {
        G4S_HIP_TRY(hipGetLastError());
        G4S_HIP_TRY(g4s::ReadScope(s).fetch(hsc, sc));
        return G4S_OK;
    };
    auto each = [&](int n, auto f) { hipLaunchKernelGGL(map_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, n, f); };
    auto strip = [&](double *x) { strip_rows(n_zero, zero_resid, x, s); };
    const auto vnorm = ops.vnorm;                                  // device lambdas take the functor, never the policy
    const int n_norms = std::max(ops.n_vnorm, nel), n_vnorm = ops.n_vnorm;
    int64_t inner_total = 0;
    const double inner_acc = prm->imp * prm->inner_accuracy_scale * prm->v_res;
    auto cg = ops.solve(BI, inner_acc, prm->v_steps_low);          // every velocity solve of the call: one workspace, one boundary mask
    int32_t cycles = 0;
    double residual = 0.0;
    bool held = true;

    // ---- initial_vel_residual (:839-881): F = FF − grad(P) − K·V, stripped; K·u1 = F; V += u1
    G4S_TRY(ops.grad_p(P, u1));
    each(neq, [=] __device__(int i) { F[i] = FF[i] - u1[i]; });
    G4S_TRY(ops.apply_K(V, u1));
    strip(u1);
    each(neq, [=] __device__(int i) { F[i] = F[i] - u1[i]; });
    strip(F);
    // this solve's result feeds sums whose inputs it also writes in place (V += u1): waited for, not speculated on — once per call
    G4S_TRY(cg.start(F, u1));
    G4S_TRY(cg.read());
    G4S_HIP_TRY(g4s::reads_sync(s));
    G4S_TRY(cg.settle(&held, &cycles, &residual));
    inner_total += cycles;
    int valid = residual < inner_acc ? 1 : 0;
    each(neq, [=] __device__(int i) { V[i] = V[i] + u1[i]; });

    // ---- r1 = div(V); incompressibility = sqrt(|r1|²_div / (1e-32 + |V|²))
    G4S_TRY(ops.div_u(V, r1));
    G4S_HIP_TRY(hipMemsetAsync(sc, 0, sizeof(double) * NSC, s));
    G4S_TRY(reduce(six, n_norms, [=] __device__(int i) {
        Sums<6> o{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        if (i < n_vnorm) o.v[0] = vnorm(V, i);
        if (i < nel) {
            o.v[1] = r1[i] * r1[i] / area[i]; o.v[2] = P[i] * P[i] * area[i];
            const double z = BPI[i] * r1[i];                          // z1 = BPI∘r1 and <r1, z1> of the first outer iteration (:296-318)
            z1[i] = z; o.v[3] = r1[i] * z;
        }
        return o;
    }, [=] __device__(const double *r) { sc[VDOTV] = r[0]; sc[DIVN] = r[1]; sc[PDOTP] = r[2]; sc[R1Z1_0] = r[3]; }));
    G4S_TRY(fetch());
    double vdotv = hsc[VDOTV] / volume, pdotp = hsc[PDOTP] / volume;
    double incompressibility = std::sqrt(hsc[DIVN] / volume / (1e-32 + vdotv));
    double dvelocity = 1.0, dpressure = 1.0;
    int count = 0, converging = 0, lines = 0;
    auto record = [&]() {
        if (lines < hist_lines) { double *h = hist + 5 * (size_t)lines; h[0] = std::sqrt(vdotv); h[1] = std::sqrt(pdotp); h[2] = dvelocity; h[3] = dpressure; h[4] = incompressibility; }
        ++lines;
    };
    record();
    for (;;) {
        const bool keep = prm->check_continuity_convergence ? (incompressibility > prm->imp || converging < 2)
                                                            : (incompressibility > prm->imp && converging < 2);   // keep_iterating :150-162
        if (!(count < prm->steps_max && keep)) break;              // (partitioned: every rank holds the same all-reduced scalars — the same verdict everywhere)
        // z1 = BPI∘r1, <r1, z1> and δ = <r1, z1> / <r0, z0> (:296-318) sit in slot `cur`: written by the closing reduction of the previous iteration
        const int cur = count & 1, nxt = cur ^ 1;
        if (hsc[R1Z1_0 + cur] == 0.0) return g4s::set_error(G4S_ERR_INVALID, "%s: <r1, z1> = 0 at the head of iteration %d (the source asserts)", entry, count);
        const bool first = count == 0;
        each(nel, [=] __device__(int i) { s2[i] = first ? z1[i] : z1[i] + sc[DELTA_0 + cur] * s1[i]; });
        // K·u1 = grad(s2). The solve's first batch (one iteration more than the previous solve needed) is only enqueued — partitioned: its products, exchanges
        // and all-reduces included, with an RCCL transport none of them waits for the host; everything that follows it in this outer iteration is enqueued
        // behind it at once, and ONE synchronisation brings back the solve's state and the nine scalars. Before round 3 the host waited for the solve, then
        // enqueued the rest and waited again: at Cookbook2's size the loop was host-bound (38 launches of 3–11 µs and two read-backs per outer iteration:
        // 0.21 ms, of which the device needs 0.13 — tools/uzawa_graph_probe.py).
        G4S_TRY(ops.grad_p(s2, tmp));
        G4S_TRY(cg.start(tmp, u1));
        held = true;
        if (!speculate) {
            G4S_TRY(cg.read());
            G4S_HIP_TRY(g4s::reads_sync(s));
            G4S_TRY(cg.settle(&held, &cycles, &residual));
        }
        auto rest_of_iteration = [&]() -> int {
            G4S_TRY(ops.div_u(u1, Fp));
            // α = <r1, z1> / <s2, div(u1)>; r2, P, V (:336-354)
            G4S_TRY(reduce(one, nel, [=] __device__(int i) { return Sums<1>{{s2[i] * Fp[i]}}; }, [=] __device__(const double *r) { sc[ALPHA] = sc[R1Z1_0 + cur] / r[0]; }));
            each(std::max(nel, neq), [=] __device__(int i) {        // one launch for the three updates
                const double alpha = sc[ALPHA];
                if (i < nel) { r2[i] = r1[i] - alpha * Fp[i]; Pn[i] = Pc[i] + alpha * s2[i]; }
                if (i < neq) Vn[i] = Vc[i] - alpha * u1[i];
            });
            G4S_TRY(ops.div_u(Vn, Fp));                             // (Fp = div(u1) has gone into r2: the buffer is free)
            // the five norms of the iteration and, since r2 is final, z1 = BPI∘r2 and <r1, z1> of the NEXT one, in one two-level pass
            return reduce(six, n_norms, [=] __device__(int i) {
                Sums<6> o{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
                if (i < n_vnorm) { o.v[0] = vnorm(Vn, i); o.v[1] = vnorm(u1, i); }
                if (i < nel) {
                    o.v[2] = Pn[i] * Pn[i] * area[i]; o.v[3] = s2[i] * s2[i] * area[i]; o.v[4] = Fp[i] * Fp[i] / area[i];
                    const double z = BPI[i] * r2[i];
                    z1[i] = z; o.v[5] = r2[i] * z;
                }
                return o;
            }, [=] __device__(const double *r) {
                sc[VDOTV] = r[0]; sc[U1DOTU1] = r[1]; sc[PDOTP] = r[2]; sc[S2S2] = r[3]; sc[DIVN] = r[4];
                sc[R1Z1_0 + nxt] = r[5]; sc[DELTA_0 + nxt] = r[5] / sc[R1Z1_0 + cur];      // δ of the next iteration = its <r1, z1> over this one's (:296-318, :405)
            });
        };
        G4S_TRY(rest_of_iteration());
        if (speculate) {
            G4S_TRY(cg.read());
            G4S_TRY(fetch());
            G4S_TRY(cg.settle(&held, &cycles, &residual));
            if (!held) G4S_TRY(rest_of_iteration());              // the first batch did not meet the test: u1 is final only now — once more, from the same V, P, r1, s2 (all ranks alike)
        }
        inner_total += cycles;
        valid = residual < inner_acc ? 1 : 0;
        if (!speculate || !held) G4S_TRY(fetch());                 // (speculation that held: the scalars came back with the solve's state)
        const double alpha = hsc[ALPHA];
        vdotv = hsc[VDOTV] / volume;
        pdotp = hsc[PDOTP] / volume;
        dvelocity = alpha * std::sqrt(hsc[U1DOTU1] / volume / (1e-32 + vdotv));
        dpressure = alpha * std::sqrt(hsc[S2S2] / volume / (1e-32 + pdotp));
        incompressibility = std::sqrt(hsc[DIVN] / volume / (1e-32 + vdotv));
        ++count;
        record();
        if (!valid) converging = 0;
        else if (prm->check_pressure_convergence) converging = (dvelocity < prm->imp && dpressure < prm->imp) ? converging + 1 : 0;
        else converging = dvelocity < prm->imp ? converging + 1 : 0;
        std::swap(s1, s2);
        std::swap(r1, r2);
        std::swap(Vc, Vn);
        std::swap(Pc, Pn);
    }
    if (Vc != V) {                                                 // an odd number of iterations: the result sits in the scratch pair
        G4S_HIP_TRY(hipMemcpyAsync(V, Vc, sizeof(double) * (size_t)neq, hipMemcpyDeviceToDevice, s));
        G4S_HIP_TRY(hipMemcpyAsync(P, Pc, sizeof(double) * (size_t)nel, hipMemcpyDeviceToDevice, s));
    }
    G4S_HIP_TRY(hipGetLastError());
    G4S_HIP_TRY(g4s::reads_sync(s));
    res->outer_iterations = count;
    res->inner_iterations = inner_total;
    res->last_solve_valid = valid;
    res->incompressibility = incompressibility;
    res->v_norm = std::sqrt(vdotv);
    res->p_norm = std::sqrt(pdotp);
    res->dvelocity = dvelocity;
    res->dpressure = dpressure;
    return G4S_OK;
}

} // namespace

G4S_API g4s_status g4s_stokes_uzawa_cg(g4s_elem_op_t op, g4s_csr_t K_csr, const double *g, const double *BI, const double *BPI, const double *nmass,
                                       const double *area, double volume, const int32_t *zero_resid, int32_t n_zero, const double *FF,
                                       double *V, double *P, const g4s_stokes_params *prm, g4s_stokes_result *res, double *hist,
                                       int32_t hist_lines, void *stream)
{
    g4s::ElemOpView v;
    G4S_TRY(g4s_elem_op_view(op, &v));
    G4S_REQUIRE(prm && res, "params / result is NULL");
    G4S_REQUIRE(v.nel > 0 && v.neq > 0 && v.nno > 0, "empty operator");
    G4S_REQUIRE(g && BI && BPI && nmass && area && FF && V && P, "NULL argument");
    G4S_REQUIRE(volume > 0.0, "volume must be positive");
    G4S_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero_resid), "zero_resid is NULL");
    G4S_REQUIRE(hist_lines >= 0 && (hist_lines == 0 || hist), "hist is NULL");
    const LocalOps ops{op, K_csr, g, zero_resid, n_zero, stream, {v.node_eq, nmass, v.dof}, v.nno, v.neq};
    return uzawa_loop(__func__, ops, v.neq, v.nel, BI, BPI, area, volume, zero_resid, n_zero, FF, V, P, prm, res, hist, hist_lines, g4s::as_stream(stream));
}

// the same iteration on a partitioned operator: this rank's neq equations and nel elements
G4S_API g4s_status g4s_stokes_uzawa_cg_dist(g4s_spmv_dist_t K, g4s_spmv_dist_t D, g4s_spmv_dist_t Dt, const g4s_transport *tr, int32_t neq, int32_t nel,
                                            const double *BI, const double *BPI, const double *vmass, const double *area, double volume,
                                            const int32_t *zero_resid, int32_t n_zero, const double *FF, double *V, double *P,
                                            const g4s_stokes_params *prm, g4s_stokes_result *res, double *hist, int32_t hist_lines, void *stream)
{
    G4S_REQUIRE(K && D && Dt && tr && tr->allreduce_sum_f64 && prm && res, "NULL argument");
    G4S_REQUIRE(neq > 0 && nel > 0, "every rank must own at least one equation and one element");
    G4S_REQUIRE(BI && BPI && vmass && area && FF && V && P, "NULL argument");
    G4S_REQUIRE(volume > 0.0, "volume must be positive");
    G4S_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero_resid), "zero_resid is NULL");
    G4S_REQUIRE(hist_lines >= 0 && (hist_lines == 0 || hist), "hist is NULL");
    const DistOps ops{K, D, Dt, tr, zero_resid, n_zero, stream, {vmass}, neq, neq};
    return uzawa_loop(__func__, ops, neq, nel, BI, BPI, area, volume, zero_resid, n_zero, FF, V, P, prm, res, hist, hist_lines, g4s::as_stream(stream));
}
