// semiring.hpp — the value operations of the numeric SpGEMM kernels (spgemm.hip, spgemm_rank.hpp) and of the SpMV kernels (spmv.hip, spmv_dia.hip, spmv_pb.hip,
// spmv_bcsr.hip), one policy per G4S_SEMIRING_* value.
// Every accumulation site of the numeric phase goes through these five calls; the pattern (symbolic phase, row classes, bitmaps, chunks) does
// not depend on them. Each policy maps onto one native instruction per product:
//   identity()          the value an accumulator starts from (a table slot, a chunk slot, a hub row's entry)
//   mul(a, b)           one product
//   combine(x, y)       two partial values in registers (the run-order merge of the short-row kernel)
//   lds_acc(p, v)       fold v into an LDS slot:     ds_add_f64 / ds_min_f64 / ds_max_f64
//   global_acc(p, v)    fold v into an HBM entry:    global_atomic_{add,min,max}_f64
// and two more that only the SpMV needs:
//   fill()              the operand x that makes mul(0.0, x) the identity: what a padded entry (value 0.0) of the blocked SpMV's producer reads
//   normalize(y)        an old y as an operand of combine (g4s_spmv_semiring with G4S_SPMV_ACCUMULATE): itself, or 1.0 / 0.0 for or-and
// PlusTimes is spelled exactly as the kernels were before the policy existed (atomicAdd, a * b, a + b), so it compiles to the same code.
// OrAnd is max over {0, 1}: it reuses the max instructions. min and max do not depend on the order of arrival, so MinPlus, MaxPlus and OrAnd
// give exact, deterministic values on every path (the fetch_min/max builtins compile to the native instructions on gfx950, no CAS loop).
#pragma once
#include <hip/hip_runtime.h>
#include "g4s.h"
#include <type_traits>

namespace g4s {
namespace semiring {

struct PlusTimes {
    static constexpr unsigned kFlag = G4S_SEMIRING_PLUS_TIMES;
    __device__ __forceinline__ static double identity() { return 0.0; }
    __device__ __forceinline__ static double mul(double a, double b) { return a * b; }
    __device__ __forceinline__ static double combine(double x, double y) { return x + y; }
    __device__ __forceinline__ static void lds_acc(double *p, double v) { atomicAdd(p, v); }
    __device__ __forceinline__ static void global_acc(double *p, double v) { atomicAdd(p, v); }
    __device__ __forceinline__ static double fill() { return 0.0; }
    __device__ __forceinline__ static double normalize(double y) { return y; }
};

struct MinPlus {
    static constexpr unsigned kFlag = G4S_SEMIRING_MIN_PLUS;
    __device__ __forceinline__ static double identity() { return __builtin_inf(); }
    __device__ __forceinline__ static double mul(double a, double b) { return a + b; }
    __device__ __forceinline__ static double combine(double x, double y) { return __builtin_fmin(x, y); }
    __device__ __forceinline__ static void lds_acc(double *p, double v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ static void global_acc(double *p, double v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ static double fill() { return __builtin_inf(); }
    __device__ __forceinline__ static double normalize(double y) { return y; }
};

struct MaxPlus {
    static constexpr unsigned kFlag = G4S_SEMIRING_MAX_PLUS;
    __device__ __forceinline__ static double identity() { return -__builtin_inf(); }
    __device__ __forceinline__ static double mul(double a, double b) { return a + b; }
    __device__ __forceinline__ static double combine(double x, double y) { return __builtin_fmax(x, y); }
    __device__ __forceinline__ static void lds_acc(double *p, double v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ static void global_acc(double *p, double v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ static double fill() { return -__builtin_inf(); }
    __device__ __forceinline__ static double normalize(double y) { return y; }
};

struct OrAnd {                                                    // std::logical_and / std::logical_or as 1.0 / 0.0; NaN != 0 counts as true
    static constexpr unsigned kFlag = G4S_SEMIRING_OR_AND;
    __device__ __forceinline__ static double identity() { return 0.0; }
    __device__ __forceinline__ static double mul(double a, double b) { return ((a != 0.0) & (b != 0.0)) ? 1.0 : 0.0; }
    __device__ __forceinline__ static double combine(double x, double y) { return __builtin_fmax(x, y); }
    __device__ __forceinline__ static void lds_acc(double *p, double v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ static void global_acc(double *p, double v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ static double fill() { return 0.0; }
    __device__ __forceinline__ static double normalize(double y) { return y != 0.0 ? 1.0 : 0.0; }
};

template <typename S>
inline constexpr bool is_plus_times = std::is_same<S, PlusTimes>::value;

// Calls f(Policy{}) with the policy the flags select (flags & G4S_SEMIRING_MASK; every value of the two bits is one of the four).
template <typename F>
auto dispatch(unsigned flags, F &&f)
{
    switch (flags & G4S_SEMIRING_MASK) {
    case G4S_SEMIRING_MIN_PLUS: return f(MinPlus{});
    case G4S_SEMIRING_MAX_PLUS: return f(MaxPlus{});
    case G4S_SEMIRING_OR_AND: return f(OrAnd{});
    default: return f(PlusTimes{});
    }
}

} // namespace semiring
} // namespace g4s
