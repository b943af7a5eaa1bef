// spmv_device.hpp — the device helper shared by the kernels of the row-streaming path (spmv.hip) and of the diagonal path (spmv_dia.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "semiring.hpp"

namespace g4s {

#ifndef G4S_STREAM_NT_Y
#define G4S_STREAM_NT_Y 0
#endif
// y stores: plain by default (a nontemporal variant measured no gain on the stencil matrices and −4 % on the cache-resident one)
template <class S>
__device__ __forceinline__ void store_y(double *y, int r, double s, double alpha, double beta)
{
    if constexpr (!g4s::semiring::is_plus_times<S>) {
        y[r] = beta == 0.0 ? s : S::combine(s, S::normalize(y[r]));   // semiring: the row's result, or y ⊕ it (ACCUMULATE)
        return;
    }
    const double v = beta == 0.0 ? alpha * s : alpha * s + beta * y[r];
#if G4S_STREAM_NT_Y
    __builtin_nontemporal_store(v, y + r);
#else
    y[r] = v;
#endif
}

} // namespace g4s
