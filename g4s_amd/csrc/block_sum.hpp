// block_sum.hpp — the sum of one double per thread over a workgroup of 256 (four wavefronts), the fixed shape every reproducible sum of cg.hip and
// stokes.hip ends in: a shuffle tree per wavefront, then (sh0 + sh1) + (sh2 + sh3). Every thread returns the sum; sh is four doubles of LDS, free again on return.
// (pagerank.hip's own block_sum adds in another order and gives other bits: not this one.)
#pragma once
#include <hip/hip_runtime.h>

namespace g4s {
__device__ __forceinline__ double block_sum(double v, double *sh)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return s;
}
} // namespace g4s
