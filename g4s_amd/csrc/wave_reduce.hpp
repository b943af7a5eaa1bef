// wave_reduce.hpp — the workgroup size of the graph kernels and the reductions over a wave: all that pagerank.hip wants of frontier.hpp.
#pragma once
namespace {
constexpr int WG = 256;
// The wave's sum, maximum or minimum by the shuffle ladder 32, 16, … 1; the result is lane 0's (the other lanes hold partial values). The order is
// fixed, so a floating-point sum has the same bits on every run. wave_max of doubles is fmax: a NaN is dropped.
template <typename T> __device__ __forceinline__ T wave_sum(T v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o); return v; }
template <typename T> __device__ __forceinline__ T wave_max(T v) { for (int o = 32; o > 0; o >>= 1) { const T y = __shfl_down(v, o); v = y > v ? y : v; } return v; }
template <typename T> __device__ __forceinline__ T wave_min(T v) { for (int o = 32; o > 0; o >>= 1) { const T y = __shfl_down(v, o); v = y < v ? y : v; } return v; }
__device__ __forceinline__ double wave_max(double v) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o)); return v; }
} // namespace
