// pagerank.hpp — the device-resident state of a g4s_pagerank call (pagerank.hip). The host reads the whole block once per batch of iterations.
#pragma once
#include <cstdint>

namespace g4s {

struct PrState {
    double residual;        // ‖r_k − r_{k−1}‖₁ of the last iteration that ran
    double prev_residual;   // of the one before: the host fits the geometric decay to the two
    double mass;            // Σ over dangling u of r_u, for the iteration that runs next
    double sum_p, sum_r;    // Σ personalization, Σ of the warm start (what the vectors are divided by)
    long long dangling;     // vertices of zero out-strength (strength pass)
    int iter;               // iterations that changed rank
    int stop;               // 0 go on; 1 residual < tol; 2 iteration cap; 3 invalid input (bad_values / bad_vec say which)
    int bad_values;         // strength pass: a stored value is negative, NaN or infinite, or a row sum overflows
    int bad_vec;            // 1: personalization, 2: the warm start — an entry negative or not finite, or the sum not in (0, inf)
};

} // namespace g4s
