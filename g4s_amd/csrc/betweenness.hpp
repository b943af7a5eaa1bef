// betweenness.hpp — the device-resident state of a g4s_betweenness call (betweenness.hip). The host reads the whole block once per batch of forward steps.
#pragma once
#include <cstdint>

namespace g4s {

struct BcState {
    // of the traversal that is running (reset per source)
    long long edges_cur;         // out-edges of the current frontier, hubs included: what the host sizes the next batch's grid from
    long long edges_next;        // of the frontier being built
    long long edges_level_max;   // the most out-edges any level had: sizes the backward grid
    int n_cur, width_max;        // vertices of the current frontier; of the widest level
    int n_hub_cur, n_hub_next;   // entries of the current hub list; of the one being built
    int tail;                    // entries of `order` so far
    int depth;                   // level of the current frontier; once stop == 1, the deepest level D
    int stop;                    // 0 go on; 1 the frontier found nothing new: the forward half is done; 4 the frontier outgrew the launch grid
    int cur;                     // which of the two hub lists is the current one
    int tickets;                 // workgroups of the running step kernel that have finished
    // of the call (reset with its first source)
    int max_depth;
    long long levels;            // forward steps
    long long reached;
    long long edges_walked;      // forward, plus the levels the backward half will walk
    unsigned long long sigma_max_bits;   // the largest σ of a frontier vertex, as the bits of a non-negative double (atomicMax)
    // of the handle
    int zero_values;             // a stored value is 0.0: the kernels have to read the values
    int max_degree;              // longest row
};

} // namespace g4s
