// traverse.hpp — the device-resident state of one g4s_sssp / g4s_bfs call (traverse.hip). The host reads the whole block once per batch of steps.
#pragma once
#include <cstdint>

namespace g4s {

struct TravState {
    long long edges_cur;       // out-edges of the current frontier: what the direction rule compares with nnz
    long long edges_next;      // of the frontier being built
    long long edges_relaxed;   // edges walked by push steps + nnz per pull step
    long long reached;         // filled once, after the last step
    int n_cur, n_hub_cur;      // entries of the current queue: from the front, and hubs from the back
    int n_next, n_hub_next;    // tails of the queue being built
    int iter;                  // steps run
    int stop;                  // 0 go on pushing; 1 frontier empty; 2 iteration cap; 3 the next step pulls; 4 the frontier outgrew the launch grid
    int cur;                   // which of the two queues is the current one
    int push_steps, pull_steps;
    int tickets;               // workgroups of the running step kernel that have finished
    int zero_values;           // any_zero_kernel's verdict
    int pad;
};

} // namespace g4s
