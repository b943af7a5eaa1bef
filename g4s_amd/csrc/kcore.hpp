// kcore.hpp — the device-resident state of one g4s_kcore call (kcore.hip). The host reads the whole block once per batch of steps.
#pragma once
#include <cstdint>

namespace g4s {

struct KcState {
    long long edges_cur;                // stored entries of the current frontier's rows: what the launch grid is sized from
    long long edges_next;               // of the frontier being built
    unsigned long long edges_walked;    // entries walked by peel steps (diagonal entries are not walked)
    unsigned long long top_core;        // vertices with core == the degeneracy: filled once, after the last step
    int head, end;                      // the current frontier is queue[head, end)
    int tail;                           // the append counter: queue[end, tail) is the frontier being built; tail == n when every vertex is removed
    int n_hub_cur, n_hub_next;          // entries of the two hub lists
    int hub_cur;                        // which hub list belongs to the current frontier
    int k;                              // the level being peeled
    int top_k;                          // the last level at which a scan collected vertices
    int min_deg;                        // minimum remaining degree seen by the running scan
    int round;                          // index of the current frontier (of the next one to be built, when it is empty)
    int levels, scans;
    int stop;                           // 0 go on; 1 every vertex removed; 2 capped by max_k; 4 the frontier outgrew the launch grid
    int invalid;                        // 1 rowptr, 2 an id out of range, 4 a row that is not strictly ascending
    int tickets;                        // workgroups of the running step kernel that have finished
    int pad;
};

} // namespace g4s
