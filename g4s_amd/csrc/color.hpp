// color.hpp — the device-resident state of one g4s_color call (color.hip). The host reads the whole block once per batch of steps.
#pragma once
#include <cstdint>

namespace g4s {

struct ClState {
    long long edges_cur;                // stored entries of the current frontier's rows: what the launch grid is sized from
    long long edges_next;               // of the frontier being built
    unsigned long long edges_walked;    // entries walked by steps (diagonal entries are not walked)
    unsigned long long class0;          // vertices coloured 0
    int head, end;                      // the current frontier is queue[head, end)
    int tail;                           // the append counter: queue[end, tail) is the frontier being built; tail == n when every vertex is queued
    int n_hub_cur, n_hub_next;          // entries of the two hub lists
    int hub_cur;                        // which hub list belongs to the current frontier
    int over_head, over_end;            // over[over_head, over_end): the vertices the last step found with a full mask, for the scan behind it
    int over_tail;                      // the append counter of the overflow list; at the end of the call: info.overflow
    int max_color;                      // the largest colour written
    int round;                          // index of the current frontier = non-empty frontiers coloured so far
    int stop;                           // 0 go on; 1 every vertex coloured; 4 the frontier outgrew the launch grid; 5 overflow with no scan behind the steps
    int invalid;                        // 1 rowptr, 2 an id out of range, 4 a row that is not strictly ascending
    int tickets;                        // workgroups of the running step kernel that have finished
    int turns;                          // page turns so far: a scan runs only behind a step that ran (the host names the count it expects)
};

} // namespace g4s
