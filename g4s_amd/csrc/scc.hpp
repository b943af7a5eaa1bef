// scc.hpp — the device-resident state of one g4s_strongly_connected_components call (scc.hip). The host reads the whole block once per batch of steps.
#pragma once
#include <cstdint>

namespace g4s {

// The phases of the call, in the order the host guesses them (scc.hip). A kernel runs only when the state says it is its turn.
enum ScPhase {
    SC_SCAN = 0,      // the first trim frontier: every vertex with din == 0 or dout == 0
    SC_PEEL,          // remove the frontier queue[head, end): decrement the neighbours' counters, claim those that reach 0
    SC_PVMAX,         // the largest din·dout among live vertices
    SC_PVMIN,         // the smallest id among the vertices that have it: the pivot
    SC_FWD,           // forward reach from the pivot over A, on the work queue
    SC_BWD,           // backward reach from the pivot over Aᵀ inside the forward set, on the queue
    SC_LABEL,         // the pivot's component gets its smallest id
    SC_CINIT,         // a colouring round begins: colour[v] = v on live vertices, all of them in the first frontier
    SC_CPUSH,         // atomicMin of the colours along live out-edges, to the fixpoint
    SC_CROOTS,        // the live vertices with colour[v] == v label themselves and seed the backward reach
    SC_CBWD,          // backward reach over Aᵀ from all roots at once, through vertices of the root's colour
    SC_DONE
};

struct ScState {
    unsigned long long edges_walked;    // stored entries walked by the stepped phases
    unsigned long long best_prod;       // SC_PVMAX's result
    unsigned long long mx_acc;          // the running kernel's maximum
    unsigned long long components;      // the statistics, filled once after the last step
    unsigned long long best;            // (size << 32) | (INT_MAX − label) of the largest component
    long long work_cur;                 // entries + vertices of the current frontier: what the launch grid is sized from
    long long work_next;                // of the frontier being built
    long long round_work;               // of everything a reach has queued so far: the frontier of the peel behind it
    int phase, stop;                    // stop: 0 go on; 1 nobody is live; 4 the frontier outgrew the launch grid
    int invalid;                        // 1 rowptr, 2 a column id, 4 trowptr, 8 an id of the transpose, 16 trowptr[n] != rowptr[n]
    int tickets;                        // workgroups of the running kernel that have finished
    int nnz[2];                         // rowptr[n], trowptr[n]
    int head, end, tail, round_start;   // the queue: [head, end) is the current frontier, [end, tail) the one being built; tail == n ends the call
    int ha_head, ha_end, ha_tail, ha_round;   // the queued vertices whose row of A is a hub, in the same layout
    int ht_head, ht_end, ht_tail, ht_round;   // the same for rows of Aᵀ
    int w_cur;                          // which work queue holds the current frontier of SC_FWD / SC_CPUSH
    int w_n, w_next;                    // its entries, and those of the one being built
    int wh_n, wh_next;                  // the hubs among them
    int open_hubs[2];                   // hubs found by the opening pass over A and over Aᵀ
    int cnt_acc, mn_acc;                // the running kernel's count and minimum
    int pivot, pivot_size, pivot_done, minid;
    int trimmed, color_rounds, cstep;
    int pad;
};

} // namespace g4s
