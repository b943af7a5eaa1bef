// ktruss.hpp — the device-resident state of one g4s_ktruss call (ktruss.hip). The host reads the whole block once per batch of steps.
#pragma once
#include <cstdint>

namespace g4s {

struct KtState {
    long long edges_cur;                // entries of the current frontier's walk rows (the shorter row of each edge): what the launch grid is sized from
    long long edges_next;               // of the frontier being built
    unsigned long long edges_walked;    // entries walked by peel steps
    unsigned long long support_walked;  // entries walked by the support pass
    unsigned long long support_sum;     // Σ support over the undirected edges = 3 · triangles
    unsigned long long top_edges;       // undirected edges with truss == the largest: filled once, after the last step
    int nnz, m;                         // rowptr[n]; undirected off-diagonal edges (the stored entries right of the diagonal)
    int head, end;                      // the current frontier is queue[head, end)
    int tail;                           // the append counter: queue[end, tail) is the frontier being built; tail == m when every edge is removed
    int n_hub_cur, n_hub_next;          // entries of the two hub lists
    int hub_cur;                        // which hub list belongs to the current frontier
    int n_hub_rows, n_hub_all;          // open phase: rows above kHubCut entries; edges whose shorter row is above it (the support pass's hubs)
    int j;                              // the level being peeled: the support at or below which an edge leaves (truss = j + 2)
    int top_j;                          // the last level at which a scan collected edges
    int min_sup;                        // minimum remaining support seen by the running scan
    int round;                          // index of the current frontier (of the next one to be built, when it is empty)
    int levels, scans;
    int stop;                           // 0 go on; 1 every edge removed; 2 capped by max_k; 4 the frontier outgrew the launch grid
    int invalid;                        // 1 rowptr, 2 an id out of range, 4 a row that is not strictly ascending, 8 the hub-edge list is full
    int tickets;                        // workgroups of the running step kernel that have finished
    int pad;
};

} // namespace g4s
