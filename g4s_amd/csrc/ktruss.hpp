// ktruss.hpp — the device-resident state of one g4s_ktruss call (ktruss.hip): the level peel's words (step_batch.hpp; an item is an edge, its row the
// shorter row of its endpoints, the level j the support at or below which an edge leaves (truss = j + 2), tail == m when every edge is removed;
// invalid bit 8: the hub-edge list is full) and the call's own behind them.
#pragma once
#include "step_batch.hpp"
#include <cstdint>

namespace g4s {

struct KtState : PeelState {
    unsigned long long support_walked;  // entries walked by the support pass
    unsigned long long support_sum;     // Σ support over the undirected edges = 3 · triangles
    unsigned long long top_edges;       // undirected edges with truss == the largest: filled once, after the last step
    int nnz, m;                         // rowptr[n]; undirected off-diagonal edges (the stored entries right of the diagonal)
    int n_hub_rows, n_hub_all;          // open phase: rows above kHubCut entries; edges whose shorter row is above it (the support pass's hubs)
};

} // namespace g4s
