// kcore.hpp — the device-resident state of one g4s_kcore call (kcore.hip): the level peel's words (step_batch.hpp; an item is a vertex, edges_walked
// leaves out diagonal entries, tail == n when every vertex is removed) and the call's own behind them.
#pragma once
#include "step_batch.hpp"
#include <cstdint>

namespace g4s {

struct KcState : PeelState {
    unsigned long long top_core;        // vertices with core == the degeneracy: filled once, after the last step
};

} // namespace g4s
