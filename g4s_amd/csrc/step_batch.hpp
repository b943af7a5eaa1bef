// step_batch.hpp — the host side of the stepped device loops (traverse.hip, betweenness.hip, kcore.hip; pagerank.hip takes kBatchMax), in plain C++
// (no HIP: tests/cpp/step_batch_test.cpp runs it on the host under a sanitizer). The host enqueues a batch of step launches blind, reads the state once
// per batch and sizes the next batch's grid from the frontier it saw; a frontier that outgrows that grid stops the batch (stop = 4, frontier.hpp).
#pragma once
#include <algorithm>
#include <climits>
namespace g4s {
constexpr int kBatchMax = 64;               // launches behind one state read, at most
constexpr long long kEdgesPerWg = 2048;     // one workgroup per 2048 frontier entries: the last-ticket counter is one contended word
constexpr long long kGridGrowth = 8;        // stop = 4 once the frontier has 8 times the entries the grid was sized for
constexpr int kMinGrid = 8;
struct StepGrid {
    int min_grid, max_grid;
    StepGrid(int lo, int hi) : min_grid(lo), max_grid(std::max(lo, hi)) {}   // a largest grid below the smallest is the smallest
    int grid(long long work) const { return (int)std::max((long long)min_grid, std::min((long long)max_grid, work / kEdgesPerWg)); }
    // the frontier entries above which a step asks for a larger grid than `grid`; the largest grid takes whatever comes
    long long cap(int grid) const { return grid == max_grid ? LLONG_MAX : (long long)grid * kEdgesPerWg * kGridGrowth; }
    static int next_batch(int batch) { return std::min(kBatchMax, 2 * batch); }
};
} // namespace g4s
