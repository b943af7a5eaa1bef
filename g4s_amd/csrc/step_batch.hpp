// step_batch.hpp — the host side of the stepped device loops (traverse.hip, betweenness.hip, kcore.hip, ktruss.hip, color.hip, scc.hip, msf.hip, trsv.hip; pagerank.hip takes
// kBatchMax), in plain C++ (no HIP: tests/cpp/step_batch_test.cpp runs it on the host under a sanitizer). The host enqueues a batch of step launches
// blind, reads the state once per batch and sizes the next batch's grid from the frontier it saw; a frontier that outgrows that grid stops the batch
// (stop = 4, frontier.hpp). For the level peels (kcore.hip, ktruss.hip through level_peel.hpp): the words of their state blocks that the page turn and
// the host loop touch (PeelState), and what launch b of a batch is (PeelSchedule).
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

// The head of the device-resident state of a level peel (KcState, KtState): items (vertices, edges) leave level by level and inside a level frontier
// by frontier, through ONE queue that holds all frontiers one behind the other. The host reads the whole block once per batch of steps. The queue words
// — edges_cur … hub_cur and tickets — carry the names flip_queue (frontier.hpp) turns them by, as in ClState (color.hpp) and TrState (trsv.hpp).
struct PeelState {
    long long edges_cur;                // stored entries of the current frontier's rows: what the launch grid is sized from
    long long edges_next;               // of the frontier being built
    unsigned long long edges_walked;    // entries walked by peel steps
    int head, end;                      // the current frontier is queue[head, end)
    int tail;                           // the append counter: queue[end, tail) is the frontier being built; every item is removed once it counts them all
    int n_hub_cur, n_hub_next;          // entries of the two hub lists
    int hub_cur;                        // which hub list belongs to the current frontier
    int level;                          // the level being peeled
    int top_level;                      // the last level at which a scan collected items
    int min_left;                       // minimum remaining degree / support seen by the running scan
    int round;                          // index of the current frontier (of the next one to be built, when it is empty)
    int levels, scans;
    int stop;                           // 0 go on; 1 every item removed; 2 capped by max_k; 4 the frontier outgrew the launch grid
    int invalid;                        // 1 rowptr, 2 an id out of range, 4 a row that is not strictly ascending; the caller's own bits above
    int tickets;                        // workgroups of the running step kernel that have finished
    int pad;
};

// The launches of a level peel's batches. A batch is units of two scans (the level jump, the collect) and `peels` peels; the kernel that finds nothing
// to do returns at once, so a wrong guess costs a launch and never a result. seen() follows what the last batch showed.
struct PeelSchedule {
    int batch, peels = 2;
    int levels_seen = 0, rounds_seen = 0;
    bool know = false;                  // the host's copy is the device's state: a batch has been read
    explicit PeelSchedule(int first_batch) : batch(first_batch) {}
    // the position in the unit at which a batch begins: a frontier is waiting → with the peels
    int start(const PeelState &h) const { return know && h.end != h.head ? 2 : 0; }
    bool is_peel(int start, int b) const { return (start + b) % (2 + peels) >= 2; }
    // a peel goes on from stop == 4 only as the first launch behind the read that saw it
    bool resumes(int start, int b, const PeelState &h) const { return b == 0 && is_peel(start, b) && know && h.stop == 4; }
    // behind a read: the batch doubles from the second read on; peels = rounds per level of the last batch, rounded up, and one to spare
    void seen(const PeelState &h)
    {
        const int dl = std::max(h.levels - levels_seen, 1), dr = h.round - rounds_seen;
        levels_seen = h.levels;
        rounds_seen = h.round;
        if (know) batch = StepGrid::next_batch(batch);
        peels = std::max(2, std::min(batch - 2, (dr + dl - 1) / dl + 1));
        know = true;
    }
};
} // namespace g4s
