// trsv.hpp — what trsv.hip shares with the outside, in plain C++ (no HIP): the device-resident state of the level peel of the
// analysis, and the way to a plan's schedule (level_schedule.hpp) for ilu.hip, which factorises on the lower plan's.
#pragma once
#include "level_schedule.hpp"
struct g4s_trsv_s;
namespace g4s {

// The state block of the analysis: the words of a frontier walk (ClState's, color.hpp) and the counts the opening pass leaves.
struct TrState {
    long long edges_cur, edges_next;    // entries of the transposed pattern under the current frontier's rows / the one being built
    unsigned long long nnz_off;         // stored off-diagonal entries of the triangle
    unsigned long long nnz_diag;        // stored diagonal entries
    int head, end, tail;                // the current frontier is queue[head, end), [end, tail) the one being built
    int n_hub_cur, n_hub_next, hub_cur; // the two hub lists of the frontier walk
    int n_hub_open;                     // rows of A above kHubCut entries (the opening pass's list)
    int round;                          // frontiers walked so far: the level the next one carries
    int stop;                           // 0 go on; 1 the frontier is empty: every row has its level; 4 the frontier outgrew the launch grid
    int invalid;                        // 1 rowptr, 2 an id out of range
    int bad_row;                        // the smallest row without a stored diagonal entry, n when there is none
    int nnz_in;                         // rowptr[n]
    int tickets;
};

// The schedule of a plan, which lives as long as the plan.
const LevelSchedule &trsv_schedule(const g4s_trsv_s *T);

} // namespace g4s
