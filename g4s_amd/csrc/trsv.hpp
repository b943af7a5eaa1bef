// trsv.hpp — what trsv.hip shares with the outside, in plain C++ (no HIP): the device-resident state of the level peel of the
// analysis, the way to a plan's schedule (level_schedule.hpp) for ilu.hip, which factorises on the lower plan's, and the refusals of a block call,
// which g4s_ilu0_apply_multi shares.
#pragma once
#include <cstdint>
#include "g4s.h"
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

int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // common.hpp's

// What a block call (g4s_sptrsv_solve_multi, g4s_ilu0_apply_multi) asks of its arguments behind a handle that is not NULL, in the
// order of g4s.h: go_on, or return status — a refusal under the name fn of the entry point, or G4S_OK where n == 0 or k == 0 leave nothing to do.
// It makes no HIP call and is given nothing of the handle but its n. in and out are the names of the two blocks in the texts.
struct BlockCall {
    int status;
    bool go_on;
};

inline BlockCall check_block_call(const char *fn, int n, int32_t k, const char *in, const void *in_dev, int64_t ld_in, const char *out, const void *out_dev,
                                  int64_t ld_out, unsigned flags)
{
    const auto refuse = [fn](const char *text) { return BlockCall{set_error(G4S_ERR_INVALID, "%s: %s", fn, text), false}; };
    if (k < 0 || k > G4S_TRSV_MAX_RHS) return refuse("k is negative or above G4S_TRSV_MAX_RHS");
    if ((flags & ~G4S_TRSV_COL_MAJOR) != 0u) return refuse("flags other than G4S_TRSV_COL_MAJOR");
    if (n == 0 || k == 0) return BlockCall{G4S_OK, false};
    if (!in_dev || !out_dev) return BlockCall{set_error(G4S_ERR_INVALID, "%s: %s or %s is NULL", fn, in, out), false};
    const int64_t need = (flags & G4S_TRSV_COL_MAJOR) ? n : k;
    if (ld_in < need || ld_out < need) return refuse("a leading dimension is too small: ld >= k row-major, ld >= n column-major");
    if (in_dev == out_dev && ld_in != ld_out) return BlockCall{set_error(G4S_ERR_INVALID, "%s: %s is %s with another leading dimension", fn, out, in), false};
    return BlockCall{G4S_OK, true};
}

} // namespace g4s
