// trsv.hpp — what the analysis and the solve of g4s_sptrsv share (trsv.hip), in plain C++ (no HIP): the device-resident state of the
// level peel and the launch list of a solve — the chaining rule of include/g4s.h, which tests/trsv_ref.py restates.
#pragma once
#include <vector>
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

// One launch of a solve: the levels [level_lo, level_hi). A chain is one workgroup that steps through its levels behind a barrier; a level
// that is not in a chain is one launch over its rows (trsv_stride: how many a workgroup takes).
struct TrLaunch {
    int level_lo, level_hi;
    bool chain;
};

// The rule (g4s.h): a level of at most chain_width rows is narrow. A maximal run of consecutive narrow levels is cut, from its first level on, into
// pieces of at most chain_levels levels; every piece is one chain — one launch —, a piece of one level included. Every other level is one launch.
// no_chains: every level is one launch and there is no chain. loff: the levels + 1 offsets of the levels in the (level, row) layout.
inline std::vector<TrLaunch> trsv_launches(const int *loff, int levels, int chain_width, int chain_levels, bool no_chains)
{
    std::vector<TrLaunch> out;
    for (int l = 0; l < levels;) {
        const bool narrow = !no_chains && loff[l + 1] - loff[l] <= chain_width;
        int e = l + 1;
        if (narrow)
            while (e < levels && e - l < chain_levels && loff[e + 1] - loff[e] <= chain_width) ++e;
        out.push_back(TrLaunch{l, e, narrow});
        l = e;
    }
    return out;
}

// How far apart the threads that own a row sit in a level launch (a power of two, 1 … 64): a level of `rows` rows and `entries` off-diagonal and
// diagonal entries. Short rows go one per lane (stride 1). A wave takes its rows above G4S_TRSV_WAVE_ROW entries one after another, so from an average
// of 8 entries a row on a wave gets fewer rows — avg / 4 apart, rounded down to a power of two —, and from 256 on one row each. It decides which
// thread sums a row, never how: x does not depend on it.
inline int trsv_stride(int rows, long long entries)
{
    const long long avg = rows > 0 ? entries / rows : 0;
    int s = 1;
    while (s < 64 && 2LL * s <= avg / 4) s *= 2;
    return s;
}

// What g4s_ilu0 (ilu.hip) takes from the plan of the lower triangle: the rows in (level, row) order and the level offsets on the device, the level
// offsets, the entry offsets of the levels and the launch list on the host. All of it lives as long as the plan. A plan of n == 0 has no level.
struct TrSchedule {
    const int *rowid, *loff;
    const int *loff_host, *lent_host;
    const std::vector<TrLaunch> *launches;
    int levels;
};
TrSchedule trsv_schedule(const g4s_trsv_s *T);

} // namespace g4s
