// level_schedule.hpp — the host side of a level-scheduled call (trsv.hip: the solve; ilu.hip: the factorisation), in plain C++ (no HIP:
// tests/cpp/level_schedule_test.cpp runs it on the host under a sanitizer): the (level, row) schedule an analysis leaves, the launch list — the
// chaining rule of include/g4s.h, which tests/trsv_ref.py restates —, the rules that spread a level's rows over the threads of its launch, and the
// walk that turns the list into launches. level_tile.hpp is the device side.
#pragma once
#include <vector>
namespace g4s {

constexpr int kLevelWg = 256;   // threads of a workgroup of a level launch and of a chain (WG, common.hpp; level_tile.hpp asserts it)

// One launch: the levels [level_lo, level_hi). A chain is one workgroup that steps through its levels behind a barrier; a level that is not in a
// chain is one launch over its rows (the stride rules below: how many a workgroup takes).
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

// How far apart the threads that own a row sit in a level launch of the solve (a power of two, 1 … 64): a level of `rows` rows and `entries`
// off-diagonal and diagonal entries. Short rows go one per lane (stride 1). A wave takes its rows above G4S_TRSV_WAVE_ROW entries one after another,
// so from an average of 8 entries a row on a wave gets fewer rows — avg / 4 apart, rounded down to a power of two —, and from 256 on one row each.
// It decides which thread sums a row, never how: x does not depend on it.
inline int trsv_stride(int rows, long long entries)
{
    const long long avg = rows > 0 ? entries / rows : 0;
    int s = 1;
    while (s < 64 && 2LL * s <= avg / 4) s *= 2;
    return s;
}

// The same for the factorisation: a level of `rows` rows whose strictly lower triangle holds `lower_entries` entries. A row's k loop is sequential
// and every step of it waits for a load, so rows are spread over waves sooner than the solve spreads them: from one pivot a row on, twice as far per
// doubling, one wave a row from 64. It decides who factorises a row, never how: the bits of include/g4s.h do not depend on it.
inline int ilu_stride(int rows, long long lower_entries)
{
    const long long avg = rows > 0 ? lower_entries / rows : 0;
    int s = 1;
    while (s < 64 && s <= avg) s *= 2;
    return s;
}

// What an analysis leaves for the launches (g4s_trsv_s owns it; g4s_ilu0 borrows the lower plan's through trsv_schedule and it lives as long as that
// plan): the rows in (level, row) order and the level offsets on the device; on the host the level offsets, for the grids of the level launches, the
// entry offsets of the levels, for their strides, and the launch list. A plan of n == 0 has no level.
struct LevelSchedule {
    int *rowid = nullptr, *loff = nullptr;
    std::vector<int> loff_host, lent_host;
    std::vector<TrLaunch> launches;
    int levels = 0;
};

// The launches of a schedule, in order: chain(level_lo, level_hi) for a chain — one workgroup —, level(lo, hi, stride, grid) for a level that is
// not in one: rows [lo, hi) of the layout, stride = stride_of(rows, entries of the level), kLevelWg / stride rows a workgroup, `grid` workgroups.
// Calls and nothing else: what the callables enqueue is what a graph captures.
template <typename StrideOf, typename Chain, typename Level>
void for_each_launch(const LevelSchedule &S, StrideOf stride_of, Chain chain, Level level)
{
    for (const TrLaunch &L : S.launches) {
        if (L.chain) {
            chain(L.level_lo, L.level_hi);
        } else {
            const int lo = S.loff_host[L.level_lo], hi = S.loff_host[L.level_hi];
            const int stride = stride_of(hi - lo, (long long)S.lent_host[L.level_hi] - S.lent_host[L.level_lo]);
            const int rows = kLevelWg / stride;
            level(lo, hi, stride, (hi - lo + rows - 1) / rows);
        }
    }
}

} // namespace g4s
