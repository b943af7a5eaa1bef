// Host test of the launch list, the two stride rules and the launch walk of the level-scheduled calls (g4s_amd/csrc/level_schedule.hpp), built with
// -fsanitize=address,undefined by tests/test_level_schedule_cpu.py. The pinned values follow from the rules of include/g4s.h: a level of at most
// G4S_TRSV_CHAIN_WIDTH rows is narrow, a run of narrow levels is cut every G4S_TRSV_CHAIN_LEVELS levels; and from the two stride rules as
// level_schedule.hpp states them.
#include "level_schedule.hpp"
#include "g4s.h"
#include <cstdio>
#include <string>
#include <vector>

using g4s::LevelSchedule;
using g4s::TrLaunch;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

constexpr int W = G4S_TRSV_CHAIN_WIDTH, L = G4S_TRSV_CHAIN_LEVELS;

// the levels + 1 offsets of levels of the given widths: exactly as long as the rule may read
static std::vector<int> offsets(const std::vector<int> &widths)
{
    std::vector<int> loff(1, 0);
    for (int w : widths) loff.push_back(loff.back() + w);
    return loff;
}

// the launch list as text: c[lo,hi) a chain, l[lo,hi) a level
static std::string plan(const std::vector<int> &widths, bool no_chains = false)
{
    const std::vector<int> loff = offsets(widths);
    std::string s;
    for (const TrLaunch &x : g4s::trsv_launches(loff.data(), (int)widths.size(), W, L, no_chains))
        s += std::string(x.chain ? "c[" : "l[") + std::to_string(x.level_lo) + "," + std::to_string(x.level_hi) + ")";
    return s;
}

static void a_the_constants()
{
    CHECK(W == 256 && L == 1024 && g4s::kLevelWg == 256);
}

static void b_no_level_and_one_level()
{
    CHECK(plan({}) == "" && plan({}, true) == "");
    CHECK(plan({5}) == "c[0,1)");                                            // a piece of one level is a chain
    CHECK(plan({300}) == "l[0,1)");
}

// (c) a run of narrow levels is cut from its first level on into pieces of at most L levels
static void c_runs_of_narrow_levels()
{
    const std::string cut = "c[0," + std::to_string(L) + ")";
    CHECK(plan(std::vector<int>(L - 1, 1)) == "c[0," + std::to_string(L - 1) + ")");
    CHECK(plan(std::vector<int>(L, 1)) == cut);
    CHECK(plan(std::vector<int>(L + 1, 1)) == cut + "c[" + std::to_string(L) + "," + std::to_string(L + 1) + ")");
    CHECK(plan(std::vector<int>(2 * L + 1, W)) == cut + "c[" + std::to_string(L) + "," + std::to_string(2 * L) + ")c[" + std::to_string(2 * L) + "," + std::to_string(2 * L + 1) + ")");
}

static void d_narrow_and_wide_alternate()
{
    CHECK(plan({3, 300, 4, 257, 256, 1}) == "c[0,1)l[1,2)c[2,3)l[3,4)c[4,6)");
    CHECK(plan({300, 3, 300}) == "l[0,1)c[1,2)l[2,3)");
    CHECK(plan({300, 400}) == "l[0,1)l[1,2)");                               // wide levels never join
}

static void e_the_width_limit()
{
    CHECK(plan({W - 1}) == "c[0,1)" && plan({W}) == "c[0,1)" && plan({W + 1}) == "l[0,1)");
    CHECK(plan({W - 1, W, W + 1}) == "c[0,2)l[2,3)");
    CHECK(plan({W + 1, W, W - 1}) == "l[0,1)c[1,3)");
}

static void f_no_chains()
{
    CHECK(plan({3, 300, 4}, true) == "l[0,1)l[1,2)l[2,3)");
    CHECK(plan(std::vector<int>(3, 1), true) == "l[0,1)l[1,2)l[2,3)");
}

// (g) the solve's stride doubles at an average of 8, 16, … 256 entries a row; the average rounds down
static void g_trsv_stride()
{
    CHECK(g4s::trsv_stride(0, 0) == 1 && g4s::trsv_stride(0, 1000) == 1);    // no rows: nothing divides
    CHECK(g4s::trsv_stride(5, 0) == 1);
    int want = 1;
    for (int avg = 8; avg <= 256; avg *= 2, want *= 2) {
        CHECK(g4s::trsv_stride(1, avg - 1) == want && g4s::trsv_stride(1, avg) == 2 * want);
        CHECK(g4s::trsv_stride(3, 3LL * avg - 1) == want && g4s::trsv_stride(3, 3LL * avg) == 2 * want);
    }
    CHECK(want == 64);
    CHECK(g4s::trsv_stride(1, 257) == 64 && g4s::trsv_stride(1, 1LL << 40) == 64 && g4s::trsv_stride(1 << 30, 1LL << 40) == 64);
    CHECK(g4s::trsv_stride(300, 5100) == 4);                                 // strided_tiles of tests/trsv_ref.py: 64 rows a workgroup
    CHECK(g4s::trsv_stride(260, 66820) == 64);                               // wave_tiles: one row a wave
}

// (h) the factorisation's stride is 1 without a pivot and doubles at an average of 1, 2, … 32 lower entries a row: one wave a row from 32 on
static void h_ilu_stride()
{
    CHECK(g4s::ilu_stride(0, 0) == 1 && g4s::ilu_stride(0, 1000) == 1);
    CHECK(g4s::ilu_stride(7, 0) == 1 && g4s::ilu_stride(7, 6) == 1 && g4s::ilu_stride(7, 7) == 2);
    int want = 2;
    for (int avg = 2; avg <= 32; avg *= 2, want *= 2) {
        CHECK(g4s::ilu_stride(1, avg - 1) == want && g4s::ilu_stride(1, avg) == 2 * want);
        CHECK(g4s::ilu_stride(3, 3LL * avg - 1) == want && g4s::ilu_stride(3, 3LL * avg) == 2 * want);
    }
    CHECK(want == 64);
    CHECK(g4s::ilu_stride(1, 63) == 64 && g4s::ilu_stride(1, 64) == 64 && g4s::ilu_stride(1, 1LL << 40) == 64);
    CHECK(g4s::ilu_stride(300, 4800) == 32);                                 // strided_tiles of tests/ilu_ref.py: 8 rows a workgroup
}

// (i) the walk: a schedule of seven levels; what is called, in which order, with which grid, and that the tiles of WG / stride rows cover every row
// of every level once
static void i_the_walk()
{
    const std::vector<int> widths = {3, 2, 700, 1, 300, 260, 5}, per_row = {0, 1, 17, 700, 3, 257, 2};
    LevelSchedule S;
    S.loff_host = offsets(widths);
    S.lent_host.assign(1, 0);
    for (size_t l = 0; l < widths.size(); ++l) S.lent_host.push_back(S.lent_host.back() + widths[l] * per_row[l]);
    S.levels = (int)widths.size();
    S.launches = g4s::trsv_launches(S.loff_host.data(), S.levels, W, L, false);
    const int n = S.loff_host.back();
    for (int rule = 0; rule < 2; ++rule) {
        std::string calls;
        std::vector<int> seen((size_t)n, 0);
        const auto chain = [&](int level_lo, int level_hi) {
            calls += "c" + std::to_string(level_lo) + "-" + std::to_string(level_hi) + " ";
            for (int p = S.loff_host[level_lo]; p < S.loff_host[level_hi]; ++p) seen[p] += 1;
        };
        const auto level = [&](int lo, int hi, int stride, int grid) {
            const int rows = g4s::kLevelWg / stride;
            calls += "l" + std::to_string(lo) + "-" + std::to_string(hi) + "/" + std::to_string(stride) + "x" + std::to_string(grid) + " ";
            CHECK(stride >= 1 && stride <= 64 && (stride & (stride - 1)) == 0);
            CHECK(grid == (hi - lo + rows - 1) / rows && grid >= 1);
            for (int g = 0; g < grid; ++g)
                for (int p = lo + g * rows; p < lo + (g + 1) * rows && p < hi; ++p) seen[p] += 1;
        };
        if (rule == 0) {
            g4s::for_each_launch(S, g4s::trsv_stride, chain, level);
            CHECK(calls == "c0-2 l5-705/4x11 c3-4 l706-1006/1x2 l1006-1266/64x65 c6-7 ");
        } else {
            g4s::for_each_launch(S, g4s::ilu_stride, chain, level);
            CHECK(calls == "c0-2 l5-705/32x88 c3-4 l706-1006/4x5 l1006-1266/64x65 c6-7 ");
        }
        for (int p = 0; p < n; ++p) CHECK(seen[p] == 1);
    }
    LevelSchedule none;                                                      // a plan of n == 0
    g4s::for_each_launch(none, g4s::trsv_stride, [&](int, int) { CHECK(false); }, [&](int, int, int, int) { CHECK(false); });
    S.launches = g4s::trsv_launches(S.loff_host.data(), S.levels, W, L, true);
    int levels = 0;
    g4s::for_each_launch(S, g4s::trsv_stride, [&](int, int) { CHECK(false); }, [&](int lo, int hi, int, int) { CHECK(lo == S.loff_host[levels] && hi == S.loff_host[levels + 1]); ++levels; });
    CHECK(levels == 7);
}

int main()
{
    a_the_constants();
    b_no_level_and_one_level();
    c_runs_of_narrow_levels();
    d_narrow_and_wide_alternate();
    e_the_width_limit();
    f_no_chains();
    g_trsv_stride();
    h_ilu_stride();
    i_the_walk();
    if (g_failed) { std::fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    std::puts("level_schedule_test: ok");
    return 0;
}
