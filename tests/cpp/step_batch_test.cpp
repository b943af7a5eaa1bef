// Host test of g4s::StepGrid and the constants of the stepped loops (g4s_amd/csrc/step_batch.hpp), built with -fsanitize=address,undefined by
// tests/test_step_batch_cpu.py. The pinned values follow from the constants: 2048 entries per workgroup, a cap of 8 times what the grid was sized for.
#include "step_batch.hpp"
#include <climits>
#include <cstdio>

using g4s::StepGrid;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static void a_the_constants()
{
    CHECK(g4s::kEdgesPerWg == 2048 && g4s::kGridGrowth == 8 && g4s::kBatchMax == 64 && g4s::kMinGrid == 8);
}

// (b) the clamp and the cap of a grid between 8 and 512 workgroups
static void b_grid_and_cap()
{
    const StepGrid g(8, 512);
    CHECK(g.min_grid == 8 && g.max_grid == 512);
    CHECK(g.grid(0) == 8 && g.grid(1) == 8 && g.cap(8) == 131072);
    CHECK(g.grid(8 * 2048 + 2047) == 8 && g.grid(9 * 2048) == 9);            // the quotient rounds down
    CHECK(g.grid(262144) == 128 && g.cap(128) == 2097152);
    CHECK(g.grid(512 * 2048 - 1) == 511 && g.cap(511) == 511LL * 2048 * 8);
    CHECK(g.grid(512 * 2048) == 512 && g.grid(512 * 2048 + 1) == 512 && g.cap(512) == LLONG_MAX);
    CHECK(g.grid(LLONG_MAX) == 512);                                         // no overflow on the way to the clamp
    CHECK(g.cap(g.grid(131072)) == 64LL * 2048 * 8);
}

// (c) a largest grid below the smallest (a graph with less work than 8 workgroups' worth, betweenness.hip): both are the smallest, and that grid is
// the largest one, so nothing outgrows it
static void c_a_small_largest_grid_is_clipped()
{
    const StepGrid g(8, 3);
    CHECK(g.min_grid == 8 && g.max_grid == 8);
    CHECK(g.grid(0) == 8 && g.grid(1 << 30) == 8 && g.cap(8) == LLONG_MAX);
    const StepGrid one(8, 8);
    CHECK(one.grid(100000) == 8 && one.cap(8) == LLONG_MAX);
    const StepGrid low(1, 512);                                              // k-core's A/B switch lowers the smallest grid
    CHECK(low.grid(0) == 1 && low.cap(1) == 16384 && low.grid(5000) == 2);
}

static void d_batches_double_up_to_64()
{
    int b = 16;
    CHECK((b = StepGrid::next_batch(b)) == 32);
    CHECK((b = StepGrid::next_batch(b)) == 64);
    CHECK((b = StepGrid::next_batch(b)) == 64);
    CHECK(StepGrid::next_batch(8) == 16 && StepGrid::next_batch(33) == 64 && StepGrid::next_batch(1) == 2);
}

int main()
{
    a_the_constants();
    b_grid_and_cap();
    c_a_small_largest_grid_is_clipped();
    d_batches_double_up_to_64();
    if (g_failed) { std::fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    std::puts("step_batch_test: ok");
    return 0;
}
