// Host test of g4s::StepGrid, g4s::PeelSchedule and the constants of the stepped loops (g4s_amd/csrc/step_batch.hpp), built with
// -fsanitize=address,undefined by tests/test_step_batch_cpu.py. The pinned values follow from the constants: 2048 entries per workgroup, a cap of 8
// times what the grid was sized for; and, for the schedule, from the batch loop that g4s_kcore and g4s_ktruss ran before they shared it.
#include "step_batch.hpp"
#include <climits>
#include <cstdio>
#include <string>

using g4s::PeelSchedule;
using g4s::PeelState;
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

// the kinds of a batch's launches from position `start`, 's' a scan and 'p' a peel
static std::string kinds(const PeelSchedule &p, int start)
{
    std::string k;
    for (int b = 0; b < p.batch; ++b) k += p.is_peel(start, b) ? 'p' : 's';
    return k;
}

// (e) a fresh schedule: units of two scans and two peels, from the scans unless a frontier is waiting — which a schedule that has read nothing cannot know
static void e_a_fresh_schedule()
{
    const PeelSchedule p(16);
    CHECK(p.batch == 16 && p.peels == 2 && !p.know);
    CHECK(kinds(p, 0) == "ssppssppssppsspp");                               // 8 scans and 8 peels
    CHECK(kinds(p, 2) == "ppssppssppssppss");
    PeelState h{};
    CHECK(p.start(h) == 0);
    h.head = 0; h.end = 5;
    CHECK(p.start(h) == 0);                                                  // not known yet
}

// (f) only launch 0 of a batch can resume: when it is a peel, the state is known, and the last read saw stop == 4
static void f_the_resume()
{
    PeelSchedule p(16);
    PeelState h{};
    h.end = 5; h.stop = 4;
    for (int b = 0; b < 16; ++b) CHECK(!p.resumes(2, b, h));                 // nothing read yet
    p.seen(h);
    CHECK(p.know && p.start(h) == 2);
    CHECK(p.resumes(2, 0, h));
    for (int b = 1; b < p.batch; ++b) CHECK(!p.resumes(2, b, h));
    CHECK(!p.resumes(0, 0, h));                                              // launch 0 is a scan
    for (int stop : {0, 1, 2, 3, 5}) { h.stop = stop; CHECK(!p.resumes(2, 0, h)); }
    h.stop = 4; h.end = h.head;
    CHECK(p.start(h) == 0);                                                  // no frontier waits: begin with the scans
}

// (g) the update behind a read: the batch stays for the first read and doubles from the second on; peels = rounds per level of the last batch,
// rounded up, and one to spare, in [2, batch − 2]
static void g_the_next_batch()
{
    PeelSchedule p(16);
    PeelState h{};
    h.levels = 3; h.round = 9;
    p.seen(h);
    CHECK(p.batch == 16 && p.peels == 4 && p.know);                          // (9 + 2) / 3 + 1
    CHECK(kinds(p, 0) == "ssppppssppppsspp");
    h.levels = 3; h.round = 40;
    p.seen(h);
    CHECK(p.batch == 32 && p.peels == 30);                                   // dl = max(0, 1), dr = 31: 32, clamped to batch − 2
    CHECK(kinds(p, 2) == std::string(30, 'p') + "ss");
    h.levels = 50; h.round = 41;                                             // many levels, one round: the floor
    p.seen(h);
    CHECK(p.batch == 64 && p.peels == 2);
    for (int i = 0; i < 4; ++i) {
        h.levels += i; h.round += 1000 * i;
        p.seen(h);
        CHECK(p.batch == 64 && p.peels >= 2 && p.peels <= 62);
    }
    CHECK(p.peels == 62);
    PeelSchedule q(4);                                                       // the smallest batch an A/B build may set: batch − 2 is the floor itself
    h = PeelState{};
    h.round = 100;
    q.seen(h);
    CHECK(q.batch == 4 && q.peels == 2);
}

int main()
{
    a_the_constants();
    b_grid_and_cap();
    c_a_small_largest_grid_is_clipped();
    d_batches_double_up_to_64();
    e_a_fresh_schedule();
    f_the_resume();
    g_the_next_batch();
    if (g_failed) { std::fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    std::puts("step_batch_test: ok");
    return 0;
}
