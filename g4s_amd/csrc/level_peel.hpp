// level_peel.hpp — what the level peels share (kcore.hip: vertices by degree; ktruss.hip: edges by triangle support) on top of frontier.hpp
// and call_util.hpp: the end of their scan and peel kernels on the PeelState words of their state blocks (step_batch.hpp; the queue words are flipped by
// flip_queue of frontier.hpp, as color.hip's and trsv.hip's are), and the host loop that enqueues PeelSchedule's batches. The kernels themselves, what
// an item and its row are, and the opening launches stay with the two files.
#pragma once
#include "frontier.hpp"
#include "call_util.hpp"
#include <climits>

namespace {

enum { KIND_SCAN = 0, KIND_PEEL = 1 };

// The end of a step kernel: the block's shares of the sums and of the minimum, then the ticket; the last block to arrive turns the page (turn_page).
// grid_cap: a built frontier with more entries asks for a larger peel grid (stop = 4); level_cap: a scan that finds every item above it ends the
// peeling (stop = 2); items(): how many there are — a peel that appends nothing once the queue holds them all has removed everything (stop = 1).
template <typename Items>
__device__ __forceinline__ void finish_step(g4s::PeelState *st, long long len_sum, long long walked, int mn, int kind, long long grid_cap, int level_cap, Items items)
{
    __shared__ long long s_len[WG / 64], s_walk[WG / 64];
    __shared__ int s_min[WG / 64];
    len_sum = wave_sum(len_sum);
    walked = wave_sum(walked);
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0) { s_len[threadIdx.x >> 6] = len_sum; s_walk[threadIdx.x >> 6] = walked; s_min[threadIdx.x >> 6] = mn; }
    if (!turn_page(&st->tickets, [&] {
        long long ls = 0, ws = 0;
        int m = INT_MAX;
        for (int w = 0; w < WG / 64; ++w) { ls += s_len[w]; ws += s_walk[w]; m = s_min[w] < m ? s_min[w] : m; }
        if (ls) atomicAdd((unsigned long long *)&st->edges_next, (unsigned long long)ls);
        if (ws) atomicAdd(&st->edges_walked, (unsigned long long)ws);
        // the word only decreases while the kernel runs, so a value read earlier is too large and costs one atomic; read at agent scope, past the
        // copy of the state line this CU has held since the kernel's first lines
        if (m < __hip_atomic_load(&st->min_left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&st->min_left, m);
    })) return;
    const int m = atomicAdd(&st->min_left, 0);
    const QueueFlip f = flip_queue(st);
    st->min_left = INT_MAX;
    int stop = f.entries > grid_cap ? 4 : 0;
    if (kind == KIND_SCAN) {
        st->scans += 1;
        if (f.appended == 0) {                                     // items are left (a scan does not run otherwise), all above the level: m is one's count
            st->level = m;
            if (m >= level_cap) stop = 2;
        } else {
            st->levels += 1;
            st->top_level = st->level;
        }
    } else {
        st->round += 1;
        if (f.appended == 0 && st->end >= items()) stop = 1;       // end: the append counter this kernel left
    }
    st->stop = stop;
}

// The batches of a level peel behind its opening launches; returns behind a wait on the stream of `reads` with *h the final state. A batch is
// PeelSchedule's launches and the caller's finish kernel (a no-op until stop is 1 or 2), then one read. scan(grid_cap), peel(grid, grid_cap, resume)
// and finish() launch the caller's kernels; entry_weight: what a frontier entry costs in the plain entries StepGrid counts.
template <typename State, typename Scan, typename Peel, typename Finish>
int run_level_peel(const g4s::StepGrid &sized, int first_batch, long long entry_weight, Scan scan, Peel peel, Finish finish, g4s::ReadScope &reads, const State *st,
                   State *h, Counts *cnt)
{
    g4s::PeelSchedule plan(first_batch);
    for (;;) {
        const int grid = plan.know ? sized.grid(entry_weight * (h->edges_cur + (h->end - h->head) + h->n_hub_cur)) : sized.max_grid;
        const long long grid_cap = sized.cap(grid) / entry_weight;
        const int start = plan.start(*h);
        for (int b = 0; b < plan.batch; ++b) {
            if (plan.is_peel(start, b)) peel(grid, grid_cap, plan.resumes(start, b, *h) ? 1 : 0);
            else scan(grid_cap);
        }
        finish();
        G4S_HIP_TRY(hipGetLastError());
        cnt->launches += plan.batch + 1;
        if (plan.know && h->stop == 4) cnt->resumes += 1;
        G4S_HIP_TRY(reads.fetch(*h, st));
        cnt->waits += 1;
        if (h->invalid || h->stop == 1 || h->stop == 2) return G4S_OK;
        plan.seen(*h);
    }
}

} // namespace
