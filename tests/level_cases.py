"""Inputs for the level-scheduled calls — g4s_sptrsv_* (g4s_amd/csrc/trsv.hip) and g4s_ilu0_* (g4s_amd/csrc/ilu.hip) over their shared frame
(level_schedule.hpp, level_tile.hpp, frontier.hpp, step_batch.hpp) — that sit ON the edges of that frame: both sides of every doubling of the two stride
rules in a level launch of several workgroups, a tile that holds lane, wave and hub rows at once with the hubs owned by threads other than 0 in a
workgroup other than 0, every chain stride, every main-loop/tail split of the strided sums, the pass boundaries of the layout's radix sort, columns of
the transposed pattern at and above the hub cut, and a frontier that outgrows the first grid of the analysis peel (stop == 4 and the resume).
Plus a numpy restatement of every one of those rules and `facts(case, cus)`, which derives from the matrix alone what each launch, tile and frontier of
a case looks like, so that tests/test_level_cases_cpu.py can hold every case against the hand-written `declared` beside its builder —
tests/test_trsv_limits_gpu.py and tests/test_ilu_limits_gpu.py then run the cases. The levels, the (level, id) schedule and the launch plan are
tests/trsv_ref.py's (levels, schedule, launch_plan), not restated again.
numpy only: no GPU, no torch."""
import functools
from typing import Callable, NamedTuple

import numpy as np

from tests import ilu_ref as il
from tests import trsv_ref as tr

# ---- the limits, each beside the source line it mirrors
WG = 256                                         # level_schedule.hpp: `constexpr int kLevelWg = 256;` (level_tile.hpp: `static_assert(g4s::kLevelWg == WG, …)`)
HUB_CUT = 4096                                   # frontier.hpp: `constexpr int kHubCut = 4096;` — a column of the transposed pattern above it is a hub of the peel,
#                                                  and trsv.hip: `deal_tile<kWaveRow, kHubCut>` — a row of the solve above it is the workgroup's
TRSV_WAVE_ROW = 32                               # g4s.h: `#define G4S_TRSV_WAVE_ROW 32`; trsv.hip: `constexpr int kWaveRow = G4S_TRSV_WAVE_ROW;`
ILU_LANE_ROW, ILU_WAVE_ROW = 8, 512              # g4s.h: `G4S_ILU0_LANE_ROW 8`, `G4S_ILU0_WAVE_ROW 512`; ilu.hip: `deal_tile<kLaneRow, kWaveRow>`
EDGES_PER_WG = 2048                              # step_batch.hpp: `constexpr long long kEdgesPerWg = 2048;`
GRID_GROWTH = 8                                  # step_batch.hpp: `constexpr long long kGridGrowth = 8;`
MIN_GRID = 8                                     # step_batch.hpp: `constexpr int kMinGrid = 8;`
BATCH = 16                                       # trsv.hip: `constexpr int kBatch = 16;`
BATCH_MAX = 64                                   # step_batch.hpp: `constexpr int kBatchMax = 64;`
NO_CAP = 2**63 - 1                               # LLONG_MAX
CUS = (1, 4, 5, 256, 304)                        # the CU counts the CPU test walks: 2·cus below, at and above kMinGrid, and two real devices


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def trsv_stride(rows, entries):
    """level_schedule.hpp: `avg = rows > 0 ? entries / rows : 0; int s = 1; while (s < 64 && 2LL * s <= avg / 4) s *= 2;`"""
    avg = int(entries) // int(rows) if rows > 0 else 0
    s = 1
    while s < 64 and 2 * s <= avg // 4:
        s *= 2
    return s


def ilu_stride(rows, lower_entries):
    """level_schedule.hpp: `avg = rows > 0 ? lower_entries / rows : 0; int s = 1; while (s < 64 && s <= avg) s *= 2;`"""
    avg = int(lower_entries) // int(rows) if rows > 0 else 0
    s = 1
    while s < 64 and s <= avg:
        s *= 2
    return s


def chain_stride(width):
    """level_tile.hpp, for_chain_levels: `int stride = 64; while (stride > 1 && WG / stride < hi - lo) stride >>= 1;`"""
    s = 64
    while s > 1 and WG // s < width:
        s >>= 1
    return s


def level_launch(rows, stride):
    """(rows a workgroup, grid, rows of the last tile). level_schedule.hpp, for_each_launch: `const int rows = kLevelWg / stride;` and
    `level(lo, hi, stride, (hi - lo + rows - 1) / rows)`; level_tile.hpp, level_tile_bounds: `std::min<long long>(hi, t0 + WG / stride)`"""
    per = WG // stride
    grid = _ceil_div(rows, per)
    return per, grid, rows - (grid - 1) * per


def row_class(m, lane_cut, wave_cut):
    """level_tile.hpp, deal_tile: `if (have && r.m <= kLaneCut) lane_row(r);`, `__ballot(r.m > kLaneCut && r.m <= kWaveCut)`, `if (r.m > kWaveCut) s_hub[…] = t;`"""
    return "lane" if m <= lane_cut else "wave" if m <= wave_cut else "hub"


def step_max_grid(cus):
    """trsv.hip, peel: `const g4s::StepGrid sized(g4s::kMinGrid, 2 * cus);`; step_batch.hpp: `max_grid(std::max(lo, hi))`"""
    return max(MIN_GRID, 2 * cus)


def step_grid(work, cus):
    """step_batch.hpp, StepGrid::grid: `std::max((long long)min_grid, std::min((long long)max_grid, work / kEdgesPerWg))`"""
    return max(MIN_GRID, min(step_max_grid(cus), int(work) // EDGES_PER_WG))


def step_cap(grid, cus):
    """step_batch.hpp, StepGrid::cap: `grid == max_grid ? LLONG_MAX : (long long)grid * kEdgesPerWg * kGridGrowth`"""
    return NO_CAP if grid == step_max_grid(cus) else grid * EDGES_PER_WG * GRID_GROWTH


def next_batch(batch):
    """step_batch.hpp, StepGrid::next_batch: `std::min(kBatchMax, 2 * batch)`"""
    return min(BATCH_MAX, 2 * batch)


def bits_of(v):
    """trsv.hip: `int b = 1; while (b < 31 && (v >> b) != 0) ++b; return b;`"""
    b = 1
    while b < 31 and (v >> b) != 0:
        b += 1
    return b


def sort_passes(levels):
    """trsv.hip, layout: `3 * ((bits_of(levels - 1) + 3) / 4)` launches: a pass sorts four bits of the key"""
    return (bits_of(levels - 1) + 3) // 4


# ------------------------------------------------------------------------------------------------------------------------------- the model
def _structure(mat, lower, unit):
    """(off-diagonal triangle entries per row, dependents per column — the rows of the transposed pattern —, kept diagonal entries per row, level)"""
    n, rp, ci, va = mat
    rowid = np.repeat(np.arange(n), np.diff(rp))
    off = (ci < rowid) if lower else (ci > rowid)
    m = np.bincount(rowid[off], minlength=n)
    tlen = np.bincount(ci[off], minlength=n)
    d = np.zeros(n, np.int64) if unit else np.bincount(rowid[ci == rowid], minlength=n)
    return m, tlen, d, tr.levels(*mat, lower, unit)


def _tile(lens, stride, cuts):
    """deal_tile on the rows of one tile, lens their class lengths in layout order: thread j·stride owns row j.
    ((lane, wave, hub) rows, the most wave rows any one wave takes, the owners of the hubs)"""
    cls = [row_class(int(v), *cuts) for v in lens]
    per_wave = np.bincount([j * stride // 64 for j, c in enumerate(cls) if c == "wave"], minlength=1)
    return (cls.count("lane"), cls.count("wave"), cls.count("hub")), int(per_wave.max()), tuple(j * stride for j, c in enumerate(cls) if c == "hub")


def _launches(lev, lens, entries, stride_of, cuts, no_chains):
    """The launches of for_each_launch on a schedule — ("chain", the stride of each of its levels) or ("level", stride, grid, rows of the last tile) —,
    and per tile (level, tile index — 0 in a chain) what _tile says. lens: the length that decides a row's class; entries: what the stride rule counts."""
    order, loff = tr.schedule(lev)
    out, tiles = [], {}
    for lo, hi, chain in tr.launch_plan(lev, no_chains):
        if chain:
            strides = tuple(chain_stride(int(loff[l + 1] - loff[l])) for l in range(lo, hi))
            out.append(("chain", strides))
            for l, s in zip(range(lo, hi), strides):
                tiles[(l, 0)] = _tile(lens[order[loff[l]:loff[l + 1]]], s, cuts)
        else:
            rows = order[loff[lo]:loff[lo + 1]]
            stride = stride_of(rows.size, int(entries[rows].sum()))
            per, grid, last = level_launch(rows.size, stride)
            out.append(("level", stride, grid, last))
            for w in range(grid):
                tiles[(lo, w)] = _tile(lens[rows[w * per:(w + 1) * per]], stride, cuts)
    return out, tiles


def peel(lev, tlen, cus, with_level=True):
    """The host loop of peel() in trsv.hip on the frontiers of a matrix — frontier l is level l: a row is appended by the step that walks its last column —
    and the launch and wait counts of the whole analysis around it."""
    width = np.bincount(lev)
    levels = width.size
    fe = np.bincount(lev, weights=tlen, minlength=levels).astype(np.int64)             # finish(): `atomicAdd(&st->edges_next, ls)`: every appended row's len, hubs included
    fh = np.bincount(lev, weights=tlen > HUB_CUT, minlength=levels).astype(np.int64)   # append_frontier: `if (want && len > kHubCut) … hubs_next[h] = v;`
    cur, stop, resumes, batches, grids, batch = 0, 0, 0, [], [], BATCH                 # behind the seed: frontier 0, `a.grid_cap = LLONG_MAX` stops nothing
    while stop != 1:                                                                  # `while (h->stop != 1)`
        grid = step_grid(fe[cur] + width[cur] + fh[cur], cus)                         # `sized.grid(h->edges_cur + (h->end - h->head) + h->n_hub_cur)`
        resumed = stop == 4                                                           # `const bool resumed = h->stop == 4;`
        cap = step_cap(grid, cus)                                                     # `a.grid_cap = sized.cap(grid);`
        resumes += resumed                                                            # `if (resumed) cnt->resumes += 1;`
        for b in range(batch):
            if not (stop == 0 or (stop == 4 and b == 0 and resumed)):                 # step_runs: `stop == 0 || (stop == 4 && resume)`, `a.resume = b == 0 && resumed`
                break
            cur += 1                                                                  # flip_queue: the frontier that was being built becomes the current one
            appended, entries = (int(width[cur]), int(fe[cur])) if cur < levels else (0, 0)
            stop = 1 if appended == 0 else 4 if entries > cap else 0                  # finish(): `f.appended == 0 ? 1 : f.entries > a.grid_cap ? 4 : 0`
        batches.append(batch)                                                         # `cnt->launches += batch; … cnt->waits += 1;`
        grids.append(grid)
        batch = next_batch(batch)
    launches = 4 + 5 + sum(batches) + 4 + 3 * sort_passes(levels) + 6                # open: 4; scan, scatter, seed: 5; layout: `4 + 3 * ((bits_of(levels - 1) + 3) / 4) + 6`
    waits = 1 + 1 + len(batches) + 1 + (1 if with_level else 0)
    return {"resumes": resumes, "launches": launches, "host_waits": waits, "batches": batches, "grids": grids, "sort_passes": sort_passes(levels),
            "frontier_entries": fe.tolist(), "frontier_hubs": {l: int(v) for l, v in enumerate(fh) if v}}


@functools.lru_cache(maxsize=None)
def _static(name, lower):
    """everything of facts() that does not depend on the CU count, computed once a case and triangle"""
    c = CASES[name]
    mat = matrix(name, lower)
    n, rp, ci, va = mat
    out = {}
    if c.kind == "solve":
        m, tlen, d, lev = _structure(mat, lower, False)
        for key, nc in (("", False), ("_no_chains", True)):
            out["launches" + key], tiles = _launches(lev, m, m + d, trsv_stride, (TRSV_WAVE_ROW, HUB_CUT), nc)
            out["tiles" + key] = tiles
    else:
        m, tlen, d, lev = _structure(mat, True, True)                                 # the lower plan of the handle: a unit diagonal, so its entries are the pivots
        stored = np.diff(rp)
        for key, nc in (("", False), ("_no_chains", True)):
            out["launches" + key], tiles = _launches(lev, stored, m, ilu_stride, (ILU_LANE_ROW, ILU_WAVE_ROW), nc)
            out["tiles" + key] = tiles
        _, tup, _, lup = _structure(mat, False, False)
        out["_upper"] = (lup, tup)
    cuts = (TRSV_WAVE_ROW, HUB_CUT) if c.kind == "solve" else (ILU_LANE_ROW, ILU_WAVE_ROW)
    lens = m if c.kind == "solve" else np.diff(rp)
    cls = np.array([("lane", "wave", "hub").index(row_class(int(v), *cuts)) for v in lens], np.int64)
    out["levels"] = int(lev.max()) + 1
    out["widths"] = np.bincount(lev).tolist()
    out["classes"] = {l: tuple(int(v) for v in np.bincount(cls[lev == l], minlength=3)) for l in range(out["levels"]) if np.any(cls[lev == l] > 0)}
    for key in ("", "_no_chains"):
        out["hubs" + key] = {k: v[2] for k, v in out["tiles" + key].items() if v[2]}
        out["waves" + key] = {l: max(v[1] for k, v in out["tiles" + key].items() if k[0] == l) for l in out["classes"]}
    out["_peel"] = (lev, tlen)
    return out


def facts(name, cus, lower=True):
    """What the frame does with a case on a device of `cus` compute units, from the matrix alone (lower = False: a solve case mirrored into its upper twin):
      levels, widths              the levels and their row counts
      launches[_no_chains]        per launch ("chain", strides) or ("level", stride, grid, rows of the last tile)
      tiles[_no_chains]           (level, tile) -> ((lane, wave, hub) rows, the most wave rows of one wave, the hubs' owner threads)
      hubs[_no_chains]            (level, tile) -> owner threads, the tiles with a hub only
      waves[_no_chains]           level -> the most wave rows of one wave in any tile, the levels of `classes` only
      classes                     level -> (lane, wave, hub) rows, the levels that hold more than lane rows
      frontier_entries, frontier_hubs   per level the entries of its rows of the transposed pattern; level -> its columns above kHubCut, where there are any
      resumes, launches_analysis, host_waits, batches, grids   the host loop of peel() and the analysis's counts around it (a level array asked for)
    An ILU case adds the same peel facts of the handle's upper plan under "upper"."""
    s = _static(name, lower)
    out = {k: v for k, v in s.items() if not k.startswith("_")}
    p = peel(*s["_peel"], cus)
    p["launches_analysis"] = p.pop("launches")
    out.update(p)
    if "_upper" in s:
        out["upper"] = peel(*s["_upper"], cus)
    return out


def ilu_analyses(name, cus):
    """peel() for the two solve plans of an ILU handle — the lower one with a unit diagonal, the upper one —, neither asked for a level array (ilu.hip, analyse)"""
    s = _static(name, True)
    return peel(*s["_peel"], cus, with_level=False), peel(*s["_upper"], cus, with_level=False)


# ------------------------------------------------------------------------------------------------------------------------------ the builders
def stack(base, levels, seed=40):
    """trsv_ref.long_rows for more than one level: `base` rows that store their diagonal only, then per entry of `levels` one level of rows, one row per
    count with that many off-diagonal entries (scaled as long_rows scales them, to keep x of size one). A row of the first list takes its columns among
    the base rows; a row of a later list takes one row of the level before it — a row above HUB_CUT entries all of them — and the rest among the base
    rows. Rows get ids in the order given, so position q of a list is position q of its level in the (level, id) layout."""
    rng = tr._rng(seed)
    rows = [[(i, tr._diag(rng))] for i in range(base)]
    prev = []
    for counts in levels:
        cur = []
        for q, m in enumerate(counts):
            assert 1 <= m <= base + len(prev), "a row of level 1 and above stores at least one off-diagonal entry"
            i = len(rows)
            own = [] if not prev else list(prev) if m > HUB_CUT else [prev[q % len(prev)]]
            cols = own + [int(c) for c in rng.permutation(base)[:m - len(own)]]
            rows.append([(c, tr._val(rng) / 8.0) for c in cols] + [(i, tr._diag(rng))])
            cur.append(i)
        prev = cur
    return tr.csr(rows)


def dense_column(k, seed=42):
    """row 0, then rows 1 … k that store (i, 0) and their diagonal: column 0 of the transposed pattern has k entries"""
    rng = tr._rng(seed)
    return tr.csr([[(0, tr._diag(rng))]] + [[(0, tr._val(rng)), (i, tr._diag(rng))] for i in range(1, k + 1)])


def hub_columns(seed=43):
    """Rows 0, 1, 2 (level 0) have 6000, 5000 and 4097 dependents, rows 3 … 9 (level 0) are ordinary columns; the 6000 rows of level 1 store column 0, the
    first 5000 of them column 1, the first 4097 column 2, and every second one an ordinary column; the first row of level 1 (id 10) has 4500 dependents of
    its own, the rows of level 2, of which every third also stores another row of level 1."""
    rng = tr._rng(seed)
    rows = [[(i, tr._diag(rng))] for i in range(10)]
    for q in range(6000):
        cols = [0] + ([1] if q < 5000 else []) + ([2] if q < 4097 else []) + ([3 + q % 7] if q % 2 else [])
        rows.append([(c, tr._val(rng) / 4.0) for c in cols] + [(10 + q, tr._diag(rng))])
    for q in range(4500):
        cols = [10] + ([11 + q] if q % 3 == 0 else [])
        rows.append([(c, tr._val(rng) / 4.0) for c in cols] + [(6010 + q, tr._diag(rng))])
    return tr.csr(rows)


def fan(R, seed=44):
    """row 0; rows 1 … 64 store (i, 0); R further rows each store columns 1 … 64 and their diagonal: the frontier behind the first step has 64 · R entries"""
    rng = tr._rng(seed)
    rows = [[(0, tr._diag(rng))]] + [[(0, tr._val(rng)), (i, tr._diag(rng))] for i in range(1, 65)]
    rows += [[(c, tr._val(rng) / 8.0) for c in range(1, 65)] + [(65 + q, tr._diag(rng))] for q in range(R)]
    return tr.csr(rows)


def ilu_stack(levels, short=64, tail=520, seed=41):
    """ilu_ref.strided_tiles for more than one level and rows of any stored length. Canonical rows, both triangles:
      `short` rows                 {i, i + 1, the first two columns of the tail}: level 0, and the only pivot rows of level 1 — pivot rows stay short
      levels[0]                    one more row of level 0 per entry nup: its diagonal and the first nup columns of the tail
      levels[k], k >= 1            one row per (nlow, nup): nlow pivots, its diagonal, the first nup columns of the tail. The pivots of a row of level 1 are
                                   the first nlow short rows; a row of a later level pivots on one row of the level before it — with more than LANE_ROW
                                   pivots on as many of them as it has room for — and on short rows for the rest
      `tail` rows                  their diagonal only, the last ids: the columns every upper part is made of
    Diagonally dominant (ilu_ref.dominant), so no pivot comes near zero and z stays of size one."""
    rng = tr._rng(seed)
    n = short + sum(len(l) for l in levels) + tail
    t0 = n - tail
    pat = [sorted({i, min(i + 1, short - 1), t0, t0 + 1}) for i in range(short)]
    pat += [[len(pat) + q] + list(range(t0, t0 + nup)) for q, nup in enumerate(levels[0])]
    prev = []
    for spec in levels[1:]:
        cur = []
        for q, (nlow, nup) in enumerate(spec):
            i = len(pat)
            own = [] if not prev else sorted(prev[:nlow]) if nlow > il.LANE_ROW else [prev[q % len(prev)]]
            assert 1 <= nlow <= short + len(own) and nup <= tail
            pat.append(list(range(nlow - len(own))) + own + [i] + list(range(t0, t0 + nup)))
            cur.append(i)
        prev = cur
    pat += [[i] for i in range(t0, n)]
    return tr.csr(il.dominant([[(j, float(rng.uniform(-1, 1))) for j in r] for r in pat]))


def arrow_both(n=4099, seed=45):
    """a dense first column and a dense last column, no dense row: row i stores {0, i, n − 1}"""
    rng = tr._rng(seed)
    return tr.csr(il.dominant([[(j, float(rng.uniform(-1, 1))) for j in sorted({0, i, n - 1})] for i in range(n)]))


# ------------------------------------------------------------------------------------------------------------------------------ the cases
class Case(NamedTuple):
    kind: str                # "solve": a lower triangle, also run mirrored as an upper one; "ilu": canonical rows, both triangles
    build: Callable          # () -> (n, rowptr, colids, values)
    declared: dict           # what the case claims to stand on, written by hand: the CPU test holds it against facts()
    peel: bool = False       # the GPU test also holds the analysis's resumes, launches and host_waits against facts()


R = 259                                          # rows of the level of a stride case: 257 and two more, so the last tile is three rows at every stride
GRID_OF = {1: 2, 2: 3, 4: 5, 8: 9, 16: 17, 32: 33, 64: 65}   # ⌈259 / (256 / stride)⌉; the last tile holds 259 − 256 = 3 rows whatever the stride
SPECIAL = [40, 50, 1, 32, 33]                    # the first rows of the level: two wave rows in wave 0 (up to stride 32), a lane row of one entry, both sides of WAVE_ROW
BASE = 320                                       # level 0 of a stride case: diagonal-only rows — the rows of 0 off-diagonal entries, a level launch of their own

# T -> (stride one entry below T·R, stride at T·R): both sides of every doubling of trsv_stride
TRSV_DOUBLING = {8: (1, 2), 16: (2, 4), 32: (4, 8), 64: (8, 16), 128: (16, 32), 256: (32, 64)}
# T -> the rows of each class in the level: up to T = 32 the padding rows are lane rows (at most 31 entries), from 64 on wave rows (at least 63)
TRSV_CLASSES = {8: (256, 3, 0), 16: (256, 3, 0), 32: (256, 3, 0), 64: (2, 257, 0), 128: (2, 257, 0), 256: (2, 257, 0)}
# T -> the most wave rows one wave takes (below, at): the three of SPECIAL while the padding is lane rows, 64 / stride of them once every padding row is one
TRSV_WAVES = {8: (3, 3), 16: (3, 3), 32: (3, 3), 64: (8, 4), 128: (4, 2), 256: (2, 1)}


def stride_counts(T, at):
    """off-diagonal entries per row of the level: SPECIAL, then 254 rows that share the rest evenly; `at` gives the last row one entry more"""
    rest = T * R - 1 - R - sum(SPECIAL)                                     # the level's entries, diagonal included, are T·R − 1
    q, r = divmod(rest, R - len(SPECIAL))
    counts = SPECIAL + [q + 1] * r + [q] * (R - len(SPECIAL) - r)
    if at:
        counts[-1] += 1
    return counts


def _stride_case(T, at):
    s = TRSV_DOUBLING[T][at]
    launches = [("level", 1, 2, BASE - WG), ("level", s, GRID_OF[s], 3)]    # both levels are wider than a chain: the same with chains on and off
    return Case("solve", lambda: stack(BASE, [stride_counts(T, at)]),
                {"widths": [BASE, R], "launches": launches, "launches_no_chains": launches, "classes": {1: TRSV_CLASSES[T]}, "hubs": {}, "hubs_no_chains": {},
                 "waves": {1: TRSV_WAVES[T][at]}, "frontier_hubs": {}, "resumes": (0, 0)})


def hub_in_tile_counts(stride):
    """stride 2: 800 rows of one entry, 128 a tile; tile 3 holds rows of 4097 and 5000 entries at its positions 5 and 70 (threads 10 and 140) and rows of
    40 and 50 entries at 6 and 7 (threads 12 and 14, one wave). stride 16: 259 rows of 60 and 3 entries in turn, 16 a tile; tile 5 holds the long rows
    at its positions 3 and 9 (threads 48 and 144) and the rows of 40 and 50 at 4 and 5 (threads 64 and 80, one wave, beside the row of 60 at 6)."""
    if stride == 2:
        counts = [1] * 800
        counts[3 * 128 + 5], counts[3 * 128 + 70], counts[3 * 128 + 6], counts[3 * 128 + 7] = 4097, 5000, 40, 50
    else:
        counts = [60 if q % 2 == 0 else 3 for q in range(R)]
        counts[5 * 16 + 3], counts[5 * 16 + 9], counts[5 * 16 + 4], counts[5 * 16 + 5] = 4097, 5000, 40, 50
    return counts


UNROLL = [3, 4, 5, 7, 8, 9, 255, 256, 257, 447, 448, 449, 511, 512, 513, 1023, 1024, 1025, 4351, 4352, 4353, 6143, 6144, 6145]
CHAIN_WIDTHS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256]
CHAIN_STRIDES = (64, 64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1)             # WG / stride is the first power of two that holds the width
MIXED = [[40, 50, 4097, 3, 1],                                                    # 5 rows, stride 32: the wave rows are threads 0 and 32, the hub thread 64
         [3, 40, 50, 4097] + [1] * 13,                                            # 17 rows, stride 8: the wave rows are threads 8 and 16, the hub thread 24
         [2, 40, 50] + [1] * 67 + [4097] + [1] * 58]                              # 129 rows, stride 1: the wave rows are threads 1 and 2, the hub thread 70
ILU_MIXED = [[],
             [(5, 10), (5, 20), (20, 500), (3, 0), (1, 0)],                       # stored 16, 26, 521, 4, 2: as MIXED[0]
             [(3, 0), (5, 10), (5, 20), (20, 500)] + [(2, 0)] * 13,               # as MIXED[1]; the hub pivots on all five rows of the level before it
             [(2, 0), (5, 10), (5, 20)] + [(1, 0)] * 67 + [(140, 400)] + [(1, 0)] * 58]   # as MIXED[2]; the hub pivots on all seventeen, the rest short rows

SOLVE = {f"stride_{T}_{'at' if at else 'below'}": _stride_case(T, at) for T in TRSV_DOUBLING for at in (0, 1)}
SOLVE.update({
    # 800 rows, 10 783 entries: an average of 13, stride 2, 128 rows a tile, seven tiles, the last of 32 rows
    "hub_in_tile_s2": Case("solve", lambda: stack(5008, [hub_in_tile_counts(2)]),
                           {"widths": [5008, 800], "launches": [("level", 1, 20, 144), ("level", 2, 7, 32)],
                            "launches_no_chains": [("level", 1, 20, 144), ("level", 2, 7, 32)], "classes": {1: (796, 2, 2)},
                            "tiles": {(1, 3): ((124, 2, 2), 2, (10, 140)), (1, 2): ((128, 0, 0), 0, ())},
                            "hubs": {(1, 3): (10, 140)}, "hubs_no_chains": {(1, 3): (10, 140)}, "waves": {1: 2}, "frontier_hubs": {}, "resumes": (0, 0)}),
    # 259 rows (126 of 3 entries, 129 of 60, the four of tile 5), about 17 500 entries: an average of 67, stride 16, 16 rows a tile; tile 5 is rows
    # 60 3 60 H 40 50 60 3 60 H 60 3 60 3 60 3: wave 1 takes three wave rows; the last tile, 60 3 60, is one wave's
    "hub_in_tile_s16": Case("solve", lambda: stack(5008, [hub_in_tile_counts(16)]),
                            {"widths": [5008, R], "launches": [("level", 1, 20, 144), ("level", 16, 17, 3)],
                             "launches_no_chains": [("level", 1, 20, 144), ("level", 16, 17, 3)], "classes": {1: (126, 131, 2)},
                             "tiles": {(1, 5): ((5, 9, 2), 3, (48, 144)), (1, 16): ((1, 2, 0), 2, ())},
                             "hubs": {(1, 5): (48, 144)}, "hubs_no_chains": {(1, 5): (48, 144)}, "waves": {1: 3}, "frontier_hubs": {}, "resumes": (0, 0)}),
    # one level of 24 rows: a chain level at stride 8 (32 rows fit, 16 do not), a wave takes eight rows, wave 1 the wave rows 8 … 15; alone in a launch 66 432 entries on 24 rows, stride 64, one row a wave
    "unroll_edges": Case("solve", lambda: stack(6200, [UNROLL]),
                         {"widths": [6200, 24], "launches": [("level", 1, 25, 56), ("chain", (8,))], "launches_no_chains": [("level", 1, 25, 56), ("level", 64, 6, 4)],
                          "classes": {1: (6, 12, 6)}, "hubs": {(1, 0): tuple(8 * q for q in range(18, 24))},
                          "hubs_no_chains": {(1, 4): (128, 192), (1, 5): (0, 64, 128, 192)}, "waves": {1: 8}, "waves_no_chains": {1: 1}, "frontier_hubs": {},
                          "resumes": (0, 0)}),
    "chain_widths": Case("solve", lambda: tr.blocks(CHAIN_WIDTHS),
                         {"widths": CHAIN_WIDTHS, "launches": [("chain", CHAIN_STRIDES)],
                          "launches_no_chains": [("level", 1, 1, w) for w in CHAIN_WIDTHS], "classes": {}, "hubs": {}, "hubs_no_chains": {}, "frontier_hubs": {},
                          "resumes": (0, 0)}),
    # without chains the three levels average 829, 245 and 33 entries a row: strides 64, 32 and 8
    "chain_mixed": Case("solve", lambda: stack(4200, MIXED),
                        {"widths": [4200, 5, 17, 129], "launches": [("level", 1, 17, 104), ("chain", (32, 8, 1))],
                         "launches_no_chains": [("level", 1, 17, 104), ("level", 64, 2, 1), ("level", 32, 3, 1), ("level", 8, 5, 1)],
                         "classes": {1: (2, 2, 1), 2: (14, 2, 1), 3: (126, 2, 1)},
                         "tiles": {(1, 0): ((2, 2, 1), 2, (64,)), (2, 0): ((14, 2, 1), 2, (24,)), (3, 0): ((126, 2, 1), 2, (70,))},
                         "hubs": {(1, 0): (64,), (2, 0): (24,), (3, 0): (70,)}, "hubs_no_chains": {(1, 0): (128,), (2, 0): (96,), (3, 2): (48,)},
                         "waves": {1: 2, 2: 2, 3: 2}, "frontier_hubs": {}, "resumes": (0, 0)}),
    # row 0 is a chain of one level; column 0 of the transposed pattern has k entries: at the cut it is walked in a tile, one above it by walk_hubs
    "col_4096": Case("solve", lambda: dense_column(4096),
                     {"widths": [1, 4096], "launches": [("chain", (64,)), ("level", 1, 16, 256)], "launches_no_chains": [("level", 1, 1, 1), ("level", 1, 16, 256)],
                      "classes": {}, "hubs": {}, "hubs_no_chains": {}, "frontier_entries": [4096, 0], "frontier_hubs": {}, "resumes": (0, 0)}, True),
    "col_4097": Case("solve", lambda: dense_column(4097),
                     {"widths": [1, 4097], "launches": [("chain", (64,)), ("level", 1, 17, 1)], "launches_no_chains": [("level", 1, 1, 1), ("level", 1, 17, 1)],
                      "classes": {}, "hubs": {}, "hubs_no_chains": {}, "frontier_entries": [4097, 0], "frontier_hubs": {0: 1}, "resumes": (0, 0)}, True),
    # frontier 0: 6000 + 5000 + 4097 entries of the hubs and 3000 of the ordinary columns; frontier 1: the 4500 of row 10 and 1500 of ordinary columns
    "hub_cols": Case("solve", hub_columns,
                     {"widths": [10, 6000, 4500], "launches": [("chain", (16,)), ("level", 1, 24, 112), ("level", 1, 18, 148)],
                      "launches_no_chains": [("level", 1, 1, 10), ("level", 1, 24, 112), ("level", 1, 18, 148)], "classes": {}, "hubs": {}, "hubs_no_chains": {},
                      "frontier_entries": [18097, 6000, 0], "frontier_hubs": {0: 3, 1: 1}, "resumes": (0, 0)}, True),
    # the first grid is 8 workgroups: its cap is 8 · 2048 · 8 = 131 072 entries. 64 · 2048 is the cap, 64 · 2049 above it — unless 8 is the largest grid
    "fan_2048": Case("solve", lambda: fan(2048),
                     {"widths": [1, 64, 2048], "launches": [("chain", (64, 4)), ("level", 16, 128, 16)],
                      "launches_no_chains": [("level", 1, 1, 1), ("level", 1, 1, 64), ("level", 16, 128, 16)], "classes": {2: (0, 2048, 0)}, "hubs": {},
                      "hubs_no_chains": {}, "frontier_entries": [64, 131072, 0], "frontier_hubs": {}, "resumes": (0, 0)}, True),
    "fan_2049": Case("solve", lambda: fan(2049),
                     {"widths": [1, 64, 2049], "launches": [("chain", (64, 4)), ("level", 16, 129, 1)],
                      "launches_no_chains": [("level", 1, 1, 1), ("level", 1, 1, 64), ("level", 16, 129, 1)], "classes": {2: (0, 2049, 0)}, "hubs": {},
                      "hubs_no_chains": {}, "frontier_entries": [64, 131136, 0], "frontier_hubs": {}, "resumes": (0, 1)}, True),
})
for _n in (16, 17, 256, 257):                    # bits_of(levels − 1) = 4, 5, 8, 9: one sort pass, two, two, three; one chain of one-row levels
    SOLVE[f"levels_{_n}"] = Case("solve", functools.partial(tr.bidiagonal, _n),
                                 {"widths": [1] * _n, "launches": [("chain", (64,) * _n)], "launches_no_chains": [("level", 1, 1, 1)] * _n, "classes": {}, "hubs": {},
                                  "hubs_no_chains": {}, "frontier_hubs": {}, "sort_passes": {16: 1, 17: 2, 256: 2, 257: 3}[_n], "resumes": (0, 0)}, True)

# ---- ILU(0). T -> (stride one pivot below T·R, stride at T·R): both sides of every doubling of ilu_stride. No level above 0 averages less than one pivot
# a row — a row without a pivot is of level 0 —, so stride 1 is level 0's alone: ilu_stride_1_below puts its mixed rows there, with no pivot at all.
ILU_DOUBLING = {1: (1, 2), 2: (2, 4), 4: (4, 8), 8: (8, 16), 16: (16, 32), 32: (32, 64)}
ILU_TARGETS = [12, 22, 8, 9, 512, 513]           # the stored lengths of the first six rows, where the pivots leave room: two wave rows, both sides of both cuts
SHORT, TAIL = 64, 520
# T -> (lane, wave, hub) rows of the level (below, at): a padding row stores its pivots and its diagonal. Up to 7 pivots it is a lane row; the first six
# rows are wave, wave, lane, wave, wave, hub while T + 1 <= 8, then wave rows but the last (T = 8: 8 pivots are 9 entries)
ILU_CLASSES = {1: (None, (254, 4, 1)), 2: ((254, 4, 1), (254, 4, 1)), 4: ((254, 4, 1), (254, 4, 1)), 8: ((1, 257, 1), (0, 258, 1)), 16: ((0, 258, 1), (0, 258, 1)),
               32: ((0, 258, 1), (0, 258, 1))}


def ilu_stride_spec(T, at):
    """(pivots, upper entries) per row of the level: every row T pivots, `below` the last row one fewer; the first six rows are padded with upper entries to
    ILU_TARGETS stored entries where T pivots and the diagonal leave room"""
    nlow = [T] * R
    if not at:
        nlow[-1] -= 1
    return [(p, max(0, ILU_TARGETS[q] - 1 - p) if q < len(ILU_TARGETS) else 0) for q, p in enumerate(nlow)]


def _ilu_stride_case(T, at):
    s = ILU_DOUBLING[T][at]
    if T == 1 and not at:                        # level 0 alone: 64 short rows, the 259 mixed rows behind them, the tail; the hub is position 69 of tile 0
        launches = [("level", 1, 4, SHORT + R + TAIL - 3 * WG)]
        return Case("ilu", lambda: ilu_stack([[t - 1 for t in ILU_TARGETS] + [1] * (R - len(ILU_TARGETS))], SHORT, TAIL),
                    {"widths": [SHORT + R + TAIL], "launches": launches, "launches_no_chains": launches, "classes": {0: (838, 4, 1)},
                     "tiles": {(0, 0): ((251, 4, 1), 4, (69,))}, "hubs": {(0, 0): (69,)}, "hubs_no_chains": {(0, 0): (69,)}, "waves": {0: 4}, "frontier_hubs": {},
                     "resumes": (0, 0)})
    launches = [("level", 1, 3, SHORT + TAIL - 2 * WG), ("level", s, GRID_OF[s], 3)]
    hub = {(1, 5 // (WG // s)): (5 % (WG // s) * s,)}                        # row 5 of the level is the row of 513 entries
    return Case("ilu", lambda: ilu_stack([[], ilu_stride_spec(T, at)], SHORT, TAIL),
                {"widths": [SHORT + TAIL, R], "launches": launches, "launches_no_chains": launches, "classes": {1: ILU_CLASSES[T][at]}, "hubs": hub,
                 "hubs_no_chains": hub, "frontier_hubs": {}, "resumes": (0, 0)})


def ilu_hub_in_tile_spec(stride):
    """hub_in_tile_counts for the factorisation. stride 2: 259 rows of one pivot, 128 a tile; tile 1 holds rows of 521 and 536 stored entries at its
    positions 5 and 70 (threads 10 and 140) and rows of 16 and 26 at 6 and 7 (threads 12 and 14, one wave). stride 16: rows of 14 pivots (15 stored: a
    wave row) and 6 pivots (7 stored: a lane row) in turn, 16 a tile; tile 5 holds the long rows at 3 and 9 (threads 48 and 144), rows of 20 and 25
    stored entries at 4 and 5 (threads 64 and 80)."""
    if stride == 2:
        spec = [(1, 0)] * R
        spec[128 + 5], spec[128 + 70], spec[128 + 6], spec[128 + 7] = (20, 500), (20, 515), (5, 10), (5, 20)
    else:
        spec = [(14, 0) if q % 2 == 0 else (6, 0) for q in range(R)]
        spec[80 + 3], spec[80 + 9], spec[80 + 4], spec[80 + 5] = (20, 500), (20, 515), (14, 5), (14, 10)
    return spec


ILU = {f"ilu_stride_{T}_{'at' if at else 'below'}": _ilu_stride_case(T, at) for T in ILU_DOUBLING for at in (0, 1)}
ILU.update({
    # 305 pivots on 259 rows: an average of 1, stride 2
    "ilu_hub_in_tile_s2": Case("ilu", lambda: ilu_stack([[], ilu_hub_in_tile_spec(2)], SHORT, TAIL),
                               {"widths": [SHORT + TAIL, R], "launches": [("level", 1, 3, 72), ("level", 2, 3, 3)],
                                "launches_no_chains": [("level", 1, 3, 72), ("level", 2, 3, 3)], "classes": {1: (255, 2, 2)},
                                "tiles": {(1, 1): ((124, 2, 2), 2, (10, 140))}, "hubs": {(1, 1): (10, 140)}, "hubs_no_chains": {(1, 1): (10, 140)},
                                "waves": {1: 2}, "frontier_hubs": {}, "resumes": (0, 0)}),
    # about 2 600 pivots on 259 rows (126 lane rows, 131 wave rows, the two hubs): an average of 10, stride 16; tile 5 is rows W L W H W W W L W H W L W L W L
    "ilu_hub_in_tile_s16": Case("ilu", lambda: ilu_stack([[], ilu_hub_in_tile_spec(16)], SHORT, TAIL),
                                {"widths": [SHORT + TAIL, R], "launches": [("level", 1, 3, 72), ("level", 16, 17, 3)],
                                 "launches_no_chains": [("level", 1, 3, 72), ("level", 16, 17, 3)], "classes": {1: (126, 131, 2)},
                                 "tiles": {(1, 5): ((5, 9, 2), 3, (48, 144))}, "hubs": {(1, 5): (48, 144)}, "hubs_no_chains": {(1, 5): (48, 144)},
                                 "waves": {1: 3}, "frontier_hubs": {}, "resumes": (0, 0)}),
    "ilu_chain_widths": Case("ilu", lambda: il.blocks(CHAIN_WIDTHS),
                             {"widths": CHAIN_WIDTHS, "launches": [("chain", CHAIN_STRIDES)], "hubs": {}, "hubs_no_chains": {}, "frontier_hubs": {},
                              "resumes": (0, 0)}),
    # without chains the three levels average 6, 3 and 2 pivots a row: strides 8, 4 and 4
    "ilu_chain_mixed": Case("ilu", lambda: ilu_stack(ILU_MIXED, 128, TAIL),
                            {"widths": [128 + TAIL, 5, 17, 129], "launches": [("level", 1, 3, 136), ("chain", (32, 8, 1))],
                             "launches_no_chains": [("level", 1, 3, 136), ("level", 8, 1, 5), ("level", 4, 1, 17), ("level", 4, 3, 1)],
                             "classes": {1: (2, 2, 1), 2: (14, 2, 1), 3: (126, 2, 1)},
                             "tiles": {(1, 0): ((2, 2, 1), 2, (64,)), (2, 0): ((14, 2, 1), 2, (24,)), (3, 0): ((126, 2, 1), 2, (70,))},
                             "hubs": {(1, 0): (64,), (2, 0): (24,), (3, 0): (70,)}, "hubs_no_chains": {(1, 0): (16,), (2, 0): (12,), (3, 1): (24,)},
                             "waves": {1: 2, 2: 2, 3: 2}, "frontier_hubs": {}, "resumes": (0, 0)}),
    # level 1 is rows 1 … 4098 with one pivot each, row 0: stride 2, 128 rows a tile. Column 0 is a hub of the lower plan's peel, column 4098 of the upper's
    "arrow_both": Case("ilu", arrow_both,
                       {"widths": [1, 4098], "launches": [("chain", (64,)), ("level", 2, 33, 2)], "launches_no_chains": [("level", 1, 1, 1), ("level", 2, 33, 2)],
                        "classes": {}, "hubs": {}, "hubs_no_chains": {}, "frontier_entries": [4098, 0], "frontier_hubs": {0: 1}, "upper_frontier_hubs": {0: 1},
                        "resumes": (0, 0)}),
})

CASES = {**SOLVE, **ILU}
REQUIRED = ("widths", "launches", "hubs", "hubs_no_chains", "frontier_hubs", "resumes")   # what every case declares; the rest where it is what the case is for


@functools.lru_cache(maxsize=None)
def matrix(name, lower=True):
    """the arrays of a case, read-only; lower = False: the upper twin of a solve case (trsv_ref.mirror)"""
    mat = CASES[name].build()
    if not lower:
        assert CASES[name].kind == "solve"
        mat = tr.mirror(mat)
    for a in mat[1:]:
        a.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def solved(name, lower=True):
    """(matrix, b, x) of a solve case: solved once by trsv_ref, shared and read-only"""
    mat = matrix(name, lower)
    b = tr._rng(300 + len(name)).uniform(-1.0, 1.0, mat[0])
    x = tr.solve(*mat, b, lower)
    b.setflags(write=False)
    x.setflags(write=False)
    return mat, b, x


@functools.lru_cache(maxsize=None)
def factored(name):
    """(matrix, factors, bad_pivot, r, z) of an ILU case: factorised and applied once by ilu_ref, shared and read-only"""
    mat = matrix(name)
    f, bad = il.factor(*mat)
    r = tr._rng(400 + len(name)).uniform(-1.0, 1.0, mat[0])
    z = il.apply(*mat[:3], f, r)
    for a in (f, r, z):
        a.setflags(write=False)
    return mat, f, bad, r, z
