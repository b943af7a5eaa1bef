"""Inputs for the device-resident graph iterations — g4s_pagerank (g4s_amd/csrc/pagerank.hip) and g4s_bfs / g4s_sssp (g4s_amd/csrc/traverse.hip over
frontier.hpp) — that sit ON the dispatch limits of their kernels: the average degree that picks 4, 16 or 64 lanes per row, the 4 096 entries above which
the strength pass hands a row to a whole workgroup, the capped grids behind which a grid-stride loop makes a second trip, the 512 partials of the
epilogue, the 4 096 out-edges above which a vertex goes to the hub end of the queue, and the push/pull switch. Plus a numpy restatement of every one of
those rules, so that tests/test_iteration_cases_cpu.py can prove that a case stands where its descriptor says, for the CU count of the device at hand
(every builder takes `cus`) — tests/test_pagerank_limits_gpu.py and tests/test_traverse_limits_gpu.py then run the cases.
numpy only: no GPU, no torch."""
import functools
from typing import NamedTuple

import numpy as np

# ---- the limits, each beside the source line it mirrors
LONG_ROW = 4096                                  # pagerank.hip: `constexpr int kLongRow = 4096;     // a row with more entries is summed by a whole workgroup`
MAX_GRID = 512                                   # pagerank.hip: `constexpr int kMaxGrid = 512;      // workgroups of the epilogue at most: …`
ITEMS = 8                                        # pagerank.hip: `constexpr int kItems = 8;          // entries per thread the epilogue's grid is sized for`
WG = 256                                         # wave_reduce.hpp: `constexpr int WG = 256;`
HUB_CUT = 4096                                   # frontier.hpp: `constexpr int kHubCut = 4096;`
LPRS = (4, 16, 64)


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def lpr_of(nnz, n):
    """pagerank.hip and traverse.hip alike: `avg = n ? A->nnz / n : 0` (integer division), then `avg <= 4 ? 4 : avg <= 16 ? 16 : 64`."""
    avg = int(nnz) // int(n) if n else 0
    return 4 if avg <= 4 else 16 if avg <= 16 else 64


def grid_rows(n, cus):
    """frontier.hpp: `g = (n + WG - 1) / WG, cap = 8LL * cus; return g < 1 ? 1 : g < cap ? g : cap;`"""
    return max(1, min(_ceil_div(n, WG), 8 * cus))


def strength_grid(n, lpr, cus):
    """pagerank.hip: `max(1LL, min(((long long)n * lpr + WG - 1) / WG, 8LL * cus))` — strength_kernel<lpr>, WG / lpr rows per workgroup and trip"""
    return max(1, min(_ceil_div(n * lpr, WG), 8 * cus))


def strength_long_grid(n, cus):
    """pagerank.hip: `max(1LL, min(((long long)n + WG - 1) / WG, 4LL * cus))` — strength_long_kernel, a window of 256 rows per workgroup and trip"""
    return max(1, min(_ceil_div(n, WG), 4 * cus))


def epilogue_grid(n):
    """pagerank.hip: `max(1LL, min(((long long)n + WG * kItems - 1) / (WG * kItems), (long long)kMaxGrid))` — G: the epilogue, init, vec_sum and the verdicts"""
    return max(1, min(_ceil_div(n, WG * ITEMS), MAX_GRID))


def pull_grid(rows, lpr, cus):
    """traverse.hip: `grid_rows((long long)rows * (avg <= 4 ? 4 : avg <= 16 ? 16 : 64), cus)` — bfs_pull_kernel<lpr>, WG / lpr rows per workgroup and trip"""
    return grid_rows(rows * lpr, cus)


def switch_threshold(nnz, alpha):
    """traverse.hip: `a.threshold = … (long long)((double)A->nnz / switch_alpha(BFS))`; finish(): `e > a.threshold ? 3` — the next step pulls"""
    return int(float(nnz) / float(alpha))


def trips(n, per_workgroup, grid):
    """The trips of workgroup 0 (the most any makes) through `for (r0 = blockIdx.x * P; r0 < n; r0 += gridDim.x * P)`."""
    return _ceil_div(n, per_workgroup * grid)


def sum_depth(n):
    """The additions a term of the dangling-mass or the residual sum passes through, read off epilogue_kernel, block_sum and ordered_sums: at most
    ⌈n / (G·256)⌉ terms per thread, 6 shuffle levels, 4 waves, and G partials in index order."""
    G = epilogue_grid(n)
    return _ceil_div(n, G * WG) + 6 + 4 + G


# ------------------------------------------------------------------------------------------------ PageRank cases
class PrCase(NamedTuple):
    name: str
    arrays: tuple            # (rowptr int32, colids int32, values float64), stored by out-edges, read-only
    rows: dict               # tag -> (vertex, out-degree): the rows the case was built around
    declared: dict           # what the case claims, written by hand at the builder: the CPU test holds it against pr_facts()
    iters: int               # iterations of the GPU test


def _fit(deg, free, target, lo, hi):
    """pad or trim the rows `free` one entry at a time until Σ deg == target, every one staying inside [lo, hi]"""
    free = np.asarray(free)
    diff = target - int(deg.sum())
    while diff != 0:
        ok = free[deg[free] < hi] if diff > 0 else free[deg[free] > lo]
        assert ok.size, "the target is out of reach"
        deg[ok[:abs(diff)]] += 1 if diff > 0 else -1
        diff = target - int(deg.sum())
    return deg


def _csr_of_degrees(deg, rng):
    """Row u: deg[u] distinct targets first[u], first[u] + 1, … (mod n) with first[u] random; weights U[0.5, 2)."""
    deg = np.asarray(deg, np.int64)
    n = deg.size
    assert deg.max() <= n
    rp = np.concatenate([[0], np.cumsum(deg)])
    row = np.repeat(np.arange(n), deg)
    ci = (rng.integers(0, n, n)[row] + (np.arange(rp[-1]) - rp[row])) % n
    return rp.astype(np.int32), ci.astype(np.int32), rng.uniform(0.5, 2.0, int(rp[-1]))


def _finish_pr(name, deg, rows, fixed, target, rng, lo, hi, declared, iters, zero_rows=()):
    """Rows `rows` (tag -> (vertex, degree)) and the vertices of `fixed` (left dangling) keep their degree; the others are padded or trimmed to `target` entries."""
    n = deg.size
    keep = np.zeros(n, bool)
    deg[fixed] = 0
    keep[fixed] = True
    for v, d in rows.values():
        deg[v] = d
        keep[v] = True
    _fit(deg, np.flatnonzero(~keep), target, lo, hi)
    rp, ci, va = _csr_of_degrees(deg, rng)
    for v in zero_rows:
        va[rp[v]:rp[v + 1]] = 0.0
    for a in (rp, ci, va):
        a.setflags(write=False)
    return PrCase(name, (rp, ci, va), dict(rows), dict(declared), iters)


def _dangling_ids(n, every=13, at=5):
    return np.arange(at, n - 8, every)


def _avg_edges(avg, cus):
    """nnz // n exactly `avg`, on the side of the cut that matters: 5n − 1 and 17n − 1 entries are the LAST counts with 4 and 16 lanes per row, 5n and 17n
    the first with 16 and 64. n = 1003 is no multiple of 64, 16 or 4, so the last group of lanes straddles n; its rows are the special ones."""
    n = 1003
    lpr = {4: 4, 5: 16, 16: 16, 17: 64}[avg]
    target = avg * n + (n - 1 if avg in (4, 16) else 0)
    rng = np.random.default_rng(1000 + avg)
    deg = rng.integers(1, 2 * avg + 1, n)
    rows = {"deg_0": (n - 6, 0), "deg_1": (n - 5, 1), "deg_lpr_minus_1": (n - 4, lpr - 1), "deg_lpr": (n - 3, lpr), "deg_lpr_plus_1": (n - 2, lpr + 1),
            "last_deg_3lpr_plus_1": (n - 1, 3 * lpr + 1)}
    declared = {"avg": avg, "lpr": lpr, "strength_trips": 1, "strength_capped": False, "tail_groups_beyond_n": True, "long_rows": 0, "G": 1}
    return _finish_pr(f"avg_edges_{avg}", deg, rows, _dangling_ids(n), target, rng, 1, 6 * avg, declared, 4)


_LONG_NNZ = {4: lambda n: 5 * n - 1, 16: lambda n: 17 * n - 1, 64: lambda n: 17 * n}   # the average stays at the named lpr — on its band's edge


def _long_row_cut(lpr, cus):
    """Rows of 4095 and 4096 entries (strength_kernel's) beside rows of 4097 and 2·4096 + 3 (strength_long_kernel's). Window 3 (ids 768 … 1023) holds
    4097 and 8195 in its first wave (ids 768 … 831), next to the rows of 4095 and 4096, and a row of 4097 stored zeros — long, yet dangling — in its
    third wave; the last vertex is long too. n = 8209 >= 8195 keeps the targets of a row distinct and is no multiple of 64, 16 or 4."""
    n, w = 8209, 3 * WG
    rng = np.random.default_rng(2000 + lpr)
    deg = rng.integers(1, 3 * lpr, n)
    rows = {"deg_4097": (w + 5, LONG_ROW + 1), "deg_4095": (w + 6, LONG_ROW - 1), "deg_4096": (w + 7, LONG_ROW), "deg_8195": (w + 40, 2 * LONG_ROW + 3),
            "zeros_4097": (w + 2 * 64 + 7, LONG_ROW + 1), "last_4097": (n - 1, LONG_ROW + 1)}
    declared = {"lpr": lpr, "long_rows": 4, "long_rows_in_one_wave": 2, "waves_with_long_rows_in_one_window": 2, "last_vertex_long": True,
                "long_dangling": 1, "long_trips": 1}
    return _finish_pr(f"long_row_cut_{lpr}", deg, rows, _dangling_ids(n), _LONG_NNZ[lpr](n), rng, 1, 48, declared, 4, zero_rows=(rows["zeros_4097"][0],))


def _grid_wrap(lpr, cus):
    """n just past the 8·cus·(256 / lpr) rows that strength_kernel<lpr>'s capped grid covers in one trip: two full groups of workgroups more and a ragged
    one, whose last groups of lanes lie beyond n. The last vertex has lpr + 1 entries, the one before it dangles."""
    gpb = WG // lpr
    n = 8 * cus * gpb + 2 * gpb + gpb // 2 + 1
    avg = {4: 3, 16: 10, 64: 20}[lpr]
    rng = np.random.default_rng(3000 + lpr)
    deg = rng.integers(1, 2 * avg, n)
    rows = {"last_deg_lpr_plus_1": (n - 1, lpr + 1), "tail_dangling": (n - 2, 0), "tail_deg_lpr": (n - 3, lpr)}
    declared = {"avg": avg, "lpr": lpr, "strength_trips": 2, "strength_capped": True, "tail_groups_beyond_n": True, "long_rows": 0}
    return _finish_pr(f"grid_wrap_{lpr}", deg, rows, _dangling_ids(n), avg * n + n // 2, rng, 1, 3 * avg, declared, 3)


def _capped_epilogue(cus):
    """n = 2^20 + 3·2048 + 5: G = 512 (the full s_part[2][512]), nine trips per workgroup of the epilogue with a ragged last one. About 3 million entries:
    4 lanes per row, whose grid wraps as well. A few thousand dangling vertices all over the id range, the last vertex among them, and three rows above
    4 096 entries behind the 4·cus·256 rows of strength_long_kernel's first trip — two waves of one window, and the window after it."""
    n = (1 << 20) + 3 * 2048 + 5
    base = 4 * cus * WG
    assert base + 2 * WG < n - 8, "the device has too many CUs for this case"
    rng = np.random.default_rng(4000)
    deg = rng.integers(1, 6, n)
    rows = {"long_a": (base + 3, LONG_ROW + 1), "long_b": (base + 70, 5000), "long_c": (base + WG + 5, 2 * LONG_ROW + 3)}
    fixed = np.concatenate([np.arange(17, n - 8, 251), [n - 1]])
    declared = {"lpr": 4, "G": MAX_GRID, "epilogue_capped": True, "epilogue_ragged": True, "strength_capped": True, "long_rows": 3,
                "first_trip_of_a_long_row": 1, "last_vertex_dangles": True}
    return _finish_pr("capped_epilogue", deg, rows, fixed, 3_000_000, rng, 1, 8, declared, 3)


class BadValues(NamedTuple):
    tag: str
    values: np.ndarray       # the values of long_row_cut_16 with one defect
    row: int                 # the row that holds it
    positions: tuple         # the positions inside that row that differ from the clean array
    what: str


BAD_BASE = "long_row_cut_16"
BAD_TAGS = ("negative_in_last_threads_share_of_long_row", "nan_in_last_lane_of_short_row", "inf_in_last_row", "long_row_sum_overflows", "short_row_sum_overflows")


@functools.lru_cache(maxsize=None)
def bad_values(cus):
    """Five value arrays for the pattern of long_row_cut_16, each with exactly one defect that the strength pass must refuse."""
    c = build(BAD_BASE, cus)
    rp, _, va = c.arrays
    lpr = c.declared["lpr"]
    deg = np.diff(rp)
    special = {v for v, _ in c.rows.values()}
    short = [int(u) for u in np.flatnonzero((deg > lpr) & (deg <= LONG_ROW)) if int(u) not in special]
    huge = np.finfo(np.float64).max
    out = []

    def one(tag, row, positions, value, what):
        v = va.copy()
        v[rp[row] + np.asarray(positions)] = value
        v.setflags(write=False)
        out.append(BadValues(tag, v, int(row), tuple(int(p) for p in positions), what))

    u = c.rows["deg_8195"][0]
    one(BAD_TAGS[0], u, [LONG_ROW + WG - 1], -0.5, "entry 4096 + 255 of a long row: thread 255 of strength_long_kernel, in its last trip")
    one(BAD_TAGS[1], short[0], [lpr - 1], np.nan, "lane lpr − 1 of a row's group in strength_kernel")
    one(BAD_TAGS[2], len(rp) - 2, [deg[-1] - 1], np.inf, "the last entry of the last row")
    u = c.rows["deg_4097"][0]
    one(BAD_TAGS[3], u, np.arange(deg[u]), huge / LONG_ROW, "4097 finite entries of DBL_MAX / 4096: only the workgroup's sum overflows")
    one(BAD_TAGS[4], short[1], np.arange(deg[short[1]]), 0.75 * huge, "finite entries of 0.75·DBL_MAX in a short row: only the sum overflows")
    return tuple(out)


def pr_facts(case, cus):
    """What the mirrored rules say about a PageRank case on a device of `cus` CUs."""
    rp, _, va = case.arrays
    n, nnz = len(rp) - 1, int(rp[-1])
    deg = np.diff(rp).astype(np.int64)
    lpr = lpr_of(nnz, n)
    gpb = WG // lpr
    g, gl, G = strength_grid(n, lpr, cus), strength_long_grid(n, cus), epilogue_grid(n)
    long_ids = np.flatnonzero(deg > LONG_ROW)
    s = np.add.reduceat(np.append(va, 0.0), rp[:-1].astype(np.int64)) * (deg > 0)
    per_wave = np.bincount(long_ids // 64) if long_ids.size else np.zeros(1, int)
    waves_per_window = max((len({int(u) // 64 for u in long_ids if u // WG == w}) for w in set(long_ids // WG)), default=0)
    return {"n": n, "nnz": nnz, "avg": nnz // n, "lpr": lpr,
            "strength_grid": g, "strength_capped": _ceil_div(n * lpr, WG) > 8 * cus, "strength_trips": trips(n, gpb, g), "tail_groups_beyond_n": n % gpb != 0,
            "long_rows": int(long_ids.size), "long_trips": trips(n, WG, gl),
            "first_trip_of_a_long_row": int((long_ids // WG // gl).min()) if long_ids.size else -1,
            "long_rows_in_one_wave": int(per_wave.max()), "waves_with_long_rows_in_one_window": waves_per_window,
            "last_vertex_long": bool(deg[-1] > LONG_ROW), "long_dangling": int(np.sum((deg > LONG_ROW) & ~(s > 0))),
            "last_vertex_dangles": not s[-1] > 0, "dangling": int(np.sum(~(s > 0))),
            "G": G, "epilogue_capped": _ceil_div(n, WG * ITEMS) > MAX_GRID, "epilogue_trips": trips(n, WG, G), "epilogue_ragged": n % (G * WG) != 0,
            "max_out_degree": int(deg.max())}


# ------------------------------------------------------------------------------------------------ traversal cases
class Special(NamedTuple):
    vertex: int
    in_degree: int
    position: int            # where, in the vertex's row of Aᵀ, the one in-neighbour of the level before stands (−1: no such claim)
    level: int               # the BFS level it must get (−1: never reached)
    value: str               # the stored value on that in-edge: "", "zero" or "nan"


class TrCase(NamedTuple):
    name: str
    arrays: tuple            # (rowptr int32, colids int32, values float64), stored by out-edges, read-only
    sources: tuple
    special: dict            # tag -> Special
    declared: dict


def _csr_of_edges(n, src, dst, w):
    src, dst, w = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.float64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    out = np.cumsum(rp).astype(np.int32), dst[order].astype(np.int32), w[order]
    for a in out:
        a.setflags(write=False)
    return out


def transpose(arrays):
    """Aᵀ, stable: row v lists the tails of v's in-edges by ascending id (what g4s_csr_transpose builds, tests/traverse_ref.py)."""
    rp, ci, va = arrays
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp).astype(np.int64))
    perm = np.argsort(ci, kind="stable")
    trp = np.zeros(n + 1, np.int64)
    np.add.at(trp, ci.astype(np.int64) + 1, 1)
    return np.cumsum(trp), row[perm], np.asarray(va)[perm]


_PULL_NNZ = {4: lambda r: 5 * r - 1, 16: lambda r: 17 * r - 1, 64: lambda r: 17 * r}


def _pull_lanes(lpr, values, cus):
    """Vertex 0 is the source; its out-neighbours M (one per special vertex) and O (ordinary, with edges among themselves that set the average) are
    level 1. A special vertex of in-degree d has one in-neighbour in M and d − 1 among the fillers F1 (smaller ids than M) and F2 (larger ids): p of F1
    put the one tail that bfs_pull_kernel may hit at position p of the row of Aᵀ. The fillers have no in-edge: they are never reached, and never a hit."""
    gpb = WG // lpr
    nf = 3 * lpr + 2
    plan = []                                                          # (tag, d, p, value on the edge from M, level, extra tail)
    for d in (1, lpr - 1, lpr, lpr + 1, 3 * lpr + 1):
        for p in sorted({0, d - 1, lpr * ((d - 1) // lpr)}):           # first, last, and the first entry of the last trip
            plan.append((f"in{d}_pos{p}", d, p, "", 2))
    plan.append((f"in{lpr + 3}_pos{lpr + 1}", lpr + 3, lpr + 1, "", 2))    # the middle of a partial last trip
    if values:
        plan.append(("zero_hidden_never", lpr + 1, 1, "zero", -1))
        plan.append(("zero_hidden_later", lpr + 3, lpr + 1, "zero", 3))     # its last in-neighbour is a special vertex of level 2
        plan.append(("nan_edge", lpr + 1, lpr - 1, "nan", 2))
    nm, nt = len(plan), len(plan)
    f1, m0 = 1, 1 + nf
    f2, t0 = m0 + nm, m0 + nm + nf
    o0 = t0 + nt
    no = 300
    while (o0 + no) % gpb == 0 or (o0 + no) % 64 == 0:
        no += 1
    rows = o0 + no
    rng = np.random.default_rng(5000 + lpr + int(values))
    src, dst, w = [0] * (nm + no), list(range(m0, m0 + nm)) + list(range(o0, rows)), list(rng.uniform(0.5, 2.0, nm + no))
    special = {}
    for i, (tag, d, p, kind, level) in enumerate(plan):
        t, m = t0 + i, m0 + i
        later = tag == "zero_hidden_later"
        tails = list(range(f1, f1 + p)) + [m] + list(range(f2, f2 + d - 1 - p - later)) + ([t0] if later else [])
        assert len(tails) == d
        src += tails
        dst += [t] * d
        vals = list(rng.uniform(0.5, 2.0, d))
        vals[p] = {"": vals[p], "zero": 0.0, "nan": np.nan}[kind]
        w += vals
        special[tag] = Special(t, d, p, level, kind)
    special["filler_without_in_edge"] = Special(f1, 0, -1, -1, "")
    pad = _PULL_NNZ[lpr](rows) - len(src)
    assert pad > 0
    src += list(rng.integers(o0, rows, pad))
    dst += list(rng.integers(o0, rows, pad))
    vals = rng.uniform(0.5, 2.0, pad)
    if values:
        vals[::37] = 0.0                                               # stored zeros elsewhere: O → O, both ends level 1 whatever they carry
    w += list(vals)
    declared = {"lpr": lpr, "values": bool(values), "tail_groups_beyond_rows": True, "depth": 3 if values else 2, "more_than_one_workgroup": True}
    return TrCase(f"pull_lanes_{lpr}_{'values' if values else 'plain'}", _csr_of_edges(rows, src, dst, w), (0,), special, declared)


def _rows_wrap(cus):
    """rows = 8·cus·256 + 300: every grid_rows(rows) kernel makes a second trip, bfs_pull_kernel<4> five. A tree of depth 3 from vertex 0 (64 children,
    90 grandchildren each, the rest below them), two random out-edges per leaf back into the tree, and 300 vertices at the high ids that nothing reaches
    (a chain among themselves, with edges into the tree). Weights U[0.05, 1)."""
    rows = 8 * cus * WG + 300
    R = rows - 300
    k1, k2 = 64, 64 * 90
    assert R > 2 * (1 + k1 + k2)
    rng = np.random.default_rng(6000)
    l1, l2, l3 = np.arange(1, 1 + k1), np.arange(1 + k1, 1 + k1 + k2), np.arange(1 + k1 + k2, R)
    unre = np.arange(R, rows)
    src = np.concatenate([np.zeros(k1, np.int64), l1[np.arange(k2) % k1], l2[np.arange(l3.size) % k2], np.repeat(l3, 2), unre[:-1], unre])
    dst = np.concatenate([l1, l2, l3, rng.integers(0, R, 2 * l3.size), unre[1:], rng.integers(0, R, unre.size)])
    special = {"first_unreachable": Special(R, 0, -1, -1, ""), "last_vertex_unreachable": Special(rows - 1, 1, -1, -1, ""),
               "last_reachable": Special(R - 1, -1, -1, 3, "")}
    declared = {"lpr": 4, "values": False, "depth": 3, "unreachable": 300, "rows_trips": 2, "rows_capped": True, "pull_capped": True}
    return TrCase("rows_wrap", _csr_of_edges(rows, src, dst, rng.uniform(0.05, 1.0, src.size)), (0,), special, declared)


HUB_FAN, HUB_LEAVES, HUB_ALPHA = 6000, 5000, 2.0


def _pull_then_push_hub(cus):
    """Vertex 0 → a fan of 6000; every fan vertex → H and two other fan vertices; H → 5000 fresh leaves. nnz = 29 000, so under G4S_TRAVERSE_ALPHA = 2 a
    frontier of more than 14 500 out-edges pulls: the source (6000) is pushed, the fan (18 000) asks for a pull, which finds H and appends it — above
    kHubCut out-edges — to the hub end of the queue from bfs_pull_kernel (BFS) or sssp_combine_kernel (SSSP); H (5000) is pushed by walk_hubs, and the
    leaves (0) by a closing push that finds nothing. The weights keep SSSP on the same steps: source → fan below 0.1 and fan → fan above 0.5, so no fan
    vertex improves after the first push and every frontier is the BFS one."""
    F, L = HUB_FAN, HUB_LEAVES
    n = 1 + F + 1 + L
    fan, H, leaves = np.arange(1, F + 1), F + 1, np.arange(F + 2, n)
    rng = np.random.default_rng(7000)
    i = np.arange(F)
    src = np.concatenate([np.zeros(F, np.int64), fan, fan, fan, np.full(L, H)])
    dst = np.concatenate([fan, fan[(i + 1) % F], np.full(F, H), fan[(i + 7) % F], leaves])
    w = np.concatenate([rng.uniform(0.05, 0.1, F), rng.uniform(0.5, 1.0, F), rng.uniform(0.05, 1.0, F), rng.uniform(0.5, 1.0, F), rng.uniform(0.05, 1.0, L)])
    special = {"hub": Special(H, F, -1, 2, ""), "first_leaf": Special(int(leaves[0]), 1, 0, 3, ""), "last_leaf": Special(n - 1, 1, 0, 3, "")}
    declared = {"lpr": 4, "values": False, "depth": 3, "trace": ("push", "pull", "push", "push"), "hub_out_degree": L, "source_out_degree": F}
    return TrCase("pull_then_push_hub", _csr_of_edges(n, src, dst, w), (0,), special, declared)


def bfs_levels(arrays, sources):
    """(level int32 with −1 where unreached, [the frontier of every level]); an entry is an edge when its value is != 0 (NaN is one)."""
    rp, ci, va = arrays
    n = len(rp) - 1
    rp64 = np.asarray(rp, np.int64)
    level = np.full(n, -1, np.int32)
    frontier = np.unique(np.asarray(sources, np.int64))
    level[frontier] = 0
    fronts, depth = [], 0
    while frontier.size:
        fronts.append(frontier)
        depth += 1
        lens = rp64[frontier + 1] - rp64[frontier]
        k = np.repeat(rp64[frontier] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
        heads = np.asarray(ci)[k][np.asarray(va)[k] != 0]
        frontier = np.unique(heads[level[heads] == -1]).astype(np.int64)
        level[frontier] = depth
    return level, fronts


def direction_trace(arrays, sources, alpha):
    """The kind of every step g4s_bfs runs in direction "auto", the closing one that finds nothing included — so that trace.count("push") is
    info["push_steps"], trace.count("pull") info["pull_steps"] and len(trace) info["iterations"]. The rule of finish() (traverse.hip): a frontier whose
    vertices have more than (long long)(nnz / alpha) out-edges together (`e > a.threshold`) is expanded by a pull step, every other one by a push."""
    rp = np.asarray(arrays[0], np.int64)
    threshold = switch_threshold(int(rp[-1]), alpha)
    _, fronts = bfs_levels(arrays, sources)
    return tuple("pull" if int((rp[f + 1] - rp[f]).sum()) > threshold else "push" for f in fronts)


def hand_worked():
    """(arrays, sources) of the 8-vertex graph 0 → 1, 2; 1 → 3, 4; 2 → 4, 5; 3, 4, 5 → 6; 6 → 7 with unit weights — small enough to trace by hand
    (tests/test_iteration_cases_cpu.py does)."""
    edges = [(0, 1), (0, 2), (1, 3), (1, 4), (2, 4), (2, 5), (3, 6), (4, 6), (5, 6), (6, 7)]
    return _csr_of_edges(8, [e[0] for e in edges], [e[1] for e in edges], np.ones(len(edges))), (0,)


def tr_facts(case, cus):
    """What the mirrored rules say about a traversal case on a device of `cus` CUs."""
    rp, ci, va = case.arrays
    rows, nnz = len(rp) - 1, int(rp[-1])
    lpr = lpr_of(nnz, rows)
    gpb = WG // lpr
    g, gr = pull_grid(rows, lpr, cus), grid_rows(rows, cus)
    level, fronts = bfs_levels(case.arrays, case.sources)
    return {"rows": rows, "nnz": nnz, "avg": nnz // rows, "lpr": lpr, "values": bool(np.any(np.asarray(va) == 0.0)),
            "pull_grid": g, "pull_capped": _ceil_div(rows * lpr, WG) > 8 * cus, "pull_trips": trips(rows, gpb, g), "tail_groups_beyond_rows": rows % gpb != 0,
            "more_than_one_workgroup": g > 1, "rows_grid": gr, "rows_capped": _ceil_div(rows, WG) > 8 * cus, "rows_trips": trips(rows, WG, gr),
            "depth": int(level.max()), "unreachable": int(np.sum(level < 0)), "max_out_degree": int(np.diff(rp).max()),
            "hub_out_degree": int(np.diff(rp)[case.special["hub"].vertex]) if "hub" in case.special else 0,
            "source_out_degree": int(np.diff(rp)[case.sources[0]])}


# ------------------------------------------------------------------------------------------------ the registry
_PR = {**{f"avg_edges_{a}": functools.partial(_avg_edges, a) for a in (4, 5, 16, 17)},
       **{f"long_row_cut_{l}": functools.partial(_long_row_cut, l) for l in LPRS},
       **{f"grid_wrap_{l}": functools.partial(_grid_wrap, l) for l in LPRS},
       "capped_epilogue": _capped_epilogue}
_TR = {**{f"pull_lanes_{l}_{'values' if v else 'plain'}": functools.partial(_pull_lanes, l, v) for l in LPRS for v in (False, True)},
       "rows_wrap": _rows_wrap, "pull_then_push_hub": _pull_then_push_hub}
PR_NAMES, TR_NAMES = tuple(_PR), tuple(_TR)
PULL_LANES = tuple(n for n in TR_NAMES if n.startswith("pull_lanes_"))


@functools.lru_cache(maxsize=None)
def build(name, cus):
    """The case for a device of `cus` CUs (cached: its arrays are read-only)."""
    return (_PR[name] if name in _PR else _TR[name])(cus)


# ------------------------------------------------------------------------------------------------ every edge against the cases that carry it
# edge: [(case, {a key of pr_facts / tr_facts: its value} or {"row:<tag>": out-degree} or {"special:<tag>": (in-degree, position, level)}), …] — checked
# by tests/test_iteration_cases_cpu.py for two CU counts
def _c(case, **want):
    return case, want


def _pull_specials(lpr, values):
    out = {}
    for d in (1, lpr - 1, lpr, lpr + 1, 3 * lpr + 1):
        for p in sorted({0, d - 1, lpr * ((d - 1) // lpr)}):
            out[f"special:in{d}_pos{p}"] = (d, p, 2)
    if values:
        out.update({"special:zero_hidden_never": (lpr + 1, 1, -1), "special:zero_hidden_later": (lpr + 3, lpr + 1, 3), "special:nan_edge": (lpr + 1, lpr - 1, 2)})
    return out


COVERAGE = {
    # PageRank: the lanes-per-row rule
    "pr_avg_4_is_lpr_4": [_c("avg_edges_4", avg=4, lpr=4, nnz=5 * 1003 - 1)],
    "pr_avg_5_is_lpr_16": [_c("avg_edges_5", avg=5, lpr=16, nnz=5 * 1003)],
    "pr_avg_16_is_lpr_16": [_c("avg_edges_16", avg=16, lpr=16, nnz=17 * 1003 - 1)],
    "pr_avg_17_is_lpr_64": [_c("avg_edges_17", avg=17, lpr=64, nnz=17 * 1003)],
    **{f"pr_row_lengths_around_lpr_{l}": [_c(f"avg_edges_{a}", tail_groups_beyond_n=True, **{"row:deg_0": 0, "row:deg_1": 1, "row:deg_lpr_minus_1": l - 1, "row:deg_lpr": l,
                                                                                         "row:deg_lpr_plus_1": l + 1, "row:last_deg_3lpr_plus_1": 3 * l + 1})
                                          for a in {4: (4,), 16: (5, 16), 64: (17,)}[l]] for l in LPRS},
    # PageRank: the long-row cut
    **{f"pr_long_row_cut_lpr_{l}": [_c(f"long_row_cut_{l}", lpr=l, long_rows=4, **{"row:deg_4095": 4095, "row:deg_4096": 4096, "row:deg_4097": 4097, "row:deg_8195": 8195})]
       for l in LPRS},
    "pr_long_rows_in_one_wave": [_c(f"long_row_cut_{l}", long_rows_in_one_wave=2) for l in LPRS],
    "pr_long_rows_in_two_waves_of_a_window": [_c(f"long_row_cut_{l}", waves_with_long_rows_in_one_window=2) for l in LPRS] + [_c("capped_epilogue", waves_with_long_rows_in_one_window=2)],
    "pr_long_row_last_vertex": [_c(f"long_row_cut_{l}", last_vertex_long=True, **{"row:last_4097": 4097}) for l in LPRS],
    "pr_long_row_of_zeros_dangles": [_c(f"long_row_cut_{l}", long_dangling=1, **{"row:zeros_4097": 4097}) for l in LPRS],
    # PageRank: capped grids
    **{f"pr_strength_grid_wraps_lpr_{l}": [_c(f"grid_wrap_{l}", lpr=l, strength_capped=True, strength_trips=2, tail_groups_beyond_n=True)] for l in LPRS},
    "pr_strength_long_second_trip": [_c("capped_epilogue", long_rows=3, first_trip_of_a_long_row=1)],
    "pr_epilogue_grid_512": [_c("capped_epilogue", G=512, epilogue_capped=True, epilogue_ragged=True, lpr=4, strength_capped=True, last_vertex_dangles=True)],
    "pr_epilogue_grid_not_capped": [_c("grid_wrap_4", epilogue_capped=False), _c("long_row_cut_16", epilogue_capped=False, G=5)],
    # PageRank: refused values
    "pr_bad_values": [_c(BAD_BASE, lpr=16)],
    # traversal: the six instantiations of bfs_pull_kernel and where the one hit stands
    **{f"tr_pull_{l}_{'values' if v else 'plain'}": [_c(f"pull_lanes_{l}_{'values' if v else 'plain'}", lpr=l, values=v, tail_groups_beyond_rows=True, more_than_one_workgroup=True,
                                                        **_pull_specials(l, v), **{"special:filler_without_in_edge": (0, -1, -1)})]
       for l in LPRS for v in (False, True)},
    "tr_pull_band_edges": [_c("pull_lanes_4_plain", avg=4), _c("pull_lanes_16_plain", avg=16), _c("pull_lanes_64_plain", avg=17)],
    # traversal: capped grids
    "tr_rows_grid_wraps": [_c("rows_wrap", rows_capped=True, rows_trips=2, pull_capped=True, lpr=4, depth=3, unreachable=300)],
    # traversal: a hub found by a pull step
    "tr_hub_found_by_pull": [_c("pull_then_push_hub", hub_out_degree=5000, source_out_degree=6000, depth=3, lpr=4, values=False, **{"special:hub": (6000, -1, 2)})],
}
