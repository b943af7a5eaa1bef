"""The cases of tests/iteration_cases.py stand where they claim — row lengths, averages, lanes per row, grids and trip counts, counted here from the arrays
and the mirrored rules for two CU counts — the "just past" cases are past their cap and the "at" cases are not, COVERAGE names every edge and every case
it names exists, the mirrored constants and rules are the source's (read from pagerank.hip, traverse.hip, frontier.hpp and wave_reduce.hpp), direction_trace
restates the push/pull switch, and the references run on every case. No GPU."""
import math
import os
import re
import time

import numpy as np
import pytest

from tests import iteration_cases as ic
from tests import pagerank_ref, traverse_ref

CUS = (256, 40)                                                        # the MI355X's count and another: the sizes must follow the device
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "g4s_amd", "csrc")
both = pytest.mark.parametrize("cus", CUS)


def source_limits(csrc=CSRC):
    """The numbers and rules of the source that iteration_cases mirrors, by regular expression; a rule that is not found word for word is None."""
    read = lambda f: open(os.path.join(csrc, f)).read()
    pr, tr, fr, wr = read("pagerank.hip"), read("traverse.hip"), read("frontier.hpp"), read("wave_reduce.hpp")
    const = lambda text, name: (lambda m: int(m.group(1)) if m else None)(re.search(r"constexpr int %s = (\d+);" % name, text))
    has = lambda text, literal: literal in text
    rule = "avg <= 4 ? 4 : avg <= 16 ? 16 : 64"
    strength = re.search(r"void strength_kernel\(.*?\n}\n", pr, re.S)
    strength_long = re.search(r"void strength_long_kernel\(.*?\n}\n", pr, re.S)
    return {"kLongRow": const(pr, "kLongRow"), "kMaxGrid": const(pr, "kMaxGrid"), "kItems": const(pr, "kItems"), "kHubCut": const(fr, "kHubCut"), "WG": const(wr, "WG"),
            "lpr_rule_pagerank": has(pr, "const int lpr = " + rule + ";") and has(pr, "const long long avg = n ? A->nnz / n : 0;"),
            "lpr_rule_traverse": has(tr, "grid_rows((long long)rows * (" + rule + "), w->mem.cus)") and has(tr, "const long long avg = rows ? A->nnz / rows : 0;")
                                 and has(tr, "if (avg <= 4) TV_PULL(4);") and has(tr, "else if (avg <= 16) TV_PULL(16);"),
            "short_rows": bool(strength) and has(strength.group(0), "if (e - b <= kLongRow) {"),
            "long_rows": bool(strength_long) and has(strength_long.group(0), "rowptr[u + 1] - rowptr[u] > kLongRow;"),
            "strength_grid": has(pr, "std::min(((long long)n * lpr + WG - 1) / WG, 8LL * w->mem.cus)"),
            "strength_long_grid": has(pr, "std::min(((long long)n + WG - 1) / WG, 4LL * w->mem.cus)"),
            "epilogue_grid": has(pr, "std::min(((long long)n + WG * kItems - 1) / (WG * kItems), (long long)kMaxGrid)"),
            "grid_rows": has(fr, "const long long g = (n + WG - 1) / WG, cap = 8LL * cus;") and has(fr, "return (int)(g < 1 ? 1 : g < cap ? g : cap);"),
            "hub": has(tr, "const bool hub = want && deg > kHubCut;"),
            "switch": has(tr, "(long long)((double)A->nnz / switch_alpha(BFS))") and has(tr, "(e > a.threshold ? 3 :")}


def test_the_mirrored_limits_are_the_sources():
    s = source_limits()
    assert (s["kLongRow"], s["kMaxGrid"], s["kItems"], s["kHubCut"], s["WG"]) == (ic.LONG_ROW, ic.MAX_GRID, ic.ITEMS, ic.HUB_CUT, ic.WG), s
    for key in ("lpr_rule_pagerank", "lpr_rule_traverse", "short_rows", "long_rows", "strength_grid", "strength_long_grid", "epilogue_grid", "grid_rows", "hub", "switch"):
        assert s[key] is True, f"{key}: the source no longer reads as tests/iteration_cases.py restates it"
    # the restated rules at and around every cut
    assert [ic.lpr_of(a * 10 + r, 10) for a, r in ((0, 0), (4, 9), (5, 0), (16, 9), (17, 0), (400, 0))] == [4, 4, 16, 16, 64, 64] and ic.lpr_of(0, 0) == 4
    assert [ic.grid_rows(n, 2) for n in (0, 1, 256, 257, 16 * 256, 16 * 256 + 1)] == [1, 1, 1, 2, 16, 16]
    assert [ic.epilogue_grid(n) for n in (1, 2048, 2049, 512 * 2048, 512 * 2048 + 1)] == [1, 1, 2, 512, 512]
    assert [ic.strength_grid(n, 16, 2) for n in (1, 16, 17, 256, 257)] == [1, 1, 2, 16, 16] and [ic.strength_long_grid(n, 2) for n in (1, 257, 2048, 2049)] == [1, 2, 8, 8]
    assert ic.switch_threshold(29000, 2.0) == 14500 and ic.switch_threshold(10, 4.0) == 2 and ic.switch_threshold(7, 1.0) == 7
    assert [ic.trips(n, 64, 4) for n in (1, 256, 257, 512, 513)] == [1, 1, 2, 2, 3]
    assert ic.sum_depth(1003) == 4 + 6 + 4 + 1 and ic.sum_depth((1 << 20) + 3 * 2048 + 5) == 9 + 6 + 4 + 512


def _well_formed(arrays):
    rp, ci, va = arrays
    n = len(rp) - 1
    assert rp.dtype == ci.dtype == np.int32 and va.dtype == np.float64
    assert rp[0] == 0 and rp[-1] == len(ci) == len(va) and np.all(np.diff(rp) >= 0) and ci.min() >= 0 and ci.max() < n
    return n


@both
@pytest.mark.parametrize("name", ic.PR_NAMES)
def test_pagerank_case_stands_where_it_claims(name, cus):
    c = ic.build(name, cus)
    rp, ci, va = c.arrays
    n = _well_formed(c.arrays)
    f = ic.pr_facts(c, cus)
    deg = np.diff(rp)
    for key, want in c.declared.items():
        assert f[key] == want, (name, cus, key, f[key], want)
    for tag, (v, d) in c.rows.items():
        assert deg[v] == d, (tag, v, deg[v], d)
    zero_rows = [v for tag, (v, _) in c.rows.items() if tag.startswith("zeros")]
    stored = np.ones(len(va), bool)
    for v in zero_rows:
        assert np.all(va[rp[v]:rp[v + 1]] == 0.0)
        stored[rp[v]:rp[v + 1]] = False
    assert np.all((va[stored] >= 0.5) & (va[stored] < 2.0)), "weights U[0.5, 2)"
    assert 3 <= c.iters <= 5
    assert f["dangling"] >= 3 and f["dangling"] < n // 4                # some vertices dangle, most do not
    lpr, gpb = f["lpr"], ic.WG // f["lpr"]
    assert n % gpb != 0, "the last group of lanes straddles n"
    if name.startswith("avg_edges"):
        # on the side of the cut that matters: one entry more (avg 4, 16) or fewer (avg 5, 17) and the other kernel runs
        nnz = f["nnz"]
        other = ic.lpr_of(nnz + 1, n) if f["avg"] in (4, 16) else ic.lpr_of(nnz - 1, n)
        assert other != lpr and {lpr, other} == ({4, 16} if f["avg"] in (4, 5) else {16, 64})
        assert any(v == n - 1 for v, _ in c.rows.values()) and sorted(d for _, d in c.rows.values()) == [0, 1, lpr - 1, lpr, lpr + 1, 3 * lpr + 1]
        assert all(v >= n - n % gpb - gpb for v, _ in c.rows.values() if gpb >= 16), "the special rows sit in the last workgroups' groups"
    if name.startswith("long_row_cut"):
        assert n >= 8200 and lpr == int(name.rsplit("_", 1)[1])
        for v in (v for v, d in c.rows.values() if d >= ic.LONG_ROW - 1):
            cols = ci[rp[v]:rp[v + 1]]
            assert len(np.unique(cols)) == len(cols), "distinct targets"
        w = {tag: v // 64 for tag, (v, _) in c.rows.items()}
        assert w["deg_4097"] == w["deg_8195"] == w["deg_4095"] == w["deg_4096"] and w["zeros_4097"] != w["deg_4097"]
        assert len({v // ic.WG for tag, (v, _) in c.rows.items() if tag != "last_4097"}) == 1 and c.rows["last_4097"][0] == n - 1
        assert deg[c.rows["deg_4096"][0]] <= ic.LONG_ROW < deg[c.rows["deg_4097"][0]]      # at the cut, and just past it
        assert f["nnz"] == {4: 5 * n - 1, 16: 17 * n - 1, 64: 17 * n}[lpr]
    if name.startswith("grid_wrap"):
        cap_rows = 8 * cus * gpb                                         # the rows of one trip of the capped grid
        assert cap_rows + 2 * gpb < n < cap_rows + 3 * gpb, "just past the cap: a second trip of three workgroups, the last one ragged"
        assert ic.strength_grid(n, lpr, cus) == 8 * cus and ic.strength_grid(cap_rows, lpr, cus) == 8 * cus and ic.trips(cap_rows, gpb, 8 * cus) == 1
        assert c.rows["last_deg_lpr_plus_1"][0] == n - 1
        assert np.sum(deg[cap_rows:] == 0) >= 1 and np.sum(deg[cap_rows:] > 0) >= 2 * gpb, "the second trip has rows to sum and a dangling one"
    if name == "capped_epilogue":
        assert n == (1 << 20) + 3 * 2048 + 5 and n > ic.MAX_GRID * ic.WG * ic.ITEMS and f["epilogue_trips"] == 9 > ic.ITEMS
        assert all(f["epilogue_trips"] - 1 <= ic._ceil_div(max(0, n - b * ic.WG), ic.MAX_GRID * ic.WG) <= f["epilogue_trips"] for b in range(ic.MAX_GRID)), "every workgroup wraps"
        assert f["nnz"] == 3_000_000 and f["avg"] <= 4 and f["strength_trips"] == ic._ceil_div(n, 8 * cus * 64) >= 2
        dang = np.flatnonzero(deg == 0)
        assert 2000 <= dang.size <= 9000 and dang[-1] == n - 1 and np.all(np.bincount(dang * 8 // n, minlength=8) > 200), "dangling vertices all over the id range"
        assert all(v >= 4 * cus * ic.WG for v, _ in c.rows.values()) and f["long_trips"] >= 2
    else:
        assert f["epilogue_capped"] is False and f["epilogue_trips"] <= ic.ITEMS   # the "at" side: below the cap a thread has its kItems entries at most


@both
def test_bad_values_have_one_defect_each(cus):
    base = ic.build(ic.BAD_BASE, cus)
    rp, _, va = base.arrays
    lpr, deg = base.declared["lpr"], np.diff(rp)
    bad = {b.tag: b for b in ic.bad_values(cus)}
    assert tuple(bad) == ic.BAD_TAGS
    for b in bad.values():
        diff = np.flatnonzero(~((b.values == va) | (np.isnan(b.values) & np.isnan(va))))
        assert np.array_equal(diff, rp[b.row] + np.asarray(b.positions)), b.tag                    # one defect, in one row
    b = bad["negative_in_last_threads_share_of_long_row"]
    assert deg[b.row] > ic.LONG_ROW + ic.WG and b.positions == (ic.LONG_ROW + ic.WG - 1,) and b.positions[0] % ic.WG == ic.WG - 1 and b.values[rp[b.row] + b.positions[0]] < 0
    b = bad["nan_in_last_lane_of_short_row"]
    assert lpr < deg[b.row] <= ic.LONG_ROW and b.positions == (lpr - 1,) and np.isnan(b.values[rp[b.row] + lpr - 1])
    b = bad["inf_in_last_row"]
    assert b.row == len(rp) - 2 and np.isinf(b.values[-1]) and np.sum(~np.isfinite(b.values)) == 1
    for tag, long in (("long_row_sum_overflows", True), ("short_row_sum_overflows", False)):
        b = bad[tag]
        row = b.values[rp[b.row]:rp[b.row + 1]]
        assert (deg[b.row] > ic.LONG_ROW) == long and deg[b.row] > lpr and np.all(np.isfinite(b.values)) and np.all(b.values >= 0)
        with np.errstate(over="ignore"):
            assert np.isinf(row.sum()) and np.isinf(row[::-1].sum()) and np.isfinite(row.astype(np.longdouble).sum())   # only the float64 sum overflows


@both
@pytest.mark.parametrize("name", ic.TR_NAMES)
def test_traversal_case_stands_where_it_claims(name, cus):
    c = ic.build(name, cus)
    rp, ci, va = c.arrays
    rows = _well_formed(c.arrays)
    f = ic.tr_facts(c, cus)
    for key, want in c.declared.items():
        if key != "trace":
            assert f[key] == want, (name, cus, key, f[key], want)
    level, depth = traverse_ref.bfs(rp, ci, va, rows, list(c.sources))
    assert np.array_equal(level, ic.bfs_levels(c.arrays, c.sources)[0]) and depth == f["depth"]
    trp, tci, tva = ic.transpose(c.arrays)
    for tag, s in c.special.items():
        tails, vals = tci[trp[s.vertex]:trp[s.vertex + 1]], tva[trp[s.vertex]:trp[s.vertex + 1]]
        assert s.in_degree < 0 or len(tails) == s.in_degree, (tag, len(tails))
        assert level[s.vertex] == s.level, (tag, level[s.vertex])
        if s.position >= 0:
            prev = 1 if s.value else s.level - 1
            assert list(np.flatnonzero(level[tails] == prev)) == [s.position], (tag, "exactly one in-neighbour in the level before, where the descriptor says")
            v = vals[s.position]
            assert {"": np.isfinite(v) and v != 0, "zero": v == 0, "nan": np.isnan(v)}[s.value], (tag, v)
            if s.value == "zero":
                assert np.all(level[np.delete(tails, s.position)] != 1), "nothing else finds it in that step"
    lpr, gpb = f["lpr"], ic.WG // f["lpr"]
    if name.startswith("pull_lanes"):
        want_lpr, want_values = int(name.split("_")[2]), name.endswith("values")
        assert (lpr, f["values"]) == (want_lpr, want_values) and rows % gpb != 0
        assert f["nnz"] == {4: 5 * rows - 1, 16: 17 * rows - 1, 64: 17 * rows}[lpr]               # the band's edge
        sp = [s for s in c.special.values() if s.position >= 0 and not s.value]
        assert sorted({s.in_degree for s in sp}) == sorted({1, lpr - 1, lpr, lpr + 1, lpr + 3, 3 * lpr + 1})
        assert any(s.position == 0 and s.in_degree > lpr for s in sp), "a hit in the first trip of several"
        assert any(s.position == s.in_degree - 1 and s.in_degree % lpr == 0 for s in sp), "a hit in the last lane of a full trip"
        assert any(s.position >= lpr * ((s.in_degree - 1) // lpr) and s.in_degree % lpr != 0 and s.in_degree > lpr for s in sp), "a hit in a partial last trip"
        assert any(0 < s.position % lpr and s.position < s.in_degree - 1 for s in sp), "a hit that is neither the first nor the last lane"
        assert f["max_out_degree"] <= ic.HUB_CUT and (np.any(np.isnan(va)) == want_values)
        if want_values:
            assert {s.value for s in c.special.values()} == {"", "zero", "nan"} and all(s.position % lpr != 0 for s in c.special.values() if s.value)
    if name == "rows_wrap":
        assert rows == 8 * cus * ic.WG + 300 and ic.grid_rows(rows, cus) == 8 * cus == ic.grid_rows(rows - 300, cus) and ic.trips(rows - 300, ic.WG, 8 * cus) == 1
        assert f["avg"] <= 4 and f["pull_trips"] == 5 and np.all(level[rows - 300:] == -1) and np.all(level[:rows - 300] >= 0) and f["max_out_degree"] <= ic.HUB_CUT
        assert np.all((va >= 0.05) & (va < 1.0))
    if name == "pull_then_push_hub":
        assert c.declared["trace"] == ic.direction_trace(c.arrays, c.sources, ic.HUB_ALPHA) == ("push", "pull", "push", "push")
        H = c.special["hub"].vertex
        leaves = ci[rp[H]:rp[H + 1]]
        assert len(leaves) == 5000 > ic.HUB_CUT and np.all(level[leaves] == level[H] + 1) and np.all(np.diff(rp)[leaves] == 0)
        assert f["nnz"] == 29000 and ic.switch_threshold(29000, ic.HUB_ALPHA) == 14500 and 6000 <= 14500 < 18000 and 5000 <= 14500
        # the weights keep SSSP on the BFS frontiers: after the first push no fan vertex improves
        d, _, converged, _ = traverse_ref.sssp(rp, ci, va, rows, [0])
        fan = ci[rp[0]:rp[1]]
        assert converged and np.array_equal(d[fan], va[rp[0]:rp[1]])


def test_direction_trace_on_a_hand_worked_graph():
    """0 → 1, 2; 1 → 3, 4; 2 → 4, 5; 3, 4, 5 → 6; 6 → 7: ten entries. alpha = 4: threshold (long long)(10 / 4) = 2. Frontiers and their out-edges:
    {0}: 2, not above 2 — push; {1, 2}: 4 — pull; {3, 4, 5}: 3 — pull; {6}: 1 — push; {7}: 0 — the closing push that finds nothing."""
    arrays, sources = ic.hand_worked()
    assert int(arrays[0][-1]) == 10
    assert ic.direction_trace(arrays, sources, 4.0) == ("push", "pull", "pull", "push", "push")
    assert ic.direction_trace(arrays, sources, 1.0) == ("push",) * 5     # g4s_bfs's default: never above nnz
    assert ic.direction_trace(arrays, sources, 100.0) == ("pull",) * 4 + ("push",)    # threshold 0: every frontier with an out-edge pulls
    level, depth = traverse_ref.bfs(*arrays, 8, list(sources))
    assert list(level) == [0, 1, 1, 2, 2, 2, 3, 4] and len(ic.direction_trace(arrays, sources, 4.0)) == depth + 1   # info["iterations"]


@both
def test_coverage_names_every_edge_and_every_case(cus):
    wanted = {"pr_avg_4_is_lpr_4", "pr_avg_5_is_lpr_16", "pr_avg_16_is_lpr_16", "pr_avg_17_is_lpr_64", "pr_long_rows_in_one_wave", "pr_long_rows_in_two_waves_of_a_window",
              "pr_long_row_last_vertex", "pr_long_row_of_zeros_dangles", "pr_strength_long_second_trip", "pr_epilogue_grid_512", "pr_epilogue_grid_not_capped", "pr_bad_values",
              "tr_pull_band_edges", "tr_rows_grid_wraps", "tr_hub_found_by_pull"}
    wanted |= {f"pr_row_lengths_around_lpr_{l}" for l in ic.LPRS} | {f"pr_long_row_cut_lpr_{l}" for l in ic.LPRS} | {f"pr_strength_grid_wraps_lpr_{l}" for l in ic.LPRS}
    wanted |= {f"tr_pull_{l}_{v}" for l in ic.LPRS for v in ("plain", "values")}
    assert set(ic.COVERAGE) == wanted
    used = set()
    for edge, carriers in ic.COVERAGE.items():
        assert carriers, edge
        for name, want in carriers:
            assert name in ic.PR_NAMES + ic.TR_NAMES, (edge, name)
            c = ic.build(name, cus)                                     # a case taken out of the module fails here
            used.add(name)
            pr = name in ic.PR_NAMES
            f = ic.pr_facts(c, cus) if pr else ic.tr_facts(c, cus)
            for key, value in want.items():
                if key.startswith("row:"):
                    v, d = c.rows[key[4:]]
                    assert d == value == np.diff(c.arrays[0])[v], (edge, name, key)
                elif key.startswith("special:"):
                    s = c.special[key[8:]]
                    assert (s.in_degree, s.position, s.level) == value, (edge, name, key, s)
                else:
                    assert f[key] == value, (edge, name, key, f[key], value)
    assert used == set(ic.PR_NAMES + ic.TR_NAMES), "every case carries an edge"


def test_gamma_takes_the_depth_of_the_sums():
    for n, i, o in ((1, 0, 0), (1003, 40, 193), (1 << 14, 3000, 2000)):
        old = (i + o + math.ceil(math.log2(max(n, 1))) + 16) * 2.0 ** -53
        assert pagerank_ref.gamma(n, i, o) == old == pagerank_ref.gamma(n, i, o, math.ceil(math.log2(max(n, 1))) + 8)   # the default is what it was
    n = (1 << 20) + 3 * 2048 + 5
    assert pagerank_ref.gamma(n, 10, 20, ic.sum_depth(n)) == (10 + 20 + 8 + 531) * 2.0 ** -53 > pagerank_ref.gamma(n, 10, 20)


def test_the_references_run_on_every_case():
    cus, spent = CUS[0], {}
    for name in ic.PR_NAMES:
        c = ic.build(name, cus)
        rp, ci, va = c.arrays
        t0 = time.perf_counter()
        ref = pagerank_ref.pagerank(rp, ci, va, len(rp) - 1, tol=0.0, max_iterations=c.iters)
        spent[name] = time.perf_counter() - t0
        assert len(ref.residuals) == c.iters and ref.dangling == ic.pr_facts(c, cus)["dangling"] and abs(float(ref.rank.sum()) - 1.0) < 1e-12
    for name in ic.TR_NAMES:
        c = ic.build(name, cus)
        rp, ci, va = c.arrays
        t0 = time.perf_counter()
        level, _ = traverse_ref.bfs(rp, ci, va, len(rp) - 1, list(c.sources))
        if not np.any(np.isnan(va)):
            d, _, converged, _ = traverse_ref.sssp(rp, ci, va, len(rp) - 1, list(c.sources))
            assert converged and (name.endswith("values") or np.array_equal(np.isfinite(d), level >= 0))
        spent[name] = time.perf_counter() - t0
    print("reference seconds:", {k: round(v, 2) for k, v in spent.items()})
    assert max(spent.values()) < 30.0, spent                            # a few seconds each here; the bound only catches a reference that stopped scaling
