"""What pins tests/level_cases.py without a device: every case stands where its hand-written `declared` says — the strides of its launches, their grids
and cut last tiles, the row classes of its tiles, the threads that own its hubs, the hub columns of its frontiers and the resumes of its peel — for CU
counts on both sides of the smallest step grid; the pairs differ in the one thing they are a pair for; the restated rules agree with the table of
tests/cpp/level_schedule_test.cpp and with g4s.h; and trsv_ref and ilu_ref hold on the new shapes (Higham's componentwise bound, which needs no measured
tolerance, and scipy on the pattern)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import ilu_ref as il
from tests import level_cases as lc
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_view(facts, declared):
    """the facts under the keys a case declares, in the shape it declares them"""
    out = {}
    for k, want in declared.items():
        if k == "tiles":
            out[k] = {t: facts["tiles"][t] for t in want}
        elif k == "upper_frontier_hubs":
            out[k] = facts["upper"]["frontier_hubs"]
        else:
            out[k] = facts[k]
    return out


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_stands_where_it_is_declared(name):
    c = lc.CASES[name]
    assert all(k in c.declared for k in lc.REQUIRED), name
    for cus in lc.CUS:
        f = lc.facts(name, cus)
        want = dict(c.declared)
        want["resumes"] = c.declared["resumes"][2 * cus > lc.MIN_GRID]      # (where the first grid is already the largest, everywhere else)
        assert _declared_view(f, want) == want, (name, cus)
        assert f["levels"] == len(f["widths"]) and f["host_waits"] == 3 + len(f["batches"]) + 1
        assert f["launches_analysis"] == 4 + 5 + sum(f["batches"]) + 4 + 3 * f["sort_passes"] + 6
        assert f["resumes"] <= len(f["batches"]) - 1 and f["batches"][0] == lc.BATCH
    if c.kind == "solve":                                                   # the upper twin: the same DAG, the rows of a level in the opposite order
        lo, up = lc.facts(name, 304), lc.facts(name, 304, lower=False)
        for k in ("levels", "widths", "launches", "launches_no_chains", "classes", "frontier_entries", "frontier_hubs", "resumes", "launches_analysis", "host_waits"):
            assert lo[k] == up[k], (name, k)
        assert {k: len(v) for k, v in lo["hubs"].items() if k[0] > 0 and lo["widths"][k[0]] <= lc.WG} == \
               {k: len(v) for k, v in up["hubs"].items() if k[0] > 0 and up["widths"][k[0]] <= lc.WG}


def test_every_gap_has_its_case():
    """the cases together reach what the suite did not: every stride of both rules in a level launch of several workgroups, every chain stride, hubs owned
    by other threads than 0 in other workgroups than 0 beside lane and wave rows, two wave rows in one wave beside a hub, hub columns from the seed and
    from a step, a resume, and both sides of both sort-pass boundaries"""
    solve = {s for n in lc.SOLVE for k in ("launches", "launches_no_chains") for l in lc.facts(n, 304)[k] if l[0] == "level" and l[2] >= 2 for s in [l[1]]}
    ilu = {s for n in lc.ILU for k in ("launches", "launches_no_chains") for l in lc.facts(n, 304)[k] if l[0] == "level" and l[2] >= 2 for s in [l[1]]}
    assert solve == {1, 2, 4, 8, 16, 32, 64} and ilu == {1, 2, 4, 8, 16, 32, 64}
    for names in (lc.SOLVE, lc.ILU):
        chain = {s for n in names for l in lc.facts(n, 304)["launches"] if l[0] == "chain" for s in l[1]}
        assert chain == {1, 2, 4, 8, 16, 32, 64}
    for name in ("hub_in_tile_s2", "hub_in_tile_s16", "ilu_hub_in_tile_s2", "ilu_hub_in_tile_s16"):
        f = lc.facts(name, 304)
        (key, owners), = f["hubs"].items()
        (lane, wave, hub), in_one_wave, _ = f["tiles"][key]
        assert key[1] > 0 and len(owners) == 2 and 0 not in owners and lane > 0 and wave >= 2 and hub == 2 and in_one_wave >= 2
        assert f["launches"][key[0]][1] == (2 if name.endswith("s2") else 16) and owners[0] // 64 != owners[1] // 64
    for name in ("hub_in_tile_s2", "hub_in_tile_s16"):                      # the upper twins turn every level round: still no hub in workgroup 0 or on thread 0
        up = lc.facts(name, 304, lower=False)["hubs"]
        assert sum(len(v) for v in up.values()) == 2 and all(k[1] > 0 and 0 not in v for k, v in up.items()), (name, up)
    for name in ("chain_mixed", "ilu_chain_mixed"):
        f = lc.facts(name, 304)
        assert f["launches"][1] == ("chain", (32, 8, 1))
        for l in (1, 2, 3):
            (lane, wave, hub), in_one_wave, owners = f["tiles"][(l, 0)]
            assert lane >= 1 and wave == 2 and in_one_wave == 2 and hub == 1 and owners[0] != 0
    f = lc.facts("hub_cols", 304)
    assert f["frontier_hubs"] == {0: 3, 1: 1}                               # three hubs appended by the seed, one by a step
    assert lc.facts("col_4096", 304)["frontier_hubs"] == {} and lc.facts("col_4097", 304)["frontier_hubs"] == {0: 1}
    assert 4097 % 1024 == 1                                                 # walk_hubs: the last chunk of the column holds one entry
    f = lc.facts("arrow_both", 304)
    assert f["frontier_hubs"] == {0: 1} and f["upper"]["frontier_hubs"] == {0: 1}
    assert [lc.facts(f"levels_{n}", 304)["sort_passes"] for n in (16, 17, 256, 257)] == [1, 2, 2, 3]


def _lengths(name):
    mat = lc.matrix(name)
    return np.diff(mat[1])


def test_pairs_differ_in_the_one_thing_they_are_a_pair_for():
    for T, strides in lc.TRSV_DOUBLING.items():
        a, b = f"stride_{T}_below", f"stride_{T}_at"
        la, lb = _lengths(a), _lengths(b)
        assert la.size == lb.size and np.flatnonzero(la != lb).tolist() == [la.size - 1] and lb[-1] == la[-1] + 1   # one entry more in the last row
        ma, mb = lc.matrix(a), lc.matrix(b)
        assert np.array_equal(ma[2][:ma[1][-2]], mb[2][:mb[1][-2]]) and np.array_equal(ma[3][:ma[1][-2]], mb[3][:mb[1][-2]])   # every other row is the same row
        fa, fb = lc.facts(a, 304), lc.facts(b, 304)
        assert int(la[lc.BASE:].sum()) == T * lc.R - 1 and int(lb[lc.BASE:].sum()) == T * lc.R
        assert (fa["launches"][1][1], fb["launches"][1][1]) == strides and strides[1] == 2 * strides[0]
        for k in fa:
            if k not in ("launches", "launches_no_chains", "tiles", "tiles_no_chains", "hubs", "hubs_no_chains", "waves", "waves_no_chains", "frontier_entries"):
                assert fa[k] == fb[k], (T, k)
        assert fa["launches"][0] == fb["launches"][0] and fa["frontier_entries"][1:] == fb["frontier_entries"][1:]
    for T, strides in lc.ILU_DOUBLING.items():
        if T == 1:                                                          # no level above 0 averages less than one pivot a row: see level_cases
            f = lc.facts("ilu_stride_1_below", 304)
            assert f["levels"] == 1 and f["launches"] == [("level", 1, 4, 75)] and lc.facts("ilu_stride_1_at", 304)["launches"][1][1] == 2
            continue
        a, b = f"ilu_stride_{T}_below", f"ilu_stride_{T}_at"
        la, lb = _lengths(a), _lengths(b)
        last = lc.SHORT + lc.R - 1
        assert np.flatnonzero(la != lb).tolist() == [last] and lb[last] == la[last] + 1
        fa, fb = lc.facts(a, 304), lc.facts(b, 304)
        assert (fa["launches"][1][1], fb["launches"][1][1]) == strides and strides[1] == 2 * strides[0]
        for mat, want in ((lc.matrix(a), T * lc.R - 1), (lc.matrix(b), T * lc.R)):
            n, rp, ci, va = mat
            rowid = np.repeat(np.arange(n), np.diff(rp))
            inlevel = (rowid >= lc.SHORT) & (rowid < lc.SHORT + lc.R)
            assert int(((ci < rowid) & inlevel).sum()) == want
    for k, a, b in ((4096, "col_4096", "col_4097"), (2048, "fan_2048", "fan_2049")):
        assert lc.matrix(a)[0] + 1 == lc.matrix(b)[0]
    assert lc.matrix("fan_2049")[0] <= 2114 and lc.matrix("fan_2049")[1][-1] <= 140000


def test_fan_resumes_exactly_where_the_first_grid_is_not_the_largest():
    for cus in lc.CUS:
        small, big = lc.facts("fan_2048", cus), lc.facts("fan_2049", cus)
        assert small["frontier_entries"][1] == lc.step_cap(lc.MIN_GRID, 304) == 131072 and big["frontier_entries"][1] == 131136
        assert small["resumes"] == 0 and small["batches"] == [16] and small["grids"] == [8]
        if 2 * cus > lc.MIN_GRID:
            assert lc.CASES["fan_2049"].declared["resumes"][1] == big["resumes"] == 1
            assert big["batches"] == [16, 32] and big["grids"] == [8, min(2 * cus, 64)] and big["host_waits"] == small["host_waits"] + 1
            assert big["launches_analysis"] == small["launches_analysis"] + 32
        else:
            assert lc.CASES["fan_2049"].declared["resumes"][0] == big["resumes"] == 0 and big["batches"] == [16]
    for name in lc.CASES:                                                   # nothing else resumes
        if name != "fan_2049":
            assert all(lc.facts(name, cus)["resumes"] == 0 for cus in lc.CUS), name


def _main_loop_trips(m, first, stride, unroll):
    """trsv.hip, strided_sum: `for (; k + (kUnroll - 1) * kStride < m; k += kUnroll * kStride)` from k = first"""
    k, trips = first, 0
    while k + (unroll - 1) * stride < m:
        k += unroll * stride
        trips += 1
    return trips


def test_unroll_edges_reach_every_split_of_every_instantiation():
    """(stride, unroll) of strided_sum<…, RhsVector, 1, 4>, <…, 64, 8>, <…, WG, 8> and strided_sum<…, RhsBlock<…>, 1, 2>, <…, 64, 4>, <…, WG, 4>, each on the rows
    of its class.
    A lane's main loop runs while k + (unroll − 1)·stride < m, in trips of unroll·stride entries. Per instantiation the lengths give lane 0 a smallest
    number of trips, one more and two more, and sit one entry short of a whole number of full trips, on it and one past it — where the LAST lane's trip
    count changes and the tail is empty, whole or one entry. The smallest number is zero wherever the class allows it; it cannot for the workgroup's
    rows (above 4096 entries they make two trips of 2048 and four of 1024 at least), and for <…, 64, 4> and <…, 1, 2> lane 0 makes no trip only below
    193 and 2 entries: those are the rows of 40, 50 and 1 entries that chain_mixed, hub_in_tile_* and every stride case hold."""
    lens = lc.UNROLL
    assert np.diff(lc.matrix("unroll_edges")[1])[6200:].tolist() == [m + 1 for m in lens]
    classes = {"lane": [m for m in lens if m <= 32], "wave": [m for m in lens if 32 < m <= 4096], "hub": [m for m in lens if m > 4096]}
    assert [len(v) for v in classes.values()] == [6, 12, 6]
    elsewhere = {"lane": [1], "wave": [40, 50], "hub": []}
    assert {1, 40, 50} <= set(lc.MIXED[0]) and {1, 40, 50} <= set(lc.SPECIAL) and {1, 40, 50} <= set(lc.hub_in_tile_counts(2))
    for cls, stride, unroll in (("lane", 1, 4), ("wave", 64, 8), ("hub", 256, 8), ("lane", 1, 2), ("wave", 64, 4), ("hub", 256, 4)):
        full = unroll * stride
        trips = {m: _main_loop_trips(m, 0, stride, unroll) for m in classes[cls]}
        least = 4097 // full if cls == "hub" else 0                         # lane 0 of the shortest row of the class
        assert least == _main_loop_trips(4097 if cls == "hub" else 1, 0, stride, unroll)
        have = set(trips.values()) | {_main_loop_trips(m, 0, stride, unroll) for m in elsewhere[cls]}
        assert {least, least + 1, least + 2} <= have or (cls == "hub" and min(have) == least and max(have) == 6144 // full), (cls, stride, unroll, trips)
        assert {1, 2} <= set(trips.values()) or cls == "hub"
        if (stride, unroll) in ((1, 4), (64, 8)):                           # the single-vector lane and wave sums: zero trips inside unroll_edges itself
            first = (unroll - 1) * stride + 1                               # the shortest row whose lane 0 enters the main loop
            assert trips[first - 1] == 0 and trips[first] == 1
        edges = [j * full for j in range(1, 7) if {j * full - 1, j * full, j * full + 1} <= set(trips)]
        assert edges, (cls, stride, unroll)                                 # one short of j full trips, on it, one past it
        for e in edges:                                                     # there the last lane makes its j-th trip, and lane 0 gets a tail of one entry
            assert _main_loop_trips(e - 1, stride - 1, stride, unroll) + 1 == _main_loop_trips(e, stride - 1, stride, unroll) == e // full
        if cls == "hub":                                                    # 4352 = 17 · 256: the last thread's tail is empty one below it and one entry on it
            assert {4351, 4352, 4353} <= set(trips) and 4352 % lc.WG == 0 and 4352 % full == lc.WG
    assert [_main_loop_trips(m, 0, 1, 2) for m in (3, 4, 5)] == [1, 2, 2] and [_main_loop_trips(m, 0, 1, 4) for m in (7, 8, 9)] == [1, 2, 2]


def test_restated_rules_agree_with_the_host_test_and_the_header():
    src = open(os.path.join(ROOT, "tests", "cpp", "level_schedule_test.cpp")).read()
    assert "the solve's stride doubles at an average of 8, 16, … 256" in src and "doubles at an average of 1, 2, … 32 lower entries" in src
    want = 1
    for avg in (8, 16, 32, 64, 128, 256):                                   # g_trsv_stride's loop
        assert lc.trsv_stride(1, avg - 1) == want and lc.trsv_stride(1, avg) == 2 * want
        assert lc.trsv_stride(3, 3 * avg - 1) == want and lc.trsv_stride(3, 3 * avg) == 2 * want
        assert lc.TRSV_DOUBLING[avg] == (want, 2 * want)
        want *= 2
    assert lc.trsv_stride(0, 0) == 1 and lc.trsv_stride(0, 1000) == 1 and lc.trsv_stride(5, 0) == 1
    assert lc.trsv_stride(1, 257) == 64 and lc.trsv_stride(1, 1 << 40) == 64 and lc.trsv_stride(300, 5100) == 4 and lc.trsv_stride(260, 66820) == 64
    want = 1
    for avg in (1, 2, 4, 8, 16, 32):                                        # h_ilu_stride's loop
        assert lc.ilu_stride(1, avg - 1) == want and lc.ilu_stride(1, avg) == 2 * want
        assert lc.ilu_stride(3, 3 * avg - 1) == want and lc.ilu_stride(3, 3 * avg) == 2 * want
        assert lc.ILU_DOUBLING[avg] == (want, 2 * want)
        want *= 2
    assert lc.ilu_stride(0, 1000) == 1 and lc.ilu_stride(7, 6) == 1 and lc.ilu_stride(7, 7) == 2 and lc.ilu_stride(1, 63) == 64 and lc.ilu_stride(300, 4800) == 32
    assert [lc.chain_stride(w) for w in lc.CHAIN_WIDTHS] == list(lc.CHAIN_STRIDES) and lc.chain_stride(255) == 1 and lc.chain_stride(3) == 64
    assert [lc.bits_of(v) for v in (0, 1, 15, 16, 255, 256, 2**31 - 1)] == [1, 1, 4, 5, 8, 9, 31]
    assert (lc.step_grid(0, 304), lc.step_grid(2048 * 9, 304), lc.step_grid(10**9, 304), lc.step_grid(10**9, 1)) == (8, 9, 608, 8)
    assert lc.step_cap(8, 304) == 131072 and lc.step_cap(608, 304) == lc.NO_CAP and lc.step_cap(8, 4) == lc.NO_CAP and lc.step_cap(8, 5) == 131072
    assert [lc.next_batch(b) for b in (16, 32, 64)] == [32, 64, 64]
    header = open(os.path.join(ROOT, "include", "g4s.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (G4S_\w+)\s+(\d+)u?\b", header)}
    assert (defs["G4S_TRSV_WAVE_ROW"], defs["G4S_ILU0_LANE_ROW"], defs["G4S_ILU0_WAVE_ROW"], defs["G4S_TRSV_CHAIN_WIDTH"]) == \
           (lc.TRSV_WAVE_ROW, lc.ILU_LANE_ROW, lc.ILU_WAVE_ROW, lc.WG)
    for text, path in (("constexpr int kHubCut = 4096;", "frontier.hpp"), ("constexpr long long kEdgesPerWg = 2048;", "step_batch.hpp"),
                       ("constexpr long long kGridGrowth = 8;", "step_batch.hpp"), ("constexpr int kMinGrid = 8;", "step_batch.hpp"),
                       ("constexpr int kBatchMax = 64;", "step_batch.hpp"), ("constexpr int kBatch = 16;", "trsv.hip"), ("constexpr int kLevelWg = 256;", "level_schedule.hpp"),
                       ("cnt->launches += 4 + 3 * ((bits_of(levels - 1) + 3) / 4) + 6;", "trsv.hip"), ("const g4s::StepGrid sized(g4s::kMinGrid, 2 * cus);", "trsv.hip")):
        assert text in open(os.path.join(ROOT, "g4s_amd", "csrc", path)).read(), text
    assert (tr.WAVE_ROW, tr.HUB_ROW, il.LANE_ROW, il.WAVE_ROW) == (lc.TRSV_WAVE_ROW, lc.HUB_CUT, lc.ILU_LANE_ROW, lc.ILU_WAVE_ROW)


def test_mirror_is_the_upper_twin():
    mat = lc.matrix("chain_mixed")
    up = tr.mirror(mat)
    n = mat[0]
    assert np.array_equal(tr.levels(*up, False)[::-1], tr.levels(*mat, True)) and tr.info(*up, False) == tr.info(*mat, True)
    back = tr.mirror(up)
    assert all(np.array_equal(a, b) for a, b in zip(back[1:], mat[1:]))
    _, b, x = lc.solved("chain_mixed")
    assert np.array_equal(tr.solve(*up, b[::-1], False)[::-1].view(np.int64), x.view(np.int64))   # the same rows in the same stored order: the same bits
    assert n == 4200 + 5 + 17 + 129


@pytest.mark.parametrize("name,lower", [("hub_in_tile_s16", True), ("chain_mixed", False), ("unroll_edges", True)])
def test_solve_reference_holds_on_the_new_shapes(name, lower):
    """|b − T x|_i <= γ (|T||x|)_i with γ = (m_i + 2)u / (1 − (m_i + 2)u) (Higham, Accuracy and Stability, §8.1): it holds for substitution in any
    summation order, so it needs no measured tolerance. Held in exact rationals for the reference's x, and for scipy's solve of the same triangle too:
    two substitutions in different orders, one bound"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve_triangular
    mat, b, x = lc.solved(name, lower)
    n, rp, ci, va = mat
    u = Fraction(1, 2**53)
    assert np.all(np.isfinite(x)) and np.max(np.abs(x)) < 64               # the scaling keeps x of size one
    want = spsolve_triangular(sp.csr_matrix((va, ci, rp), shape=(n, n)), b, lower=lower)
    for sol in (x, want):
        for i in range(n):
            ent = [(Fraction(float(va[k])), Fraction(float(sol[ci[k]]))) for k in range(rp[i], rp[i + 1])]
            m = len(ent) + 2
            assert abs(Fraction(float(b[i])) - sum(v * y for v, y in ent)) <= m * u / (1 - m * u) * sum(abs(v * y) for v, y in ent), (name, i)


@pytest.mark.parametrize("name", ["ilu_hub_in_tile_s2", "ilu_chain_mixed", "arrow_both"])
def test_ilu_reference_holds_on_the_new_shapes(name):
    """(L U)_ij = a_ij on the pattern, within the componentwise bound of an inner product of the terms that make it up (γ_k for k terms): the defining
    property of ILU(0), with no measured tolerance"""
    import scipy.sparse as sp
    mat, f, bad, r, z = lc.factored(name)
    n, rp, ci, va = mat
    assert bad == -1 and np.all(np.isfinite(f)) and np.all(np.isfinite(z)) and np.max(np.abs(z)) < 64
    F = sp.csr_matrix((f, ci, rp), shape=(n, n))
    L = sp.tril(F, -1).tocsr() + sp.identity(n, format="csr")
    U = sp.triu(F, 0).tocsr()
    A = sp.csr_matrix((va, ci, rp), shape=(n, n))
    P = sp.csr_matrix((np.ones_like(va), ci, rp), shape=(n, n))
    prod = (L @ U).multiply(P).tocsr()
    bound = (abs(L) @ abs(U)).multiply(P).tocsr()
    k = int(np.diff(rp).max()) + 2
    gamma = 2 * k * 2.0**-53                                                # k terms summed by the factorisation, and k more roundings in this check's own product
    diff = abs(prod - A)
    assert (diff - gamma * bound).max() <= 0.0, name
