"""What pins tests/trsv_ref.py, and what of g4s_sptrsv_* can be checked without a device: the reference against scipy's spsolve_triangular with == on
integer-exact inputs, Higham's componentwise residual bound on random diagonally dominant inputs (it holds for substitution in any summation order, so
it needs no measured tolerance), the levels against a longest-path computation, the chaining rule on hand-made level widths, the layout of
g4s_trsv_info, the signatures and the flag values of capi, and every refusal of the Python layer that comes before the first GPU call."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import trsv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy_triangle(mat, lower, unit):
    import scipy.sparse as sp
    n, rp, ci, va = mat
    a = sp.csr_matrix((va, ci, rp), shape=(n, n))                          # repeats are summed, which is exact on these inputs
    t = sp.tril(a, 0) if lower else sp.triu(a, 0)
    if unit:
        t = t - sp.diags(t.diagonal()) + sp.identity(n)
    return sp.csr_matrix(t)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_reference_equals_scipy_on_exact_inputs(lower, unit):
    from scipy.sparse.linalg import spsolve_triangular
    for seed, diag in ((9, 2.0), (10, 4.0), (11, 0.5)):
        mat = ref.exact_case(48, seed, diag)
        assert int(ref.levels(*mat, lower, unit).max()) <= 2
        b = np.random.default_rng(seed).integers(-8, 9, mat[0]).astype(np.float64)
        want = spsolve_triangular(_scipy_triangle(mat, lower, unit), b, lower=lower, unit_diagonal=unit)
        got = ref.solve(*mat, b, lower, unit)
        assert np.array_equal(got, want)


def test_exact_case_is_exact_through_three_symmetric_sweeps():
    """the Gauss–Seidel tests compare with ==: every intermediate of the sweeps must be a dyadic rational that fp64 holds, whatever the order of a sum"""
    mat = ref.exact_case()
    n, rp, ci, va = mat
    b = np.random.default_rng(5).integers(-4, 5, n).astype(np.float64)
    a = [[Fraction(0)] * n for _ in range(n)]
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            a[i][ci[k]] += Fraction(float(va[k]))
    x = [Fraction(0)] * n
    for _ in range(3):
        for lower in (True, False):
            r = [Fraction(float(b[i])) - sum(a[i][j] * x[j] for j in range(n)) for i in range(n)]
            y = [Fraction(0)] * n
            for i in (range(n) if lower else range(n - 1, -1, -1)):
                dep = range(i) if lower else range(i + 1, n)
                y[i] = (r[i] - sum(a[i][j] * y[j] for j in dep)) / a[i][i]
            x = [p + q for p, q in zip(x, y)]
            for v in x + y + r:
                assert v.denominator & (v.denominator - 1) == 0 and abs(v.numerator).bit_length() <= 40, v   # far inside 53 bits, products included
    got = ref.gauss_seidel(*mat, b, np.zeros(n), 3, True)
    assert [Fraction(float(v)) for v in got] == x


@pytest.mark.parametrize("name", ["dense_lower_70", "grid40", "blocks", "wave_row_edges", "hub_row", "messy", "bidiagonal_cap_plus_1"])
def test_componentwise_residual_bound(name):
    """|b − T x|_i <= γ (|T||x|)_i with γ = (m_i + 2)u / (1 − (m_i + 2)u), m_i the stored triangle entries of row i (Higham, Accuracy and Stability, §8.1)"""
    u = Fraction(1, 2**53)
    for lower in (True, False):
        mat, _, _, b, x = ref.case(name, lower)
        n = mat[0]
        off, dia = ref.triangle(*mat, lower)
        for i in range(n):
            ent = [(Fraction(float(v)), Fraction(float(x[c]))) for c, v, _ in off[i]] + [(Fraction(float(v)), Fraction(float(x[i]))) for v, _ in dia[i]]
            m = len(ent) + 2
            res = abs(Fraction(float(b[i])) - sum(v * y for v, y in ent))
            assert res <= m * u / (1 - m * u) * sum(abs(v * y) for v, y in ent), (name, lower, i)


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_levels_are_the_longest_paths(name):
    import networkx as nx
    for lower in (True, False):
        mat, lev, info, _, _ = ref.case(name, lower)
        n = mat[0]
        off, _ = ref.triangle(*mat, lower)
        g = nx.DiGraph()
        g.add_nodes_from(range(n))
        g.add_edges_from((c, i) for i in range(n) for c, _, _ in off[i])
        depth = {}
        for v in nx.topological_sort(g):
            depth[v] = 1 + max((depth[p] for p in g.predecessors(v)), default=-1)
        assert [depth[v] for v in range(n)] == lev.tolist()
        assert info["levels"] == (nx.dag_longest_path_length(g) + 1 if n else 0)
        order, loff = ref.schedule(lev)
        assert sorted(order.tolist()) == list(range(n)) and all((lev[a], a) < (lev[b], b) for a, b in zip(order[:-1], order[1:]))
        assert all(np.all(lev[order[loff[l]:loff[l + 1]]] == l) for l in range(info["levels"]))


def test_the_named_cases_reach_the_edges_they_are_named_for():
    assert ref.case("grid40")[2]["levels"] == 79 and np.bincount(ref.case("grid40")[1]).tolist() == list(range(1, 41)) + list(range(39, 0, -1))
    for name, lv in (("bidiagonal_cap_minus_1", ref.CHAIN_LEVELS - 1), ("bidiagonal_cap", ref.CHAIN_LEVELS), ("bidiagonal_cap_plus_1", ref.CHAIN_LEVELS + 1)):
        i = ref.case(name)[2]
        assert (i["levels"], i["chains"], i["launches_per_solve"]) == (lv, 1 + (lv > ref.CHAIN_LEVELS), 1 + (lv > ref.CHAIN_LEVELS))
    i = ref.case("blocks")[2]
    assert np.bincount(ref.case("blocks")[1]).tolist() == [255, 256, 257, 256, 255, 257, 5] and (i["launches_per_solve"], i["chains"]) == (5, 3)
    i = ref.case("dense_lower_70")[2]
    assert (i["levels"], i["widest_level"], i["chains"]) == (70, 1, 1)
    assert ref.case("diagonal_300")[2]["chains"] == 0 and ref.case("diagonal_300")[2]["launches_per_solve"] == 1
    off, _ = ref.triangle(*ref.case("wave_row_edges")[0])
    assert [len(o) for o in off[70:]] == [31, 32, 33, 63, 64, 65]
    off, dia = ref.triangle(*ref.case("hub_row")[0])
    assert [len(o) for o in off[-2:]] == [ref.HUB_ROW + 1, ref.HUB_ROW]
    for name, rows, m in (("strided_tiles", 300, 16), ("wave_tiles", 260, 256)):   # level 1 is one launch, with chains or without: wider than a chain
        (n, rp, ci, va), lev, i, _, _ = ref.case(name)
        assert np.bincount(lev).tolist() == [m, rows] and rows > ref.CHAIN_WIDTH and np.diff(rp)[m:].tolist() == [m + 1] * rows
        assert (i["launches_per_solve"], i["chains"], i["nnz_triangle"] - m) == (2, 1, rows * (m + 1))
    mat = ref.case("messy")[0]
    off, dia = ref.triangle(*mat)
    assert max(len(d) for d in dia) == 3 and any(len({c for c, _, _ in o}) < len(o) for o in off)
    assert any([c for c, _, _ in o] != sorted(c for c, _, _ in o) for o in off)
    assert ref.case("n0")[2]["launches_per_solve"] == 0


def test_chaining_rule_on_level_widths():
    def plan(widths, no_chains=False):
        return ref.launch_plan(np.repeat(np.arange(len(widths)), widths).astype(np.int32), no_chains)
    W, L = ref.CHAIN_WIDTH, ref.CHAIN_LEVELS
    assert plan([1]) == [(0, 1, True)] and plan([W + 1]) == [(0, 1, False)] and plan([]) == []
    assert plan([W, W + 1, 1, 1, W + 1, W + 1, 2]) == [(0, 1, True), (1, 2, False), (2, 4, True), (4, 5, False), (5, 6, False), (6, 7, True)]
    assert plan([1] * (2 * L + 1)) == [(0, L, True), (L, 2 * L, True), (2 * L, 2 * L + 1, True)]
    assert plan([1, W + 1, 1], True) == [(0, 1, False), (1, 2, False), (2, 3, False)]


def test_row_sum_shapes():
    """the three shapes, on values whose order of summation shows: 1, 2^-53 repeated"""
    tiny = np.float64(2.0**-53)
    assert ref.row_sum([]) == 0.0 and np.signbit(ref.row_sum([np.float64(-0.0)])) == False   # noqa: E712  — the sum starts from +0.0
    p = [np.float64(1.0)] + [tiny] * 31
    assert ref.row_sum(p) == 1.0                                            # one lane, left to right: every tiny term is rounded away
    p = [np.float64(1.0)] + [tiny] * 63
    assert ref.row_sum(p) == 1.0 + 31 * 2.0**-52                              # the ladder adds the tiny terms among themselves first: only lane 32's is lost
    p = [np.float64(1.0)] + [tiny] * 4999
    part = [np.float64(0.0)] * 256
    for k, v in enumerate(p):
        part[k % 256] += v
    w = [ref._ladder(part[64 * j:64 * j + 64]) for j in range(4)]
    assert ref.row_sum(p) == ((w[0] + w[1]) + w[2]) + w[3] and ref.row_sum(p) != ref._ladder(ref._strided(p, 64))


def test_capi_struct_signatures_and_flags():
    from g4s_amd import capi
    assert C.sizeof(capi.TRSVInfo) == 48
    assert [n for n, _ in capi.TRSVInfo._fields_] == ["nnz_triangle", "n", "levels", "widest_level", "launches_per_solve", "chains", "bad_row", "launches",
                                                     "host_waits", "resumes", "reserved"]
    assert capi.TRSVInfo.nnz_triangle.offset == 0 and capi.TRSVInfo.n.offset == 8 and capi.TRSVInfo.bad_row.offset == 28 and capi.TRSVInfo.resumes.offset == 40
    header = open(os.path.join(ROOT, "include", "g4s.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (G4S_TRSV_\w+)\s+(\d+)u?\b", header)}
    assert defs == {"G4S_TRSV_UPPER": capi.TRSV_UPPER, "G4S_TRSV_UNIT_DIAGONAL": capi.TRSV_UNIT_DIAGONAL, "G4S_TRSV_NO_CHAINS": capi.TRSV_NO_CHAINS,
                    "G4S_TRSV_WAVE_ROW": capi.TRSV_WAVE_ROW, "G4S_TRSV_CHAIN_WIDTH": capi.TRSV_CHAIN_WIDTH, "G4S_TRSV_CHAIN_LEVELS": capi.TRSV_CHAIN_LEVELS}
    assert (capi.TRSV_WAVE_ROW, capi.TRSV_CHAIN_WIDTH, capi.TRSV_CHAIN_LEVELS, capi.TRSV_HUB_ROW) == (ref.WAVE_ROW, ref.CHAIN_WIDTH, ref.CHAIN_LEVELS, ref.HUB_ROW)
    flags = [capi.TRSV_UPPER, capi.TRSV_UNIT_DIAGONAL, capi.TRSV_NO_CHAINS]
    others = [capi.DEVICE_POINTERS, capi.SORT_OUTPUT, capi.SPMV_NO_NT, capi.SPMV_BLOCKED, capi.SPMV_STREAM, capi.DIST_LOOPBACK, capi.DIST_ALLGATHER, capi.SPMV_UPDATABLE,
              capi.SPMM_COL_MAJOR, capi.SEMIRING_MASK, capi.SPMV_ACCUMULATE, capi.TRAVERSE_PUSH, capi.TRAVERSE_PULL, capi.TRAVERSE_SYMMETRIC, capi.CC_SYMMETRIC,
              capi.PAGERANK_SYMMETRIC, capi.PAGERANK_WARM_START, capi.BC_ACCUMULATE, capi.COLOR_LARGEST_FIRST, capi.MSF_MAXIMUM]
    assert all(f & (f - 1) == 0 for f in flags) and len(set(flags)) == 3 and all(f & o == 0 for f in flags for o in others)
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_sptrsv_analyse"] == (C.c_int, [C.POINTER(vp), C.c_int32, vp, vp, vp, vp, C.c_uint, C.POINTER(capi.TRSVInfo), vp])
    assert capi.SIGNATURES["g4s_sptrsv_solve"] == (C.c_int, [vp, vp, vp, vp])
    assert capi.SIGNATURES["g4s_sptrsv_update_values"] == (C.c_int, [vp, vp, C.c_uint, vp])
    assert capi.SIGNATURES["g4s_sptrsv_get_info"] == (C.c_int, [vp, C.POINTER(capi.TRSVInfo)])
    assert capi.SIGNATURES["g4s_sptrsv_destroy"] == (C.c_int, [vp])
    lib = capi.load()
    for name in ("g4s_sptrsv_analyse", "g4s_sptrsv_solve", "g4s_sptrsv_update_values", "g4s_sptrsv_get_info", "g4s_sptrsv_destroy"):
        assert getattr(lib, name).argtypes == capi.SIGNATURES[name][1]


def test_c_refusals_that_come_before_any_hip_call():
    """the argument checks of the entry points return before the first HIP call, so they can be asked without a device"""
    from g4s_amd import capi
    lib = capi.load()
    rp, ci, va = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0])
    P = lambda a: C.c_void_p(a.ctypes.data)
    h = C.c_void_p(0x1234)
    for args, text in (((C.byref(h), 1, P(rp), P(ci), P(va), None, 2, None, None), "flags"),
                       ((C.byref(h), 1, P(rp), P(ci), P(va), None, capi.TRSV_NO_CHAINS << 1, None, None), "flags"),
                       ((None, 1, P(rp), P(ci), P(va), None, 0, None, None), "out is NULL"),
                       ((C.byref(h), -1, P(rp), P(ci), P(va), None, 0, None, None), "negative"),
                       ((C.byref(h), 1, None, P(ci), P(va), None, 0, None, None), "rowptr is NULL"),
                       ((C.byref(h), 1, P(rp), None, P(va), None, 0, None, None), "colids or values"),
                       ((C.byref(h), 1, P(rp), P(ci), None, None, 0, None, None), "colids or values"),
                       ((C.byref(h), 1, P(rp), P(ci), P(va), P(ci), 0, None, None), "overlap")):
        assert lib.g4s_sptrsv_analyse(*args) == capi.ERR_INVALID and text in lib.g4s_last_error().decode(), text
        assert h.value == 0x1234                                            # *out is untouched
    assert lib.g4s_sptrsv_solve(None, None, None, None) == capi.ERR_INVALID
    assert lib.g4s_sptrsv_update_values(None, None, 0, None) == capi.ERR_INVALID
    assert lib.g4s_sptrsv_get_info(None, None) == capi.ERR_INVALID
    assert lib.g4s_sptrsv_destroy(None) == capi.OK


def test_python_refusals_need_no_device():
    import torch
    from g4s_amd import host
    rp, ci, va = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 1.0])
    for bad in ((rp, ci), (rp, ci, va, va), (rp, ci, va[:1]), (rp, torch.zeros(2, dtype=torch.int32), va), (np.zeros(0, np.int32), ci, va)):
        with pytest.raises(ValueError):
            host.sptrsv_analyse(bad)
    for kw in ({"lower": 1}, {"unit_diagonal": "yes"}, {"return_level": None}, {"no_chains": 0}):
        with pytest.raises(ValueError, match="must be a bool"):
            host.sptrsv_analyse((rp, ci, va), **kw)
    with pytest.raises(ValueError, match="must be a bool"):
        host.spsolve_triangular((rp, ci, va), np.ones(2), lower=1)
    with pytest.raises(ValueError, match="b must have 2 entries"):
        host.spsolve_triangular((rp, ci, va), np.ones(3))

    class Rect:                                                             # what _pattern_of reads of a CSR
        rows, cols, rowptr, colids, values = 2, 3, rp, ci, va
    with pytest.raises(ValueError, match="square"):
        host.sptrsv_analyse(Rect())
    with pytest.raises(ValueError, match="A must be a CSR"):
        host.gauss_seidel((rp, ci, va), None, None)
    plan = host.TriangularPlan(None, 2, 2, __import__("g4s_amd.capi", fromlist=["x"]).TRSVInfo())
    assert "reserved" not in plan.info and plan.info["levels"] == 0
    with pytest.raises(ValueError, match="closed"):
        plan.solve(torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="closed"):
        plan.update_values(va)
