"""g4s_ilu0_* without a device: the numpy restatement (tests/ilu_ref.py) against dense LU, exact rationals and the defining property of ILU(0) —
(L U)_ij = a_ij at every stored position —, the named cases against the edges they are named for, the ctypes table against the header, and the
refusals of the C entry points and of the Python layer that come before any HIP call."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import ilu_ref as ref
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE = sorted(set(ref.CASES) - {"zero_pivot", "specials"})


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", FINITE)
def test_product_of_the_factors_equals_a_on_the_pattern(name):
    """|a_ij − Σ_k l_ik u_kj| <= γ Σ_k |l_ik| |u_kj| over the k <= min(i, j) whose (i, k) and (k, j) are both stored, l_ii = 1, with
    γ = (m + 2)u / (1 − (m + 2)u) and m the number of terms: every stored value is c − Σ a_k b_k, divided or not, subtracted in order (Higham,
    Accuracy and Stability, Lemma 8.4)"""
    (n, rp, ci, va), f, _, _, _ = ref.case(name)
    u = Fraction(1, 2**53)
    at = {(i, int(ci[q])): q for i in range(n) for q in range(rp[i], rp[i + 1])}
    for i in range(n):
        lower = [(int(ci[q]), Fraction(float(f[q]))) for q in range(rp[i], rp[i + 1]) if ci[q] < i]
        for q in range(rp[i], rp[i + 1]):
            j = int(ci[q])
            terms = [l * Fraction(float(f[at[k, j]])) for k, l in lower if k <= j and (k, j) in at]
            if j >= i:
                terms.append(Fraction(float(f[q])))
            m = len(terms) + 2
            assert abs(Fraction(float(va[q])) - sum(terms)) <= m * u / (1 - m * u) * sum(abs(t) for t in terms), (name, i, j)


def test_full_pattern_equals_dense_lu_without_pivoting():
    """on a full pattern nothing is dropped: the bits of the kij elimination on a dense array, whose every element takes its updates in ascending k too"""
    for name in ("dense_70", "n1"):
        (n, rp, ci, va), f, info, _, _ = ref.case(name)
        a = tr.dense(n, rp, ci, va)
        for k in range(n):
            for i in range(k + 1, n):
                a[i, k] = a[i, k] / a[k, k]
                a[i, k + 1:] = a[i, k + 1:] - a[i, k] * a[k, k + 1:]
        assert np.array_equal(_bits(a.reshape(-1)), _bits(f)) and info["bad_pivot"] == -1
        L, U = ref.split(n, rp, ci, f)
        assert np.allclose(L @ U, tr.dense(n, rp, ci, va), rtol=1e-13, atol=1e-13)


def test_exact_case_is_exact():
    (n, rp, ci, va), L0, U0 = ref.exact_full()
    f, bad = ref.factor(n, rp, ci, va)
    L, U = ref.split(n, rp, ci, f)
    assert bad == -1 and np.array_equal(L, L0) and np.array_equal(U, U0)
    w = [[Fraction(float(va[i * n + j])) for j in range(n)] for i in range(n)]   # the same loop in exact rationals
    for i in range(n):
        for k in range(i):
            w[i][k] = w[i][k] / w[k][k]
            for j in range(k + 1, n):
                w[i][j] = w[i][j] - w[i][k] * w[k][j]
    assert all(Fraction(float(f[i * n + j])) == w[i][j] for i in range(n) for j in range(n))
    r = np.arange(1.0, n + 1.0)
    z = ref.apply(n, rp, ci, f, r)
    assert np.allclose(tr.dense(n, rp, ci, va) @ z, r, rtol=1e-9, atol=1e-9)      # L U = A here: the apply is the solve


def _dropped(n, rp, ci):
    at = {(i, int(ci[q])) for i in range(n) for q in range(rp[i], rp[i + 1])}
    return sum(1 for i in range(n) for q in range(rp[i], rp[i + 1]) if ci[q] < i
               for t in range(rp[ci[q]], rp[ci[q] + 1]) if ci[t] > ci[q] and (i, int(ci[t])) not in at)


def test_the_named_cases_reach_the_edges_they_are_named_for():
    for name in ref.CASES:
        mat = ref.case(name)[0]
        assert ref.refusal(*mat[:3]) is None, name
    i = ref.case("grid40")[2]
    lev = tr.levels(*ref.case("grid40")[0], True, True)
    assert i["levels"] == 79 and np.bincount(lev).tolist() == list(range(1, 41)) + list(range(39, 0, -1)) and i["nnz"] == 5 * 1600 - 4 * 40
    for name, lv in (("tridiagonal_cap_minus_1", ref.CHAIN_LEVELS - 1), ("tridiagonal_cap", ref.CHAIN_LEVELS), ("tridiagonal_cap_plus_1", ref.CHAIN_LEVELS + 1)):
        i = ref.case(name)[2]
        chains = 1 + (lv > ref.CHAIN_LEVELS)
        assert (i["levels"], i["chains"], i["launches_per_factor"], i["launches_per_apply"]) == (lv, chains, chains, 2 * chains)
    i = ref.case("blocks")[2]
    assert np.bincount(tr.levels(*ref.case("blocks")[0], True, True)).tolist() == [255, 256, 257, 256, 255, 257, 5]
    assert (i["launches_per_factor"], i["chains"]) == (5, 3) and _dropped(*ref.case("blocks")[0][:3]) > 0
    i = ref.case("dense_70")[2]
    assert (i["levels"], i["widest_level"], i["chains"], i["nnz"]) == (70, 1, 1, 4900) and ref.LANE_ROW < 64 < 70 <= ref.WAVE_ROW
    i = ref.case("diagonal_300")[2]
    assert (i["levels"], i["chains"], i["launches_per_factor"], i["launches_per_apply"]) == (1, 0, 1, 2)
    assert ref.case("n0")[2]["launches_per_factor"] == 0 and ref.case("n0")[2]["launches_per_apply"] == 0
    for stem, limit in (("arrow_lane", ref.LANE_ROW), ("arrow_wave", ref.WAVE_ROW)):
        for suffix, n in (("_minus_1", limit - 1), ("", limit), ("_plus_1", limit + 1)):
            (m, rp, ci, va), _, i, _, _ = ref.case(stem + suffix)
            assert m == n and int(np.diff(rp).max()) == n == rp[n] - rp[n - 1] and np.all(np.diff(rp)[:-1] <= 4) and i["levels"] == 2
            assert np.all(ci[rp[:-1] + np.diff(rp) - 1] == n - 1)                 # the last column is full
    (n, rp, ci, va), _, i, _, _ = ref.case("two_long_rows")
    assert np.diff(rp)[-2:].tolist() == [ref.WAVE_ROW + 9] * 2 and np.diff(rp)[:-2].max() <= 5 and (i["levels"], i["widest_level"]) == (2, ref.WAVE_ROW + 8)
    assert tr.levels(n, rp, ci, va, True, True)[-2:].tolist() == [1, 1]
    (n, rp, ci, va), _, i, _, _ = ref.case("strided_tiles")
    lev = tr.levels(n, rp, ci, va, True, True)
    assert np.bincount(lev).tolist() == [16, 300] and np.diff(rp)[16:].tolist() == [17] * 300 and (i["launches_per_factor"], i["chains"]) == (2, 1)
    assert ref.LANE_ROW < 17 <= ref.WAVE_ROW and 300 > ref.CHAIN_WIDTH and np.all(ci[rp[16:-1]] == 0) and np.all(ci[rp[17:] - 2] == 15)   # 16 pivots a row
    assert np.diff(rp)[:16].max() == 4 and rp[16] > 3 * 16                    # the pivot rows have entries behind their diagonals
    n, rp, ci, va = ref.case("row0_full")[0]
    assert rp[1] == n == 200 and np.all(ci[rp[1:-1]] == 0) and np.diff(rp)[1:].max() > ref.LANE_ROW and np.diff(rp)[1:].min() == 2
    assert _dropped(n, rp, ci) > 150 * 190
    n, rp, ci, va = ref.case("messy")[0]
    assert n == 60 and _dropped(n, rp, ci) > 100 and not np.array_equal(tr.dense(n, rp, ci, va) != 0, (tr.dense(n, rp, ci, va) != 0).T)
    (n, rp, ci, va), f, i, _, z = ref.case("zero_pivot")
    assert i["bad_pivot"] == 2 and f[rp[2] + 1] == 0.0 and np.isinf(f[rp[3]:rp[4]]).all() and np.isnan(f[rp[4] + 1]) and np.isnan(f[rp[4] + 2])
    assert np.signbit(f[rp[5] + 1]) and f[rp[5] + 1] == 0.0 and np.all(np.isfinite(f[rp[5]:]))
    assert np.all(_bits(f[np.isnan(f)]) == 0x7FF8000000000000) and np.isnan(z).any()
    (n, rp, ci, va), f, i, _, _ = ref.case("specials")
    assert np.isnan(va).sum() == 1 and np.isinf(va).sum() == 1 and np.isnan(f).any() and np.all(_bits(f[np.isnan(f)]) == 0x7FF8000000000000)


def test_refusals_of_the_reference():
    n, rp, ci, va = ref.case("messy")[0]
    swap = np.array(ci)
    k = int(rp[7])
    assert rp[8] - rp[7] >= 2
    swap[k], swap[k + 1] = ci[k + 1], ci[k]
    assert ref.refusal(n, rp, swap) == ("order", 7)
    rep = np.array(ci)
    rep[k + 1] = rep[k]
    assert ref.refusal(n, rp, rep)[0] in ("order", "diag") and ref.refusal(n, rp, rep)[1] == 7
    out = np.array(ci)
    out[int(rp[30])] = n
    assert ref.refusal(n, rp, out) == ("id", 30)
    r2 = np.array(rp)
    r2[0] = 1
    assert ref.refusal(n, r2, ci) == ("rowptr", -1)
    assert ref.refusal(2, np.array([0, 1, 2]), np.array([0, 0])) == ("diag", 1)


def test_preconditioned_cg_of_the_reference():
    """the restated loop converges on the grid Laplacian with and without the factors, in fewer than half the iterations with them"""
    (n, rp, ci, va), f, _, _, _ = ref.case("grid40")
    b = np.random.default_rng(40).uniform(-1.0, 1.0, n)
    a = tr.dense(n, rp, ci, va)
    x0, it0, res0 = ref.pcg(n, rp, ci, va, b, None)
    x1, it1, res1 = ref.pcg(n, rp, ci, va, b, f)
    print("reference pcg iterations:", it0, it1)
    for x in (x0, x1):
        assert np.linalg.norm(b - a @ x) <= 1e-9 * np.linalg.norm(b)
    assert it1 < it0 / 2 and res0 <= 1e-10 and res1 <= 1e-10


def test_capi_struct_signatures_and_flags():
    from g4s_amd import capi
    assert C.sizeof(capi.ILU0Info) == 48
    assert [n for n, _ in capi.ILU0Info._fields_] == ["nnz", "n", "levels", "widest_level", "launches_per_factor", "chains", "launches_per_apply", "bad_row",
                                                     "bad_pivot", "launches", "host_waits"]
    assert capi.ILU0Info.nnz.offset == 0 and capi.ILU0Info.n.offset == 8 and capi.ILU0Info.bad_row.offset == 32 and capi.ILU0Info.host_waits.offset == 44
    header = open(os.path.join(ROOT, "include", "g4s.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (G4S_ILU0_\w+)\s+(\d+)u?\b", header)}
    assert defs == {"G4S_ILU0_NO_CHAINS": capi.ILU0_NO_CHAINS, "G4S_ILU0_LANE_ROW": capi.ILU0_LANE_ROW, "G4S_ILU0_WAVE_ROW": capi.ILU0_WAVE_ROW}
    assert (capi.ILU0_LANE_ROW, capi.ILU0_WAVE_ROW) == (ref.LANE_ROW, ref.WAVE_ROW)
    others = [capi.DEVICE_POINTERS, capi.TRSV_UPPER, capi.TRSV_UNIT_DIAGONAL, capi.TRSV_NO_CHAINS, capi.SORT_OUTPUT, capi.SPMV_NO_NT, capi.SPMV_BLOCKED,
              capi.SPMV_STREAM, capi.DIST_LOOPBACK, capi.DIST_ALLGATHER, capi.SPMV_UPDATABLE, capi.SPMM_COL_MAJOR, capi.SEMIRING_MASK, capi.SPMV_ACCUMULATE,
              capi.TRAVERSE_PUSH, capi.TRAVERSE_PULL, capi.TRAVERSE_SYMMETRIC, capi.CC_SYMMETRIC, capi.PAGERANK_SYMMETRIC, capi.PAGERANK_WARM_START,
              capi.BC_ACCUMULATE, capi.COLOR_LARGEST_FIRST, capi.MSF_MAXIMUM]
    f = capi.ILU0_NO_CHAINS
    assert f & (f - 1) == 0 and all(f & o == 0 for o in others)
    vp = C.c_void_p
    want = {"g4s_ilu0_analyse": (C.c_int, [C.POINTER(vp), C.c_int32, vp, vp, vp, C.c_uint, C.POINTER(capi.ILU0Info), vp]),
            "g4s_ilu0_factor": (C.c_int, [vp, vp, C.c_uint, vp, vp]),
            "g4s_ilu0_apply": (C.c_int, [vp, vp, vp, vp]),
            "g4s_ilu0_get_factors": (C.c_int, [vp, vp, C.c_uint, vp]),
            "g4s_ilu0_get_info": (C.c_int, [vp, C.POINTER(capi.ILU0Info)]),
            "g4s_ilu0_destroy": (C.c_int, [vp])}
    lib = capi.load()
    for name, sig in want.items():
        assert capi.SIGNATURES[name] == sig and getattr(lib, name).argtypes == sig[1], name


def test_c_refusals_that_come_before_any_hip_call():
    """the argument checks of the entry points return before the first HIP call, so they can be asked without a device"""
    from g4s_amd import capi
    lib = capi.load()
    rp, ci, va = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0])
    neg = np.array([0, -1], np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    h = C.c_void_p(0x1234)
    for args, text in (((C.byref(h), 1, P(rp), P(ci), P(va), 2, None, None), "flags"),
                       ((C.byref(h), 1, P(rp), P(ci), P(va), capi.TRSV_NO_CHAINS, None, None), "flags"),
                       ((C.byref(h), 1, P(rp), P(ci), P(va), capi.ILU0_NO_CHAINS << 1, None, None), "flags"),
                       ((None, 1, P(rp), P(ci), P(va), 0, None, None), "out is NULL"),
                       ((C.byref(h), -1, P(rp), P(ci), P(va), 0, None, None), "negative"),
                       ((C.byref(h), 1, None, P(ci), P(va), 0, None, None), "rowptr is NULL"),
                       ((C.byref(h), 1, P(rp), None, P(va), 0, None, None), "colids or values"),
                       ((C.byref(h), 1, P(rp), P(ci), None, 0, None, None), "colids or values"),
                       ((C.byref(h), 1, P(neg), P(ci), P(va), 0, None, None), "rowptr[n] is negative")):
        assert lib.g4s_ilu0_analyse(*args) == capi.ERR_INVALID and text in lib.g4s_last_error().decode(), text
        assert h.value == 0x1234                                            # *out is untouched
    assert lib.g4s_ilu0_factor(None, None, 0, None, None) == capi.ERR_INVALID
    assert lib.g4s_ilu0_apply(None, None, None, None) == capi.ERR_INVALID
    assert lib.g4s_ilu0_get_factors(None, None, 0, None) == capi.ERR_INVALID
    assert lib.g4s_ilu0_get_info(None, None) == capi.ERR_INVALID
    assert lib.g4s_ilu0_destroy(None) == capi.OK


def test_python_refusals_need_no_device():
    import torch
    from g4s_amd import capi, host
    rp, ci, va = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 1.0])
    for bad in ((rp, ci), (rp, ci, va, va), (rp, ci, va[:1]), (rp, torch.zeros(2, dtype=torch.int32), va), (np.zeros(0, np.int32), ci, va)):
        with pytest.raises(ValueError):
            host.ilu0(bad)
    with pytest.raises(ValueError, match="must be a bool"):
        host.ilu0((rp, ci, va), no_chains=1)

    class Rect:                                                             # what _pattern_of reads of a CSR
        rows, cols, rowptr, colids, values = 2, 3, rp, ci, va
    with pytest.raises(ValueError, match="square"):
        host.ilu0(Rect())
    with pytest.raises(ValueError, match="A must be a CSR"):
        host.pcg((rp, ci, va), None)
    M = host.ILU0(None, 2, 2, capi.ILU0Info())
    assert M.info["levels"] == 0 and set(M.info) == {n for n, _ in capi.ILU0Info._fields_}
    for call in (lambda: M.apply(torch.zeros(2, dtype=torch.float64)), lambda: M.factor(), lambda: M.factors()):
        with pytest.raises(ValueError, match="closed"):
            call()
    M.close()
