"""The cases of the concurrency tests (tests/concurrency_cases.py), checked without a GPU: the condition under which every comparison may be ==
(Σ|a·b| per output entry below 2^53, integer values), the sizes the scenarios rely on, and the expected results against scipy where scipy has the
operation — and against the references of this directory called the way the other tests call them."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import components_ref, masked_ref, semiring_ref
from tests import concurrency_cases as cc

EXACT = float(2 ** 53)


def _sp(A, n):
    return sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n), copy=True)


def _at(C, rows, cols):
    """the values of the scipy matrix C at (rows, cols), 0.0 where it stores nothing"""
    C = C.tocsr()
    C.sort_indices()
    n = np.int64(C.shape[1])
    key = masked_ref.mask_rows(C.indptr) * n + C.indices.astype(np.int64)
    want = np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64)
    pos = np.minimum(np.searchsorted(key, want), max(key.size - 1, 0))
    return np.where(key[pos] == want, C.data[pos], 0.0)


@pytest.mark.parametrize("i", range(3))
def test_products_are_exact_and_match_scipy(i):
    P = cc.products()[i]
    assert 1 << 13 <= P.n <= 1 << 16
    for A in (P.A, P.A2):
        assert np.array_equal(A[2], np.round(A[2])) and np.abs(A[2]).max() <= 4
    assert P.abs_sum_bound < EXACT
    # scipy drops the entries whose sum is 0.0, so the pattern is that of the product of the patterns (all ones: nothing cancels), and the values are
    # looked up at it (an entry scipy dropped reads as 0.0, which is its value)
    ones = sp.csr_matrix((np.ones(P.nnz), P.A[1], P.A[0]), shape=(P.n, P.n))
    C1 = (ones @ ones).tocsr()
    C1.sort_indices()
    assert np.array_equal(C1.indptr, P.crpt) and np.array_equal(C1.indices, P.ccol)
    crow = masked_ref.mask_rows(P.crpt)
    for second in (False, True):
        S = _sp(P.A2 if second else P.A, P.n)
        assert np.array_equal(_at(S @ S, crow, P.ccol), P.cval("plus_times", second))
    # the masked plus-times product on the mask A is (A·A) ∘ pattern(A)
    S = _sp(P.A, P.n)
    rows = masked_ref.mask_rows(P.A[0])
    assert np.array_equal(_at(S @ S, rows, P.A[1]), P.masked("plus_times"))
    assert np.array_equal(_at(ones @ ones, rows, P.A[1]), P.masked("plus_times", True))
    assert P.masked_products == int((ones @ np.diff(P.A[0]).astype(np.float64)).sum())
    # components, transpose, SpMV, triangles
    lab, k = components_ref.scipy_labels(P.A[0], P.A[1], P.n)
    assert np.array_equal(lab, P.labels) and P.cc_stats[0] == k
    T = S.T.tocsr()
    assert np.array_equal(T.indptr, P.transpose[0]) and np.array_equal(T.indices, P.transpose[1]) and np.array_equal(T.data, P.transpose[2])
    assert np.array_equal(P.A[2][P.transpose[3]], P.transpose[2])
    assert np.array_equal(2.0 * (S @ P.x) - 3.0 * P.y0, P.spmv)
    G = sp.csr_matrix((np.ones(len(P.graph[1])), P.graph[1], P.graph[0]), shape=(P.n, P.n))
    assert P.triangles == masked_ref.triangles_trace(G)
    # shortest paths and levels
    from scipy.sparse.csgraph import dijkstra
    W, src = P.weights
    assert np.array_equal(dijkstra(_sp(W, P.n), directed=True, indices=src), P.sssp)      # integer weights: every path sum is exact
    E = _sp(P.A, P.n)
    E.eliminate_zeros()
    E.data[:] = 1.0
    hops = dijkstra(E, directed=True, indices=src, unweighted=True)
    assert np.array_equal(np.where(np.isinf(hops), -1, hops).astype(np.int32), P.bfs)


def test_shared_sort_agrees_with_the_references_called_directly():
    """concurrency_cases expands and sorts the products of a problem once; the references, called as the other tests call them, give the same arrays"""
    P = cc.products()[0]
    for s in cc.SEMIRINGS:
        crpt, ccol, cval = semiring_ref.spgemm(P.A, P.A, P.n, s)
        assert np.array_equal(crpt, P.crpt) and np.array_equal(ccol, P.ccol) and np.array_equal(cval, P.cval(s))
        assert np.array_equal(masked_ref.spgemm_masked(P.A, P.A, P.n, P.n, (P.A[0], P.A[1]), s)[0], P.masked(s))
    assert np.array_equal(masked_ref.spgemm_masked(P.A, P.A, P.n, P.n, (P.A[0], P.A[1]), "plus_times", True)[0], P.masked("plus_times", True))


def test_two_outputs_fit_each_others_cached_block():
    """big_alloc hands out a cached block for a request it fits within 25 %: the outputs of the first two problems are that close, and they have
    the same shape (the in-place scenario rewrites one into the other)"""
    a, b = cc.products()[:2]
    assert a.n == b.n
    lo, hi = sorted((a.cnnz, b.cnnz))
    assert hi - lo <= lo // 4, (a.cnnz, b.cnnz)
    assert len({p.cnnz for p in cc.products()}) == 3
    big = cc.products()[2]
    assert (big.row_flop > 8192).sum() > 0                           # rows long enough for the column scratch / the cut-carrying classes


def test_every_call_runs_on_every_problem():
    """the mixes of threads_synchronous_calls: six threads, eight rounds of five calls, and every call of OP_NAMES meets each of the three problems
    (sssp and bfs through the handle its thread owns: problem t % 3)"""
    assert cc.THREADS == len(cc.STRIDES) <= 6 and len(cc.products()) == 3
    assert all(np.gcd(s, len(cc.OP_NAMES)) == 1 for s in cc.STRIDES)
    met = {name: set() for name in cc.OP_NAMES}
    for t in range(cc.THREADS):
        rounds = cc.schedule(t)
        assert len(rounds) == cc.ROUNDS and all(len(r) == cc.OPS_PER_ROUND for r in rounds)
        for op, p in (job for r in rounds for job in r):
            met[cc.OP_NAMES[op]].add(t % 3 if cc.OP_NAMES[op] in ("sssp", "bfs") else p)
    assert all(ps == {0, 1, 2} for ps in met.values()), met
    assert cc.schedule(0) != cc.schedule(1)


@pytest.mark.parametrize("i", range(4))
def test_handles_are_exact_and_match_scipy(i):
    H = cc.handles()[i]
    assert 1 << 13 <= H.n <= 1 << 16
    assert np.array_equal(H.A[2], np.round(H.A[2])) and H.abs_sum_bound < EXACT
    S = _sp(H.A, H.n)
    for r in (0, cc.ROUNDS - 1):
        i_, e = H.inputs(r), H.expected(r)
        assert np.array_equal(S @ i_["x"], e["spmv"]) and np.array_equal(S @ i_["X"], e["spmm"]) and np.array_equal(S.T @ i_["xt"], e["transpose"])
        dense_rows = np.flatnonzero(np.diff(H.A[0]) > 0)[:50]                    # min-plus with accumulate, a sample of rows by hand
        for row in dense_rows:
            k0, k1 = H.A[0][row], H.A[0][row + 1]
            assert e["min_plus_acc"][row] == min(i_["y_acc"][row], np.min(H.A[2][k0:k1] + i_["x"][H.A[1][k0:k1]]))
    assert not np.array_equal(H.inputs(0)["x"], H.inputs(1)["x"])               # fresh inputs every round


def test_invalid_inputs_are_invalid_in_one_place():
    P = cc.products()[0]
    bad_ci, bad_mask = cc.invalid_inputs()
    assert (bad_ci >= P.n).sum() == 1 and (bad_ci != P.A[1]).sum() == 1
    assert (bad_mask != P.A[1]).sum() == 2 and np.array_equal(np.sort(bad_mask), np.sort(P.A[1]))
    descents = sum(int((np.diff(bad_mask[P.A[0][r]:P.A[0][r + 1]]) <= 0).sum()) for r in range(P.n))
    assert descents == 1
