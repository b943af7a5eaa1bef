"""g4s_pagerank on the GPU against the longdouble reference of tests/pagerank_ref.py, after the same number of iterations.

The accuracy bound, derived rather than measured. Every quantity of an iteration is non-negative, so a sum of k terms computed in ANY order carries a
relative error of at most (depth)·u, u = 2⁻⁵³, where depth is the largest number of additions a term passes through — no cancellation, whatever the
grouping (a sequential row sum, a butterfly over lanes, the blocked path's LDS atomics). Per iteration and per component:
    x_u = r_u · (1 / s_u)        s_u is a sum of out-degree terms, then one division and one product: (max_out_degree + 1)·u
    y_v = Σ a_uv · x_u           one product per term and a sum of in-degree terms: max_in_degree·u on top
    m   = Σ_{dangling} r_u       ⌈n / (G·256)⌉ terms per thread, 6 shuffle levels, 4 waves and the G = min(⌈n / 2048⌉, 512) partials added in index
                                 order: depth·u with depth = ⌈n / (G·256)⌉ + 6 + 4 + G (tests/iteration_cases.py, sum_depth). While the grid is far below
                                 its cap that is 8 terms per thread and n / 2048 partials, below (⌈log₂ n⌉ + 8)·u for n <= 2¹⁴ — the default of
                                 pagerank_ref.gamma. Under the capped grid (G = 512, more than 8 terms per thread) the 512 partials alone pass the
                                 default, and the tests that go there (tests/test_pagerank_limits_gpu.py) hand gamma the depth read off the code.
                                 The residual Σ|r' − r| is summed the same way.
    r'  = d·(y + m·p) + (1 − d)·p, with p = pers / Σ pers: seven more roundings
so r'_v is computed with a relative error of at most γ = (max_in_degree + max_out_degree + depth + 8)·u (⌈log₂ n⌉ + 16 by default), i.e. the computed step is
T(r) + e with ‖e‖₁ <= γ·‖r'‖₁ = γ (the ranks sum to one). T contracts in L1 by d = damping (it is d times a column-stochastic map plus a constant), hence
E_k <= d·E_{k−1} + γ <= γ / (1 − d) for every k: a float64 run and the exact iteration differ by at most γ / (1 − damping) in L1 after the same
number of iterations, and so does |Σr − 1|. The longdouble reference's own error is 2⁻¹¹ of that. A float64 numpy run of 60 iterations sits at
3–6·2⁻⁵³ — the bound is loose by about 10³ and still a million times below the effect of one missed edge or a mishandled dangling vertex."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import pagerank_ref
from tests.pagerank_ref import csr_of_edges, gamma

pytestmark = pytest.mark.gpu

ITERS = 30


def _host():
    from g4s_amd import capi, host
    return capi, host


def _from_arrays(arrays, **kw):
    _, host = _host()
    rp, ci, va = arrays
    n = len(rp) - 1
    return host.CSR.from_host(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64), n, n, **kw)


def _dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def _bound(ref, n, damping, depth=None):
    """depth: the depth of the mass and residual sums where the default of gamma does not cover it (the module's docstring)"""
    return gamma(n, ref.max_in_degree, ref.max_out_degree, depth) / (1.0 - damping)


def _compare(label, r, want, ref, n, damping, depth=None):
    """err <= γ / (1 − d) and |Σr − 1| under the same bound; returns err / bound."""
    got = r.cpu().numpy().astype(np.longdouble)
    err, off = float(np.abs(got - want).sum()), abs(float(got.sum() - np.longdouble(1)))
    bound = _bound(ref, n, damping, depth)
    print(f"pagerank {label}: n {n}, L1 err {err:.3e}, |sum - 1| {off:.3e}, bound {bound:.3e}, err / bound {err / bound:.2e}")
    assert err <= bound, (label, err, bound)
    assert off <= bound, (label, off, bound)
    return err / bound


def _run_fixed(label, A, arrays, iters=ITERS, damping=0.85, pers=None, ref=None, symmetric=False, start=None, depth=None):
    rp, ci, va = arrays
    n = len(rp) - 1
    if ref is None:
        ref = pagerank_ref.pagerank(rp, ci, va, n, damping=damping, tol=0.0, max_iterations=iters, personalization=pers, start=start)
    r, info = A.pagerank(damping=damping, tol=0.0, max_iterations=iters, personalization=_dev(pers), start=_dev(start), symmetric=symmetric)
    print(f"pagerank {label}: {info}")
    assert info["iterations"] == iters == len(ref.residuals) and info["converged"] == 0, info
    assert info["dangling"] == ref.dangling, (info, ref.dangling)
    assert abs(info["residual"] - float(ref.residuals[-1])) <= 2 * _bound(ref, n, damping, depth)
    _compare(label, r, ref.rank, ref, n, damping, depth)
    return r, info, ref


@pytest.fixture(scope="module")
def rmat14():
    arrays = pagerank_ref.rmat_csr(14, 16, 20260114)
    rp, ci, va = arrays
    ref = pagerank_ref.pagerank(rp, ci, va, 1 << 14, tol=0.0, max_iterations=ITERS, keep=(10, 15))
    assert ref.max_in_degree > 2048 and ref.dangling > 1000           # long-row chunks and the fix-up take part; thousands of dangling vertices
    return arrays, ref


@pytest.fixture(scope="module")
def rmat10():
    arrays = pagerank_ref.rmat_csr(10, 8, 77)
    return arrays


def _banded(n=6000, offsets=(-2, 1, 3, 10)):
    src = np.concatenate([np.arange(n)[(np.arange(n) + o >= 0) & (np.arange(n) + o < n)] for o in offsets])
    dst = np.concatenate([(np.arange(n) + o)[(np.arange(n) + o >= 0) & (np.arange(n) + o < n)] for o in offsets])
    order = np.lexsort((dst, src))
    return csr_of_edges(n, src[order], dst[order], np.random.default_rng(9).uniform(0.5, 2.0, src.size))


def _blocks(nb=900, b=3):
    """A pattern of aligned dense b×b blocks: block row i holds the blocks (i, i) and (i, j) for a few random j; weights U[0.5, 2)."""
    rng = np.random.default_rng(21)
    cols = [np.unique(np.concatenate([[i], rng.integers(0, nb, 5)])) for i in range(nb)]
    src = np.concatenate([np.repeat(np.arange(b) + i * b, len(c) * b) for i, c in enumerate(cols)])
    dst = np.concatenate([np.tile((c[:, None] * b + np.arange(b)[None, :]).ravel(), b) for c in cols])
    return csr_of_edges(nb * b, src, dst, rng.uniform(0.5, 2.0, src.size))


# ---------------------------------------------------------------------------------------------- 1. every SpMV path of Aᵀ
@pytest.mark.parametrize("path_flag,path", [("SPMV_STREAM", 0), ("SPMV_BLOCKED", 1)])
def test_rmat_streaming_and_blocked_paths(rmat14, path_flag, path):
    capi, _ = _host()
    arrays, ref = rmat14
    A = _from_arrays(arrays, spmv_flags=getattr(capi, path_flag))
    _run_fixed(f"rmat14 path {path}", A, arrays, ref=ref)
    assert A.transpose_info()["spmv_path"] == path                    # a silent fallback fails here
    assert A.transpose_info()["long_rows"] > 0 or path == 1


def test_diagonal_and_block_row_paths():
    for label, arrays, path in (("banded", _banded(), 3), ("3x3 blocks", _blocks(), 4)):
        A = _from_arrays(arrays)
        r, info, ref = _run_fixed(label, A, arrays)
        assert A.transpose_info()["spmv_path"] == path, label
        r2, info2 = A.pagerank(tol=0.0, max_iterations=ITERS)         # 6. reproducible on these paths
        assert torch.equal(r, r2) and info2["residual"] == info["residual"]


# ---------------------------------------------------------------------------------------------- 2. sizes at kernel boundaries
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049, 5000])
def test_sizes_at_kernel_boundaries(n):
    """5000 is no multiple of the epilogue's 256 threads × 8 entries; 2049 is one past a full workgroup's share (two workgroups)."""
    rng = np.random.default_rng(n)
    m = 4 * n
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = src % 7 != 3 if n > 1 else np.ones(m, bool)                # some dangling vertices
    arrays = csr_of_edges(n, src[keep], dst[keep], rng.uniform(0.5, 2.0, int(keep.sum())))
    _run_fixed(f"random n={n}", _from_arrays(arrays, spmv_flags=_host()[0].SPMV_STREAM), arrays, iters=12)


def test_no_edges_no_dangling_all_dangling():
    capi, _ = _host()
    n = 64                                                            # a power of two: every operation is exact and r == p bit for bit
    empty = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    A = _from_arrays(empty)
    r, info, _ = _run_fixed("nnz == 0", A, empty, iters=9)
    assert torch.equal(r, torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")) and info["dangling"] == n and info["products"] == 0
    r, info = A.pagerank(damping=0.5, tol=1e-3)
    assert info["converged"] == 1 and info["iterations"] == 1 and info["residual"] == 0.0
    for n2 in (100, 3000):
        e2 = (np.zeros(n2 + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        _run_fixed(f"nnz == 0, n={n2}", _from_arrays(e2), e2, iters=5, pers=np.random.default_rng(n2).uniform(0, 1, n2))
    # stored zeros only: every vertex dangles although no row is empty
    n3 = 500
    zeros = csr_of_edges(n3, np.arange(n3), (np.arange(n3) + 1) % n3, np.zeros(n3))
    r, info, _ = _run_fixed("all weights zero", _from_arrays(zeros, spmv_flags=capi.SPMV_STREAM), zeros, iters=6)
    assert info["dangling"] == n3
    # no dangling vertex: a cycle plus chords
    n4 = 1000
    ring = csr_of_edges(n4, np.concatenate([np.arange(n4), np.arange(0, n4, 3)]), np.concatenate([(np.arange(n4) + 1) % n4, (np.arange(0, n4, 3) * 7) % n4]),
                        np.random.default_rng(4).uniform(0.5, 2.0, n4 + len(range(0, n4, 3))))
    r, info, _ = _run_fixed("no dangling vertex", _from_arrays(ring, spmv_flags=capi.SPMV_STREAM), ring)
    assert info["dangling"] == 0


# ---------------------------------------------------------------------------------------------- 3. personalisation
def test_personalization(rmat10):
    capi, _ = _host()
    arrays = rmat10
    n = len(arrays[0]) - 1
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM)
    one = np.zeros(n)
    one[17] = 3.0
    some = np.random.default_rng(8).uniform(0.0, 1.0, n)
    some[::3] = 0.0
    for label, pers in (("one entry", one), ("with zeros", some)):
        r, _, _ = _run_fixed(f"personalised, {label}", A, arrays, pers=pers)
        r8, _ = A.pagerank(tol=0.0, max_iterations=ITERS, personalization=_dev(pers * 8.0))
        assert torch.equal(r, r8), label                              # a power of two normalises exactly
    neg, nan, inf = some.copy(), some.copy(), some.copy()
    neg[5], nan[6], inf[7] = -1e-3, math.nan, math.inf
    for label, pers in (("negative", neg), ("NaN", nan), ("inf", inf), ("all zero", np.zeros(n))):
        with pytest.raises(capi.G4SError) as e:
            A.pagerank(personalization=_dev(pers))
        assert e.value.status == capi.ERR_INVALID and "personalization" in str(e.value), label
    _run_fixed("after the refusals", A, arrays, pers=some)


# ---------------------------------------------------------------------------------------------- 4. stop test, 6. reproducibility (streaming)
def test_stop_rule_and_no_ops_behind_the_stop(rmat14):
    capi, _ = _host()
    arrays, ref = rmat14
    n = len(arrays[0]) - 1
    k = 11
    before, at = float(ref.residuals[k - 2]), float(ref.residuals[k - 1])
    assert before >= 1.5 * at                                         # the two residuals the tolerance sits between are well apart
    tol = math.sqrt(before * at)
    rp, ci, va = arrays
    ref_k = pagerank_ref.pagerank(rp, ci, va, n, tol=tol, max_iterations=0)
    assert len(ref_k.residuals) == k
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM)
    r, info = A.pagerank(tol=tol)
    print(f"pagerank stop: {info}, reference residual {at:.6e}")
    assert info["iterations"] == k and info["converged"] == 1, info
    assert abs(info["residual"] - at) <= 2 * _bound(ref, n, 0.85)
    assert info["products"] >= k and info["host_waits"] <= 2 + k // capi.PAGERANK_BATCH
    _compare("stopped by tol", r, ref_k.rank, ref, n, 0.85)
    r2, info2 = A.pagerank(tol=0.0, max_iterations=k)
    assert info2["iterations"] == k and info2["converged"] == 0
    assert torch.equal(r, r2) and info2["residual"] == info["residual"]   # iterations enqueued behind the stop are no-ops
    r3, info3 = A.pagerank(tol=tol)
    assert torch.equal(r, r3) and info3["residual"] == info["residual"] and info3["iterations"] == k


# ---------------------------------------------------------------------------------------------- 5. the loop lives on the device
def test_loop_on_the_device():
    capi, host = _host()
    L = host.laplacian_csr(5, 48, 48)
    rp, ci, _ = L.to_host()
    arrays = (rp, ci, np.ones(ci.size))
    A = _from_arrays(arrays)
    iters = 80
    r, info, _ = _run_fixed("grid, damping 0.99", A, arrays, iters=iters, damping=0.99)
    assert A.transpose_info()["spmv_path"] == 3
    assert info["host_waits"] <= 2 + info["iterations"] // capi.PAGERANK_BATCH, info
    assert info["products"] == iters
    cap = capi.PAGERANK_BATCH - 3
    r, info, _ = _run_fixed("cap below the batch", A, arrays, iters=cap, damping=0.99)
    assert info["converged"] == 0 and info["iterations"] == cap and info["products"] == cap and info["host_waits"] == 1


# ---------------------------------------------------------------------------------------------- 7. warm start
def test_warm_start(rmat14):
    capi, _ = _host()
    arrays, ref = rmat14
    n = len(arrays[0]) - 1
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM)
    start = ref.kept[10].astype(np.float64)
    t = _dev(start)
    r, info = A.pagerank(tol=0.0, max_iterations=5, start=t)
    assert info["iterations"] == 5 and torch.equal(t, _dev(start))    # the caller's tensor is not modified
    _compare("warm start 10 -> 15", r, ref.kept[15], ref, n, 0.85)
    r8, info8 = A.pagerank(tol=0.0, max_iterations=5, start=_dev(start * 8.0))
    assert torch.equal(r, r8) and info8["residual"] == info["residual"]
    for bad in (-1.0, math.nan):
        s2 = start.copy()
        s2[3] = bad
        with pytest.raises(capi.G4SError) as e:
            A.pagerank(start=_dev(s2))
        assert e.value.status == capi.ERR_INVALID and "starting vector" in str(e.value)
    with pytest.raises(capi.G4SError):
        A.pagerank(start=_dev(np.zeros(n)))


# ---------------------------------------------------------------------------------------------- 8. g4s_csr_update_values
@pytest.mark.parametrize("path_flag", ["SPMV_STREAM", "HOST_POINTERS"])
def test_update_values(rmat10, path_flag):
    capi, _ = _host()
    rp, ci, va = rmat10
    A = _from_arrays((rp, ci, va), spmv_flags=getattr(capi, path_flag) | capi.SPMV_UPDATABLE)   # forced streaming, and the library's own choice
    _run_fixed("before the update", A, (rp, ci, va))
    va2 = np.random.default_rng(12).uniform(0.1, 5.0, va.size)
    va2[rp[40]:rp[41]] = 0.0                                          # a row that now dangles
    A.update_values(_dev(va2))
    _, info, ref2 = _run_fixed("after the update", A, (rp, ci, va2))  # a stale 1 / s fails here
    bad = va2.copy()
    bad[11] = -0.5
    A.update_values(_dev(bad))
    with pytest.raises(capi.G4SError) as e:
        A.pagerank()
    assert e.value.status == capi.ERR_INVALID and "value" in str(e.value)
    A.update_values(_dev(va2))
    _run_fixed("after the repair", A, (rp, ci, va2), ref=ref2)


# ---------------------------------------------------------------------------------------------- 9. G4S_PAGERANK_SYMMETRIC
def test_symmetric_flag_builds_no_transpose(rmat10):
    capi, _ = _host()
    rp, ci, va = rmat10
    n = len(rp) - 1
    src = np.repeat(np.arange(n), np.diff(rp))
    arrays = csr_of_edges(n, np.concatenate([src, ci]), np.concatenate([ci, src]), np.concatenate([va, va]))
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM)
    A.pagerank_reserve(symmetric=True)
    _run_fixed("symmetrised", A, arrays, symmetric=True)
    with pytest.raises(capi.G4SError):
        A.transpose_info()                                            # still no transpose on that handle


# ---------------------------------------------------------------------------------------------- 10. contract corners
def test_contract_corners(rmat10):
    capi, host = _host()
    lib = capi.load()
    rp, ci, va = rmat10
    n = len(rp) - 1
    A = _from_arrays((rp, ci, va), spmv_flags=capi.SPMV_STREAM)
    bytes0 = A.info()["plan_bytes"]
    A.pagerank_reserve()
    bytes1 = (A.info()["plan_bytes"], A.transpose_info()["plan_bytes"])
    assert bytes1[0] >= bytes0 + 8 * 4 * n                            # 1 / s, x, y and the normalised p
    r, info, ref = _run_fixed("after the reserve", A, (rp, ci, va))
    A.pagerank(personalization=_dev(np.arange(n, dtype=np.float64)), start=r)
    assert (A.info()["plan_bytes"], A.transpose_info()["plan_bytes"]) == bytes1
    # a non-square handle
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    R = host.CSR.from_host(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 1.0]), 2, 3)
    assert lib.g4s_pagerank(R.handle, 0.85, 1e-10, 0, None, C.c_void_p(out.data_ptr()), 0, None, None) == capi.ERR_INVALID
    assert lib.g4s_csr_pagerank_reserve(R.handle, 0) == capi.ERR_INVALID
    with pytest.raises(ValueError, match="square"):
        R.pagerank()
    # a capturing stream is refused, the capture stays valid and the handle still multiplies
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_pagerank(A.handle, 0.85, 1e-10, 0, None, C.c_void_p(out.data_ptr()), 0, None, C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and "captured" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    v = np.random.default_rng(1).uniform(0, 1, n)
    got = A.spmv_transpose(_dev(v)).cpu().numpy()
    want = np.zeros(n)
    np.add.at(want, ci, va * v[np.repeat(np.arange(n), np.diff(rp))])
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    _run_fixed("after the refused capture", A, (rp, ci, va), ref=ref)


# ---------------------------------------------------------------------------------------------- 11. against networkx
def test_against_networkx(rmat10):
    import networkx as nx
    capi, _ = _host()
    rp, ci, va = rmat10
    n = len(rp) - 1
    damping, tol_nx = 0.85, 1e-12
    G = nx.MultiDiGraph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from(zip(np.repeat(np.arange(n), np.diff(rp)).tolist(), ci.tolist(), va.tolist()))
    pr = nx.pagerank(G, alpha=damping, max_iter=1000, tol=tol_nx, weight="weight")
    want = np.array([pr[v] for v in range(n)])
    A = _from_arrays((rp, ci, va))
    r, info = A.pagerank(damping=damping, tol=1e-11)
    assert info["converged"] == 1
    max_in, max_out = int(np.bincount(ci, minlength=n).max()), int(np.diff(rp).max())
    bound = (n * tol_nx + info["residual"]) * damping / (1.0 - damping) + gamma(n, max_in, max_out) / (1.0 - damping)
    dist = float(np.abs(r.cpu().numpy() - want).sum())
    print(f"pagerank vs networkx: {info}, L1 distance {dist:.3e}, bound {bound:.3e}")
    assert dist <= bound
