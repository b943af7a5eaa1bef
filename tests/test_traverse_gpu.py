"""g4s_sssp / g4s_bfs on the GPU: every direction (auto, forced push, forced pull) equals the numpy reference of tests/traverse_ref.py bit for bit, on
R-MAT graphs (every SpMV path of Aᵀ), a grid (hundreds of steps: the loop must live on the device), a chain, a hub, the corner cases of the contract,
negative weights, value updates, and the host loops of INTEGRATION.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import traverse_ref
from tests.traverse_ref import same_values

pytestmark = pytest.mark.gpu

DIRECTIONS = ("auto", "push", "pull")


def _host():
    from g4s_amd import capi, host
    return capi, host


def _from_arrays(rp, ci, va, n, **kw):
    _, host = _host()
    return host.CSR.from_host(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64), n, n, **kw)


def _csr_of_edges(n, src, dst, w):
    """CSR by out-edges of an edge list, in the given order inside a row (duplicates kept)."""
    src, dst, w = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.float64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    return np.cumsum(rp).astype(np.int32), dst[order].astype(np.int32), w[order]


def _check_sssp(A, arrays, sources, directions=DIRECTIONS, symmetric=False, ref=None):
    rp, ci, va = arrays
    n = len(rp) - 1
    if ref is None:
        ref = traverse_ref.sssp(rp, ci, va, n, sources)
    d_ref, rounds, converged, _ = ref
    assert converged
    out = {}
    for direction in directions:
        d, info = A.sssp(sources, direction=direction, symmetric=symmetric)
        d = d.cpu().numpy()
        print(f"sssp {direction}: {info}")
        assert same_values(d, d_ref), (direction, int(np.sum(d != d_ref)), info)
        assert info["converged"] == 1 and info["reached"] == int(np.isfinite(d_ref).sum()), (direction, info)
        assert info["iterations"] == info["push_steps"] + info["pull_steps"]
        if direction == "push":
            assert info["pull_steps"] == 0
        if direction == "pull":
            assert info["push_steps"] == 0 and info["iterations"] == rounds and info["edges_relaxed"] == rounds * len(ci)
        out[direction] = info
    return d_ref, out


def _check_bfs(A, arrays, sources, directions=DIRECTIONS, symmetric=False):
    rp, ci, va = arrays
    n = len(rp) - 1
    l_ref, depth = traverse_ref.bfs(rp, ci, va, n, sources)
    out = {}
    for direction in directions:
        lv, info = A.bfs(sources, direction=direction, symmetric=symmetric)
        assert lv.dtype == torch.int32
        lv = lv.cpu().numpy()
        print(f"bfs {direction}: {info}")
        assert np.array_equal(lv, l_ref), (direction, int(np.sum(lv != l_ref)), info)
        assert info["converged"] == 1 and info["reached"] == int((l_ref >= 0).sum()), (direction, info)
        assert info["iterations"] == depth + 1                    # the step after the deepest level finds nothing
        out[direction] = info
    return l_ref, out


@pytest.fixture(scope="module")
def rmat():
    """R-MAT 2^16 with weights U[0.05, 1): (rowptr, colids, values) on the host and the vertex of largest out-degree."""
    _, host = _host()
    G = host.rmat_csr(1 << 16, 16, 10 << 16, 20240611)
    rp, ci, _ = G.to_host()
    va = np.random.default_rng(5).uniform(0.05, 1.0, ci.size)
    return (rp, ci, va), int(np.argmax(np.diff(rp)))


@pytest.fixture(scope="module")
def rmat_ref(rmat):
    (rp, ci, va), src = rmat
    return traverse_ref.sssp(rp, ci, va, len(rp) - 1, [src], keep=(2,))


@pytest.mark.parametrize("path_flag,path", [("auto", None), ("SPMV_BLOCKED", 1), ("SPMV_STREAM", 0)])
def test_sssp_rmat_every_direction_and_path(rmat, rmat_ref, path_flag, path):
    from scipy.sparse.csgraph import dijkstra
    import scipy.sparse as sp
    capi, _ = _host()
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n, spmv_flags=0 if path is None else getattr(capi, path_flag))
    d_ref, _ = _check_sssp(A, (rp, ci, va), [src], ref=rmat_ref)
    if path is not None:
        assert A.transpose_info()["spmv_path"] == path
    assert np.array_equal(d_ref, dijkstra(sp.csr_matrix((va, ci, rp), shape=(n, n)), directed=True, indices=src))


def _grid(nx):
    """The pattern of the 5-point stencil on nx × nx with weights U[0.05, 1) (the Laplacian's own values would make negative cycles)."""
    _, host = _host()
    L = host.laplacian_csr(5, nx, nx)
    rp, ci, _ = L.to_host()
    return rp, ci, np.random.default_rng(17).uniform(0.05, 1.0, ci.size)


def test_sssp_grid_loop_lives_on_the_device():
    capi, _ = _host()
    rp, ci, va = _grid(300)
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n)
    _, infos = _check_sssp(A, (rp, ci, va), [0])
    assert A.transpose_info()["spmv_path"] == 3
    push = infos["push"]
    B = capi.TRAVERSE_BATCH
    assert B >= 8 and push["iterations"] > 300
    assert push["host_waits"] * B <= push["iterations"] + 2 * B, push
    _check_bfs(A, (rp, ci, va), [0])


def test_chain_and_iteration_caps(rmat, rmat_ref):
    n = 4096
    rp, ci, va = _csr_of_edges(n, np.arange(n - 1), np.arange(1, n), np.random.default_rng(2).uniform(0.05, 1.0, n - 1))
    A = _from_arrays(rp, ci, va, n)
    exact = np.concatenate([[0.0], np.cumsum(va)])                  # left to right, as every path sum
    for direction in DIRECTIONS:
        d, info = A.sssp([0], direction=direction)
        assert same_values(d.cpu().numpy(), exact) and info["converged"] == 1
        assert abs(info["iterations"] - 4095) <= 1, info
        d, info = A.sssp([0], max_iterations=100, direction=direction)
        d = d.cpu().numpy()
        assert info["converged"] == 0 and info["iterations"] == 100, info
        assert same_values(d[:101], exact[:101]) and np.all(np.isinf(d[101:]))
        lv, info = A.bfs([0], max_depth=100, direction=direction)
        lv = lv.cpu().numpy()
        assert info["converged"] == 0 and np.array_equal(lv[:101], np.arange(101)) and np.all(lv[101:] == -1)
    (rp, ci, va), src = rmat
    d_ref, _, _, after = rmat_ref
    R = _from_arrays(rp, ci, va, len(rp) - 1)
    for direction in DIRECTIONS:
        d, info = R.sssp([src], max_iterations=2, direction=direction)
        d = d.cpu().numpy()
        assert info["converged"] == 0 and info["iterations"] == 2, info
        assert np.all(d_ref <= d) and np.all(d <= after[2]), direction


def test_hub_forced_push():
    leaves = 200_000
    n = leaves + 1
    leaf = np.arange(1, n)
    src = np.concatenate([np.zeros(leaves, np.int64), leaf, leaf])
    dst = np.concatenate([leaf, np.zeros(leaves, np.int64), np.where(leaf + 1 < n, leaf + 1, 1)])
    w = np.random.default_rng(8).uniform(0.05, 1.0, src.size)
    rp, ci, va = _csr_of_edges(n, src, dst, w)
    A = _from_arrays(rp, ci, va, n)
    _check_sssp(A, (rp, ci, va), [0], directions=("push",))
    _check_bfs(A, (rp, ci, va), [0], directions=("push",))
    _check_sssp(A, (rp, ci, va), [5], directions=("push", "auto"))


def test_corner_cases():
    # 0 → 1 (0.5), 0 → 1 (0.25: repeated column, the minimum wins), 1 → 2 (0.0: SSSP an edge of length 0, BFS no edge), 2 → 2 (self-loop), 2 → 3,
    # 4 → 0 (4 has no in-edge: unreachable), row 3 and row 5 empty, 6 → 7 (a second component), 3 → 1 (back edge)
    edges = [(0, 1, 0.5), (0, 1, 0.25), (1, 2, 0.0), (2, 2, 0.125), (2, 3, 0.75), (4, 0, 0.3), (6, 7, 0.1), (3, 1, 0.2), (0, 3, 1.5)]
    n = 8
    rp, ci, va = _csr_of_edges(n, [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges])
    A = _from_arrays(rp, ci, va, n)
    d_ref, _ = _check_sssp(A, (rp, ci, va), [0])
    assert d_ref[1] == 0.25 and d_ref[2] == 0.25 and d_ref[3] == 1.0 and np.isinf(d_ref[[4, 5, 6, 7]]).all()
    l_ref, _ = _check_bfs(A, (rp, ci, va), [0])
    assert list(l_ref) == [0, 1, -1, 1, -1, -1, -1, -1]                                   # 1 → 2 has weight 0: not an edge for BFS
    for sources in ([0, 6, 0, 6, 6], [5], [3, 5], [7, 7], [4]):                           # repeats, no out-edges, several components
        _check_sssp(A, (rp, ci, va), sources)
        _check_bfs(A, (rp, ci, va), sources)
    # random graph with empty rows, self-loops, repeated columns and zero weights, several sources
    rng = np.random.default_rng(23)
    n, m = 3000, 12000
    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    s[s % 7 == 3] = 0                                                                    # rows ≡ 3 (mod 7) are empty
    w = rng.uniform(0.05, 1.0, m)
    w[rng.integers(0, m, 400)] = 0.0
    s, t, w = np.concatenate([s, s[:2000]]), np.concatenate([t, t[:2000]]), np.concatenate([w, rng.uniform(0.05, 1.0, 2000)])
    rp, ci, va = _csr_of_edges(n, s, t, w)
    A = _from_arrays(rp, ci, va, n)
    _check_sssp(A, (rp, ci, va), [1, 2, 2, 2999])
    _check_bfs(A, (rp, ci, va), [1, 2, 2, 2999])


def test_negative_weights():
    rng = np.random.default_rng(31)
    n, m = 2000, 16000
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    s, t = np.minimum(a, b)[keep], np.maximum(a, b)[keep]                                 # a DAG: edges only i → j with j > i
    w = rng.uniform(-1.0, 1.0, s.size)
    rp, ci, va = _csr_of_edges(n, s, t, w)
    A = _from_arrays(rp, ci, va, n)
    d_ref, _ = _check_sssp(A, (rp, ci, va), [0, 3])
    assert (d_ref < 0).any()
    # a negative 3-cycle reachable from the source: no fixed point
    n = 40
    edges = [(i, i + 1, 0.5) for i in range(n - 1)] + [(12, 10, -1.5)]                    # 10 → 11 → 12 → 10 sums to −0.5
    rp, ci, va = _csr_of_edges(n, [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges])
    A = _from_arrays(rp, ci, va, n)
    for direction in DIRECTIONS:
        d, info = A.sssp([0], direction=direction)
        assert info["converged"] == 0 and info["iterations"] == n, (direction, info)


def test_bfs_rmat_and_direction_switch(rmat, monkeypatch):
    from scipy.sparse.csgraph import shortest_path
    import scipy.sparse as sp
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n)
    l_ref, _ = _check_bfs(A, (rp, ci, va), [src])
    hops = shortest_path(sp.csr_matrix((va, ci, rp), shape=(n, n)), directed=True, unweighted=True, indices=src)
    assert np.array_equal(l_ref, np.where(np.isfinite(hops), hops, -1).astype(np.int32))
    # the A/B switch: push only while the frontier has at most nnz / 64 out-edges, so that the middle steps pull and the ends push (the source is
    # moved to a vertex of small out-degree so that the first step is a push too)
    small = int(np.flatnonzero((np.diff(rp) > 0) & (np.diff(rp) < 4) & (l_ref > 0))[0])
    monkeypatch.setenv("G4S_TRAVERSE_ALPHA", "64")
    _, infos = _check_bfs(A, (rp, ci, va), [small], directions=("auto",))
    assert infos["auto"]["push_steps"] > 0 and infos["auto"]["pull_steps"] > 0, infos
    _, infos = _check_sssp(A, (rp, ci, va), [small], directions=("auto",))
    assert infos["auto"]["push_steps"] > 0 and infos["auto"]["pull_steps"] > 0, infos


def test_symmetric_needs_no_transpose(rmat):
    capi, _ = _host()
    import scipy.sparse as sp
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    G = sp.csr_matrix((va, ci, rp), shape=(n, n))
    S = G.maximum(G.T).tocsr()
    S.sort_indices()
    arrays = (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))
    A = _from_arrays(*arrays, n)
    A.traverse_reserve(symmetric=True)
    _check_sssp(A, arrays, [src], symmetric=True)
    _check_bfs(A, arrays, [src], symmetric=True)
    inf = capi.CsrInfo()
    assert capi.load().g4s_csr_transpose_info(A.handle, C.byref(inf)) == capi.ERR_INVALID      # nothing was reserved


@pytest.mark.parametrize("updatable", [False, True])
def test_update_values_then_sssp(rmat, updatable):
    capi, _ = _host()
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n, spmv_flags=capi.SPMV_BLOCKED | (capi.SPMV_UPDATABLE if updatable else 0))
    A.sssp([src])
    A.bfs([src])
    vb = np.random.default_rng(77).uniform(0.05, 1.0, ci.size)
    vb[::5] = 0.0                                                    # now some entries are no BFS edges any more
    A.update_values(torch.from_numpy(vb).cuda())
    _check_sssp(A, (rp, ci, vb), [src], directions=("push", "pull", "auto"))
    _check_bfs(A, (rp, ci, vb), [src], directions=("push", "pull"))


def test_repeatable_no_growth_and_refusals(rmat):
    capi, host = _host()
    lib = capi.load()
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n)
    A.traverse_reserve()
    first = {}
    for direction in DIRECTIONS:
        first[direction] = (A.sssp([src], direction=direction)[0].clone(), A.bfs([src], direction=direction)[0].clone())
    bytes0 = A.info()["plan_bytes"], A.transpose_info()["plan_bytes"]
    assert bytes0[0] >= 20 * n
    for _ in range(9):
        for direction in DIRECTIONS:
            d, _ = A.sssp([src], direction=direction)
            lv, _ = A.bfs([src], direction=direction)
            assert torch.equal(d, first[direction][0]) and torch.equal(lv, first[direction][1])
    assert (A.info()["plan_bytes"], A.transpose_info()["plan_bytes"]) == bytes0
    # refusals that need the handle: a source out of range, a non-square handle — nothing is enqueued
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    for bad in ([n], [-1], [0, n + 5]):
        s = np.asarray(bad, np.int32)
        assert lib.g4s_sssp(A.handle, C.c_void_p(s.ctypes.data), s.size, C.c_void_p(out.data_ptr()), 0, 0, None, None) == capi.ERR_INVALID
        assert lib.g4s_bfs(A.handle, C.c_void_p(s.ctypes.data), s.size, C.c_void_p(out.data_ptr()), 0, 0, None, None) == capi.ERR_INVALID
    R = host.CSR.from_host(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 1.0]), 2, 3)
    s = np.zeros(1, np.int32)
    assert lib.g4s_sssp(R.handle, C.c_void_p(s.ctypes.data), 1, C.c_void_p(out.data_ptr()), 0, 0, None, None) == capi.ERR_INVALID
    assert lib.g4s_csr_traverse_reserve(R.handle, 0) == capi.ERR_INVALID
    # a capturing stream is refused and the capture stays valid
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        s = np.asarray([src], np.int32)
        st = lib.g4s_sssp(A.handle, C.c_void_p(s.ctypes.data), 1, C.c_void_p(out.data_ptr()), 0, 0, None, C.c_void_p(stream.cuda_stream))
        st2 = lib.g4s_bfs(A.handle, C.c_void_p(s.ctypes.data), 1, C.c_void_p(out.data_ptr()), 0, 0, None, C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and st2 == capi.ERR_INVALID
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))


def test_equals_the_integration_host_loops(rmat):
    (rp, ci, va), src = rmat
    n = len(rp) - 1
    A = _from_arrays(rp, ci, va, n)
    d = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
    d[src] = 0.0
    while True:                                                      # Bellman-Ford on a graph stored by out-edges
        prev = d.clone()
        A.spmv_semiring_transpose(prev, d, semiring="min_plus", accumulate=True)
        if torch.equal(d, prev):
            break
    frontier = torch.zeros(n, dtype=torch.float64, device="cuda")
    frontier[src] = 1.0
    visited, level, depth = frontier.clone(), torch.full_like(frontier, float("inf")), 0
    level[src] = 0.0
    while bool(frontier.any()):                                      # BFS levels, or-and
        depth += 1
        frontier = A.spmv_semiring_transpose(frontier, semiring="or_and") * (1.0 - visited)
        level[frontier != 0] = depth
        visited = torch.maximum(visited, frontier)
    for direction in DIRECTIONS:
        got, _ = A.sssp([src], direction=direction)
        assert torch.equal(got, d), direction
        lv, _ = A.bfs([src], direction=direction)
        assert torch.equal(torch.where(lv >= 0, lv.double(), torch.full_like(level, float("inf"))), level), direction
