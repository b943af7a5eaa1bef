"""A refused call leaves nothing behind in the calling thread's read-back ledger (g4s_amd/csrc/readback.hpp): for every entry point that reads a
verdict back, one call the library refuses, then — same thread, same stream — a valid call on a 64-row matrix and a 300-row SpGEMM that takes the
rank path, both equal to their oracles bit for bit. A note left behind by the refused call would be handed out by the next wait on the stream:
into a dead frame, with the pinned block never starting over.

Every refused input is one the existing tests already show is refused cleanly; nothing here provokes a fault. ewise, masked SpGEMM, triangle count,
PageRank and components find the violation on the device (the verdict comes back through the ledger); the traversals and betweenness have no
device-side refusal that fits in 64 rows (betweenness' only one, σ past the range of a double, takes 3 301), so theirs is the out-of-range source
of test_traverse_gpu / test_betweenness_gpu, refused on the host.

The host-pointer cases at the end go through the staging frame of the two-call builders (g4s_amd/csrc/call_util.hpp): the refused call hands its device
copies back to the block cache, a valid call of the same sizes takes the same blocks out again, and a device-pointer call follows. One of their matrices
has a row of 65 entries (two work units) and an empty row. Only the first of them ends with the 300-row product.

Bit for bit: all values are small integers or dyadic fractions, so every sum is exact in float64 whatever its order — the float64 results and the
longdouble references are the same numbers. PageRank: unit weights, out-degrees 0, 1, 2 and 4, damping 0.5, n = 64 = 2⁶; an iteration divides by at
most 4, by 64 (dangling mass · p) and by 2: 9 more fraction bits, 6 + 4 · 9 = 42 < 53 after four iterations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import betweenness_ref, components_ref, coo_ref, ewise_ref, extract_ref, masked_ref, pagerank_ref, semiring_ref, traverse_ref
from tests import test_coo_gpu as coo_calls, test_ewise_gpu as ewise_calls, test_extract_gpu as extract_calls   # their ctypes wrappers of both pointer forms

pytestmark = pytest.mark.gpu

N = 64


def _host():
    from g4s_amd import capi, host
    return capi, host


def _ints(rng, count):
    v = rng.integers(1, 5, count) * rng.choice([-1, 1], count)
    return v.astype(np.float64)


def _square(seed, per_row=8, n=N):
    """n × n, per_row strictly ascending columns in every row, integer values in ±1 … ±4"""
    rng = np.random.default_rng(seed)
    ci = np.concatenate([np.sort(rng.choice(n, per_row, replace=False)) for _ in range(n)]).astype(np.int32)
    return np.arange(n + 1, dtype=np.int32) * per_row, ci, _ints(rng, ci.size)


def _unsorted(A, row=N - 1):
    """the same matrix with the first two of the row's 8 columns exchanged"""
    ci = A[1].copy()
    k = int(A[0][row])
    ci[k], ci[k + 1] = ci[k + 1], ci[k]
    return A[0], ci, A[2]


def _refused(capi, call):
    with pytest.raises(capi.G4SError) as e:
        call()
    assert e.value.status == capi.ERR_INVALID, str(e.value)


# ------------------------------------------------------------------------------------------------ the 300-row product on the rank path
@pytest.fixture(scope="module")
def rank_product():
    """A (300 × 300) · B (300 × 65 536) after the warm-up matrix (g4s_warm_up): B's rows 64 … 191 hold 128 scattered entries, A's rows 192 … 255 point
    forty times at them — 5 120 products a row, the rank path from 4 096 — and A's rows 256 … 299 twelve times (the mid-size classes in between the
    rank launch's two stages). Integer values. The oracle is computed once."""
    rng = np.random.default_rng(300)
    M, K, NB = 300, 300, 1 << 16
    arows, brows = [], []
    for r in range(M):
        if 192 <= r < 256:
            arows.append(64 + np.sort(rng.choice(128, 40, replace=False)))
        elif r >= 256:
            arows.append(64 + np.sort(rng.choice(128, 12, replace=False)))
        else:
            arows.append(np.sort(rng.choice(K, 6, replace=False)))
    for r in range(K):
        brows.append(np.sort(rng.choice(NB, 128 if 64 <= r < 192 else 6, replace=False)))
    csr = lambda rows: (np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32), np.concatenate(rows).astype(np.int32))
    A, B = csr(arows), csr(brows)
    A, B = (A[0], A[1], _ints(rng, A[1].size)), (B[0], B[1], _ints(rng, B[1].size))
    want = semiring_ref.spgemm(A, B, M, "plus_times")
    assert int(np.diff(want[0])[192:256].min()) > 4096                # the rank rows are past the mid-size limit in outputs too
    return (A, B, M, K, NB), want


def _then_the_rank_product(rank_product, monkeypatch, capfd):
    _, host = _host()
    (A, B, M, K, NB), want = rank_product
    a, b = host.CSR.from_host(*A, M, K), host.CSR.from_host(*B, K, NB)
    monkeypatch.setenv("G4S_DEBUG", "1")                              # the library's own account of its row classes, on stderr
    capfd.readouterr()
    c = host.HashSpGEMM(a, b, sortOutput=True)
    err = capfd.readouterr().err
    monkeypatch.delenv("G4S_DEBUG")
    ranked = re.search(r"g4s numeric classes:.* rank (\d+)", err)
    assert ranked and int(ranked.group(1)) == 64, err                 # rows 192 … 255 took the rank path
    crp, cci, cva = c.to_host()
    assert np.array_equal(crp, want[0]) and np.array_equal(cci, want[1])
    assert np.array_equal(cva.view(np.int64), want[2].view(np.int64))


# ------------------------------------------------------------------------------------------------ the entry points
def test_ewise_symbolic(rank_product, monkeypatch, capfd):
    capi, host = _host()
    A, B = _square(1), _square(2)
    a, b = host.CSR.from_host(*A, N, N), host.CSR.from_host(*B, N, N)
    _refused(capi, lambda: host.csr_ewise(host.CSR.from_host(*_unsorted(A), N, N), b))
    _refused(capi, lambda: host.csr_ewise(a, host.CSR.from_host(*_unsorted(B, row=0), N, N)))
    got = host.csr_ewise(a, b, "union", "plus").to_host()
    want = ewise_ref.ewise(A, B, N, N, "union", "plus")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.int64), np.asarray(want[2], np.float64).view(np.int64))
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_masked_spgemm(rank_product, monkeypatch, capfd):
    capi, host = _host()
    A = _square(3)
    a = host.CSR.from_host(*A, N, N)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    bad = _unsorted(A)
    _refused(capi, lambda: host.spgemm_masked(a, a, (t(bad[0]), t(bad[1]))))
    got = host.spgemm_masked(a, a, a).values.cpu().numpy()
    want, hit = masked_ref.spgemm_masked(A, A, N, N, (A[0], A[1]), "plus_times")
    assert hit.any() and np.array_equal(got.view(np.int64), want.view(np.int64))
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_triangle_count(rank_product, monkeypatch, capfd):
    capi, host = _host()
    A = _square(4)
    G = masked_ref.symmetric_simple_graph(A[0], A[1], N)
    g = (G.indptr.astype(np.int32), G.indices.astype(np.int32), np.ones(G.nnz))
    row = int(np.flatnonzero(np.diff(g[0]) >= 8)[-1])
    _refused(capi, lambda: host.CSR.from_host(*_unsorted(g, row=row), N, N).triangle_count())
    want = masked_ref.triangles_lower(G)
    assert want > 0 and host.CSR.from_host(*g, N, N).triangle_count() == want
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def _edges_with_out_degrees(seed):
    """64 vertices with out-degrees 0, 1, 2 and 4 (sixteen of each), unit weights: (rowptr, colids, values)"""
    rng = np.random.default_rng(seed)
    deg = rng.permutation(np.repeat([0, 1, 2, 4], N // 4))
    src = np.repeat(np.arange(N), deg)
    dst = np.concatenate([np.sort(rng.choice(N, d, replace=False)) for d in deg])
    return pagerank_ref.csr_of_edges(N, src, dst, np.ones(src.size))


def test_traverse(rank_product, monkeypatch, capfd):
    capi, host = _host()
    rp, ci, _ = _edges_with_out_degrees(5)
    va = np.random.default_rng(6).integers(1, 9, ci.size) / 8.0      # eighths: every path length is exact
    A = host.CSR.from_host(rp, ci, va, N, N)
    lib = capi.load()
    out = torch.empty(N, dtype=torch.float64, device="cuda")
    s = np.array([N], np.int32)
    assert lib.g4s_sssp(A.handle, C.c_void_p(s.ctypes.data), 1, C.c_void_p(out.data_ptr()), 0, 0, None, None) == capi.ERR_INVALID
    src = [int(np.argmax(np.diff(rp)))]
    d_ref, _, converged, _ = traverse_ref.sssp(rp, ci, va, N, src)
    l_ref, _ = traverse_ref.bfs(rp, ci, va, N, src)
    assert converged and np.isfinite(d_ref).sum() > 8
    d, _ = A.sssp(src)
    lv, _ = A.bfs(src)
    assert np.array_equal(d.cpu().numpy().view(np.int64), d_ref.view(np.int64))
    assert np.array_equal(lv.cpu().numpy(), l_ref)
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_pagerank(rank_product, monkeypatch, capfd):
    capi, host = _host()
    rp, ci, va = _edges_with_out_degrees(7)
    bad = va.copy()
    bad[11] = -0.5
    _refused(capi, lambda: host.CSR.from_host(rp, ci, bad, N, N).pagerank())
    ref = pagerank_ref.pagerank(rp, ci, va, N, damping=0.5, tol=0.0, max_iterations=4)
    want = ref.rank.astype(np.float64)
    assert ref.dangling == N // 4 and np.array_equal(want.astype(np.longdouble), ref.rank)   # the reference's ranks ARE float64 numbers
    r, info = host.CSR.from_host(rp, ci, va, N, N).pagerank(damping=0.5, tol=0.0, max_iterations=4)
    assert info["iterations"] == 4 and info["dangling"] == ref.dangling
    assert np.array_equal(r.cpu().numpy().view(np.int64), want.view(np.int64))
    assert info["residual"] == float(ref.residuals[-1])
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_betweenness(rank_product, monkeypatch, capfd):
    capi, host = _host()
    arrays = betweenness_ref.diamonds(21)                             # 64 vertices, σ up to 2²¹, every δ a dyadic fraction
    assert len(arrays[0]) - 1 == N
    A = host.CSR.from_host(*arrays, N, N)
    lib = capi.load()
    out = torch.zeros(N, dtype=torch.float64, device="cuda")
    s = np.array([0, N], np.int32)
    assert lib.g4s_betweenness(A.handle, C.c_void_p(s.ctypes.data), 2, 1.0, C.c_void_p(out.data_ptr()), 0, None, None) == capi.ERR_INVALID
    ref = betweenness_ref.betweenness(*arrays, N, [0, 3])
    want = ref.bc.astype(np.float64)
    assert np.array_equal(want.astype(np.longdouble), ref.bc) and want.max() > 0
    bc, _ = A.betweenness([0, 3])
    assert np.array_equal(bc.cpu().numpy().view(np.int64), want.view(np.int64))
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_components(rank_product, monkeypatch, capfd):
    capi, host = _host()
    rng = np.random.default_rng(8)
    rp = np.arange(N + 1, dtype=np.int32)                             # one edge a vertex, inside its block of 16: at least four components
    ci = ((np.arange(N) // 16) * 16 + rng.integers(0, 16, N)).astype(np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    bad = ci.copy()
    bad[N - 1] = N
    _refused(capi, lambda: host.connected_components((t(rp), t(bad))))
    want, _ = components_ref.labels(rp, ci, N)
    got = host.connected_components((t(rp), t(ci)))
    assert len(np.unique(want)) >= 4 and np.array_equal(got.cpu().numpy(), want)
    _then_the_rank_product(rank_product, monkeypatch, capfd)


# ------------------------------------------------------------------------------------------------ host pointers: the staging frame after a refusal
COLS = 128


def _ragged(seed):
    """64 × 128 with integer values: eight ascending columns a row, but 65 in row 5 (two work units) and none in row 6"""
    rng = np.random.default_rng(seed)
    lengths = np.full(N, 8)
    lengths[5], lengths[6] = 65, 0
    ci = np.concatenate([np.sort(rng.choice(COLS, n, replace=False)) for n in lengths]).astype(np.int32)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), ci, _ints(rng, ci.size)


def _rowptr_from_one(A):
    rp = A[0].copy()
    rp[0] = 1
    return rp, A[1], A[2]


def test_ewise_host_pointers(rank_product, monkeypatch, capfd):
    capi, _ = _host()
    A, B = _square(11), _square(12)
    want = ewise_ref.ewise(A, B, N, N, "union", "plus")
    assert ewise_calls._ewise(_unsorted(A), B, N, N, "union", device=False)[0] == capi.ERR_INVALID        # found by the symbolic call on the device
    assert ewise_calls._ewise(_rowptr_from_one(A), B, N, N, "union", device=False)[0] == capi.ERR_INVALID
    for device in (False, True):
        st, got, _ = ewise_calls._ewise(A, B, N, N, "union", "plus", device=device)
        assert st == 0
        ewise_calls._same(got, want, device)
    _then_the_rank_product(rank_product, monkeypatch, capfd)


def test_select_host_pointers():
    capi, _ = _host()
    A = _ragged(13)
    want = ewise_ref.select(A, N, "triu", 3)
    assert 0 < len(want[1]) < len(A[1]) and want[0][6] == want[0][7]
    _refused(capi, lambda: ewise_calls._select(_rowptr_from_one(A), N, COLS, "triu", 3, device=False))
    for device in (False, True):
        ewise_calls._same(ewise_calls._select(A, N, COLS, "triu", 3, device=device), want, device)


def test_from_coo_host_pointers():
    capi, _ = _host()
    rp, col, val = _ragged(14)
    rng = np.random.default_rng(15)
    order = rng.permutation(col.size + 40)                            # forty triples twice, in no order: the sort and the fold both run
    row = np.concatenate([ewise_ref.row_of_entry(rp), ewise_ref.row_of_entry(rp)[:40]]).astype(np.int32)[order]
    col, val = np.concatenate([col, col[:40]])[order], np.concatenate([val, val[:40]])[order]
    want = coo_ref.from_coo(row, col, val, N, COLS, "plus")
    assert len(want[1]) == rp[N] and np.diff(want[0])[5] == 65 and np.diff(want[0])[6] == 0
    bad = row.copy()
    bad[17] = N
    assert coo_calls._symbolic(bad, col, N, COLS, "plus", device=False)[0] == capi.ERR_INVALID
    for device in (False, True):
        coo_calls._check(row, col, val, N, COLS, "plus", want, device=device)


def test_extract_host_pointers():
    capi, _ = _host()
    A = _ragged(16)
    rng = np.random.default_rng(17)
    I, J = rng.permutation(N)[:48], rng.integers(0, COLS, 96)         # rows 5 and 6 among them, columns in no order with repeats
    I[:2] = 5, 6
    want = extract_ref.extract(A[0], A[1], A[2], N, COLS, I, J)
    assert len(want[1]) > 0
    bad = I.copy()
    bad[9] = N
    out = extract_calls._raw(A, N, COLS, bad, J, device=False)
    assert out[0] == capi.ERR_INVALID and out[1] is None
    for device in (False, True):
        extract_calls._exact(extract_calls._raw(A, N, COLS, I, J, device=device), want)
