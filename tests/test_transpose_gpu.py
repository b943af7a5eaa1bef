"""Device transpose and transposed products (include/g4s.h: g4s_csr_transpose, g4s_csr_transpose_reserve / _info, g4s_spmv_transpose,
g4s_spmv_semiring_transpose).

g4s_csr_transpose must equal the numpy stable-argsort transpose exactly: perm = argsort(colids, kind="stable"), tcolids = row_of_entry[perm],
tvalues = values[perm], trowptr = the scan of the column counts. A transposed product must equal the forward product of a handle created from that
transpose with the same flags: bit for bit on every path for the semirings and on paths 0, 3 and 4 for plus-times; within 1e-10·Σ|a·x| on the blocked
path (1), whose LDS atomic sums are not reproducible."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import spmv_semiring_ref as ref
from tests.helpers import power_law_csr, random_csr

pytestmark = pytest.mark.gpu
STREAM, BLOCKED, DIAGONAL, BLOCKROW = 0, 1, 3, 4
NEW = ref.NEW


def np_transpose(rp, ci, va, rows, cols):
    """The oracle: (trowptr, tcolids, tvalues, perm) of the stable transpose."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    perm = np.argsort(ci, kind="stable")
    trp = np.zeros(cols + 1, np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=cols)) if cols else []
    return trp.astype(np.int32), row[perm].astype(np.int32), (None if va is None else np.asarray(va)[perm]), perm.astype(np.int32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_transpose(rp, ci, va, rows, cols, kinds=("host", "device")):
    """g4s_csr_transpose against the oracle, all four arrays exact, host and device pointers, with and without values and perm."""
    from g4s_amd import host
    want = np_transpose(rp, ci, va, rows, cols)
    for kind in kinds:
        for with_values in (True, False):
            for with_perm in (True, False):
                v = va if with_values else None
                args = (rp, ci, v) if kind == "host" else (_cuda(rp), _cuda(ci), None if v is None else _cuda(v))
                torch.cuda.synchronize()
                out = host.csr_transpose(*args, rows, cols, with_perm=with_perm)
                trp, tci, tva = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2]
                assert np.array_equal(trp, want[0]), (kind, with_values, with_perm)
                assert np.array_equal(tci, want[1]), (kind, with_values, with_perm)
                if with_values:
                    assert np.array_equal(tva.cpu().numpy().view(np.int64), want[2].view(np.int64)), (kind, with_perm)   # bit for bit
                else:
                    assert tva is None
                if with_perm:
                    assert np.array_equal(out[3].cpu().numpy(), want[3]), (kind, with_values)
    return want


# ------------------------------------------------------------------------------------------------ 1. g4s_csr_transpose
@pytest.mark.parametrize("shape", [(500, 500), (3000, 200), (200, 3000)])
def test_transpose_square_tall_wide(shape):
    rows, cols = shape
    rp, ci, va = random_csr(rows, cols, 0.02, rows + cols, empty_rows=(0, 7, rows - 1))
    _check_transpose(rp, ci, va, rows, cols)


def test_transpose_empty_rows_and_columns():
    rows, cols = 4000, 5000
    rp, ci, va = power_law_csr(rows, cols, 3, 300)
    ci = (ci // 3 * 3).astype(np.int32)                               # two columns in three are empty (repeated columns appear too)
    assert (np.diff(rp) == 0).any()
    _check_transpose(rp, ci, va, rows, cols)


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0), (4, 6)])
def test_transpose_zero_sizes(rows, cols):
    rp = np.zeros(rows + 1, np.int32)
    ci, va = np.zeros(0, np.int32), np.zeros(0)
    trp, tci, tva, perm = _check_transpose(rp, ci, va, rows, cols)
    assert len(trp) == cols + 1 and not trp.any()


def test_transpose_repeated_columns_and_unsorted_rows():
    rng = np.random.default_rng(5)
    rows, cols = 700, 90
    lens = rng.integers(0, 40, rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, cols, rp[-1]).astype(np.int32)               # unsorted rows, many repeats inside a row
    va = rng.uniform(-1, 1, rp[-1])
    va[::7] = -0.0
    want = _check_transpose(rp, ci, va, rows, cols)
    assert np.array_equal(want[2], va[want[3]])


def test_transpose_column_of_more_than_a_million_entries():
    rng = np.random.default_rng(6)
    rows, cols = 1_200_000, 50_000
    other = rng.integers(0, cols, rows).astype(np.int32)
    other[other == 7] = 8
    ci = np.stack([np.minimum(other, 7), np.maximum(other, 7)], 1).ravel().astype(np.int32)   # each row: column 7 and one other, sorted
    rp = (2 * np.arange(rows + 1)).astype(np.int32)
    va = rng.uniform(-1, 1, len(ci))
    trp, _, _, _ = _check_transpose(rp, ci, va, rows, cols)
    assert trp[8] - trp[7] == rows


def test_transpose_rmat_2_20():
    from g4s_amd import host
    n = 1 << 20
    R = host.rmat_csr(n, 20, 10 * n, 11)
    rp, ci, va = R.to_host()
    assert np.diff(rp).max() > 1000
    _check_transpose(rp, ci, va, n, n)


def test_transpose_full_rmat_once():
    """The bench's 10M R-MAT (98.7M entries), device pointers, against the oracle; then back: Aᵀᵀ = A (sorted, duplicate-free)."""
    from g4s_amd import host
    from bench import build_matrix
    A = build_matrix("rmat", host, False)
    trp, tci, tva, perm = host.csr_transpose(A.rowptr, A.colids, A.values, A.rows, A.cols, with_perm=True)
    rr, rc, rv = host.csr_transpose(trp, tci, tva, A.cols, A.rows)
    assert torch.equal(rr, A.rowptr) and torch.equal(rc, A.colids) and torch.equal(rv, A.values)
    rp, ci, va = A.to_host()
    want = np_transpose(rp, ci, None, A.rows, A.cols)
    assert np.array_equal(trp.cpu().numpy(), want[0])
    assert np.array_equal(perm.cpu().numpy(), want[3])
    assert np.array_equal(tci.cpu().numpy(), want[1])
    assert np.array_equal(tva.cpu().numpy(), va[want[3]])


def test_transpose_of_transpose_sorts_rows():
    rng = np.random.default_rng(7)
    rows, cols = 2000, 1500
    rp, ci, va = random_csr(rows, cols, 0.01, 7)                      # sorted and duplicate-free
    shuf_ci, shuf_va = ci.copy(), va.copy()
    for r in range(rows):                                            # the same rows, unsorted
        k0, k1 = rp[r], rp[r + 1]
        p = rng.permutation(k1 - k0)
        shuf_ci[k0:k1], shuf_va[k0:k1] = ci[k0:k1][p], va[k0:k1][p]
    from g4s_amd import host
    t = host.csr_transpose(rp, shuf_ci, shuf_va, rows, cols)
    back = host.csr_transpose(t[0], t[1], t[2], cols, rows)
    assert np.array_equal(back[0].cpu().numpy(), rp) and np.array_equal(back[1].cpu().numpy(), ci) and np.array_equal(back[2].cpu().numpy(), va)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_transpose_invalid_inputs(kind):
    from g4s_amd import capi
    lib = capi.load()
    rp = np.array([0, 2, 3, 5], np.int32)
    ci = np.array([0, 3, 1, 2, 0], np.int32)
    va = np.arange(5, dtype=np.float64)
    cases = [(rp, np.array([0, 4, 1, 2, 0], np.int32), 4),           # a column == cols
             (rp, np.array([0, -1, 1, 2, 0], np.int32), 4),          # a negative column
             (rp, ci, 0),                                             # cols == 0 with entries
             (np.array([0, 3, 2, 5], np.int32), ci, 4),               # rowptr decreases
             (np.array([1, 2, 3, 5], np.int32), ci, 4),               # rowptr[0] != 0
             (np.array([0, 2, 3, 4], np.int32), ci, 4)]               # rowptr[rows] != nnz
    for r, c, cols in cases:
        trp, tci, tva = np.zeros(cols + 1, np.int32), np.zeros(5, np.int32), np.zeros(5)
        if kind == "host":
            P = lambda a: a.ctypes.data_as(C.c_void_p)
            st = lib.g4s_csr_transpose(3, cols, 5, P(r), P(c), P(va), P(trp), P(tci), P(tva), None, capi.HOST_POINTERS, None)
        else:
            d = [_cuda(a) for a in (r, c, va, trp, tci, tva)]
            torch.cuda.synchronize()
            P = lambda t: C.c_void_p(t.data_ptr())
            st = lib.g4s_csr_transpose(3, cols, 5, *[P(t) for t in d], None, capi.DEVICE_POINTERS, None)
        assert st == capi.ERR_INVALID, (r, c, cols, lib.g4s_last_error())
    # and a valid call right after them still works
    _check_transpose(rp, ci, va, 3, 4, kinds=(kind,))


# ------------------------------------------------------------------------------------------------ 2. the Uzawa operators
def test_uzawa_divergence_transpose():
    from g4s_amd import host
    from tests.helpers import stokes_problem
    from tests.test_stokes_dist_gpu import div_grad_csr
    pr = stokes_problem(6, 5, 4, 3)
    (drp, dci, dva), (trp, tci, tva) = div_grad_csr(pr["ien"], pr["id"], pr["g"], pr["neq"])
    nel, neq = len(drp) - 1, pr["neq"]
    o = host.csr_transpose(drp, dci, dva, nel, neq)
    assert np.array_equal(o[0].cpu().numpy(), trp) and np.array_equal(o[1].cpu().numpy(), tci)
    assert np.array_equal(o[2].cpu().numpy(), tva)
    D = host.CSR.from_host(drp, dci, dva, nel, neq)
    Dt = host.CSR.from_host(trp, tci, tva, neq, nel)
    p = _cuda(np.random.default_rng(8).uniform(-1, 1, nel))
    a = D.spmv_transpose(p)
    b = Dt.spmv(p)
    assert D.transpose_info()["spmv_path"] == Dt.info()["spmv_path"]
    if Dt.info()["spmv_path"] == BLOCKED:
        assert float((a - b).abs().max()) <= 1e-10 * max(float(b.abs().max()), 1.0)
    else:
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the four paths
def _block_csr(nbr, nbc, b, per_row, seed):
    from tests.test_spmv_semiring_gpu import _block_csr as blocks
    return blocks(nbr, nbc, b, per_row, seed)


@functools.lru_cache(maxsize=None)
def _power_law():
    return power_law_csr(60000, 50000, 21, 3000)


def _path_cases():
    """(name, forward handle, expected path of Aᵀ, host arrays): the forward flags carry over to Aᵀ."""
    from g4s_amd import capi, host
    rp, ci, va = _power_law()
    yield "stream", host.CSR.from_host(rp, ci, va, 60000, 50000, spmv_flags=capi.SPMV_STREAM), STREAM, (rp, ci, va)
    yield "blocked", host.CSR.from_host(rp, ci, va, 60000, 50000, spmv_flags=capi.SPMV_BLOCKED), BLOCKED, (rp, ci, va)
    L = host.laplacian_csr(7, 23, 21, 19)
    yield "diagonal", L, DIAGONAL, L.to_host()
    B = host.banded_csr(5001, 3, 12)
    yield "banded", B, DIAGONAL, B.to_host()
    brp, bci, bva = _block_csr(600, 700, 3, 4, 22)
    yield "blockrow", host.CSR.from_host(brp, bci, bva, 1800, 2100), BLOCKROW, (brp, bci, bva)


def _forward_of_transpose(A):
    """the handle of §1's output with A's flags (device pointers, as the inner handle)"""
    from g4s_amd import host
    trp, tci, tva = host.csr_transpose(A.rowptr, A.colids, A.values, A.rows, A.cols)
    return host.CSR(trp, tci, tva, A.cols, A.rows, spmv_flags=A._spmv_flags)


def _same(a, b, path, absx=None):
    if path == BLOCKED:
        assert float((a - b).abs().max()) <= 1e-10 * max(float(absx), 1.0)
    else:
        assert torch.equal(a, b)


def test_plus_times_transpose_on_every_path():
    rng = np.random.default_rng(30)
    for name, A, path, (rp, ci, va) in _path_cases():
        info_before = A.info()
        A.transpose_reserve()
        assert A.info() == info_before                               # g4s_csr_get_info(A) does not change
        ti = A.transpose_info()
        assert ti["spmv_path"] == path and ti["rows"] == A.cols and ti["cols"] == A.rows and ti["nnz"] == A.nnz, (name, ti)
        T = _forward_of_transpose(A)
        assert T.info()["spmv_path"] == path
        assert ti["plan_bytes"] >= T.info()["plan_bytes"] + 4 * (A.cols + 1) + 20 * A.nnz
        xh = rng.uniform(-1, 1, A.rows)
        x = _cuda(xh)
        absx = np.abs(va) @ np.abs(xh)[np.repeat(np.arange(A.rows), np.diff(rp))] if path == BLOCKED else None
        for alpha, beta in ((1.0, 0.0), (-0.5, 0.0), (2.0, 0.5), (1.0, 1.0), (0.0, 1.5)):
            y0 = _cuda(rng.uniform(-1, 1, A.cols))
            if beta == 0.0:
                y0.fill_(float("nan"))                               # never read when beta == 0
            a = A.spmv_transpose(x, y0.clone(), alpha, beta)
            b = T.spmv(x, y0.clone(), alpha, beta)
            assert not torch.isnan(a).any(), (name, alpha, beta)
            _same(a, b, path, absx)
        a = A.spmv_transpose(x)                                      # y allocated
        assert a.numel() == A.cols
        if path != BLOCKED:
            assert torch.equal(A.spmv_transpose(x), a)               # reproducible


def test_semiring_transpose_on_every_path_exact():
    rng = np.random.default_rng(31)
    for name, A, path, (rp, ci, va) in _path_cases():
        trp, tci, tva, _ = np_transpose(rp, ci, va, A.rows, A.cols)
        for semiring in NEW:
            x = rng.uniform(-1, 1, A.rows)
            if semiring == "or_and":
                x[rng.random(A.rows) < 0.5] = 0.0
            y0 = rng.uniform(-2, 2, A.cols) if semiring != "or_and" else np.where(rng.random(A.cols) < 0.7, 0.0, 5.0)
            for accumulate in (False, True):
                yd = _cuda(y0.copy()) if accumulate else torch.full((A.cols,), float("nan"), dtype=torch.float64, device="cuda")
                out = A.spmv_semiring_transpose(_cuda(x), yd, semiring=semiring, accumulate=accumulate).cpu().numpy()
                want = ref.spmv(trp, tci, tva, x, semiring, y0 if accumulate else None)
                assert ref.same_values(out, want), (name, semiring, accumulate)
        assert A.transpose_info()["spmv_path"] == path


def test_first_product_reserves_and_null_vectors_are_invalid():
    from g4s_amd import capi, host
    lib = capi.load()
    rp, ci, va = random_csr(300, 200, 0.05, 32)
    A = host.CSR.from_host(rp, ci, va, 300, 200)
    with pytest.raises(RuntimeError):
        A.transpose_info()                                           # INVALID before a reserve
    x, y = _cuda(np.ones(300)), torch.zeros(200, dtype=torch.float64, device="cuda")
    assert lib.g4s_spmv_transpose(A.handle, None, C.c_void_p(y.data_ptr()), 1.0, 0.0, None) == capi.ERR_INVALID
    assert lib.g4s_spmv_transpose(A.handle, C.c_void_p(x.data_ptr()), None, 1.0, 0.0, None) == capi.ERR_INVALID
    assert lib.g4s_spmv_semiring_transpose(A.handle, C.c_void_p(x.data_ptr()), None, capi.SEMIRING_MIN_PLUS, None) == capi.ERR_INVALID
    for bad in (4096, 1 << 20, 1 << 31, capi.DEVICE_POINTERS):
        assert lib.g4s_spmv_semiring_transpose(A.handle, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), capi.SEMIRING_MIN_PLUS | bad, None) == capi.ERR_INVALID
    y = A.spmv_transpose(x)                                          # the first call reserves
    assert A.transpose_info()["rows"] == 200
    want = np.zeros(200)
    np.add.at(want, ci, va)                                          # Aᵀ·1 = column sums (short columns: summed in entry order)
    assert np.allclose(y.cpu().numpy(), want, rtol=0, atol=1e-12)


def test_module_level_functions_and_csr_transpose_method():
    from g4s_amd import capi, host
    rp, ci, va = power_law_csr(5000, 3000, 33, 200)
    A = host.CSR.from_host(rp, ci, va, 5000, 3000, spmv_flags=capi.SPMV_STREAM)
    T = A.transpose()
    assert (T.rows, T.cols, T.nnz) == (3000, 5000, A.nnz) and T._spmv_flags == capi.SPMV_STREAM
    want = np_transpose(rp, ci, va, 5000, 3000)
    assert all(np.array_equal(a, b) for a, b in zip(T.to_host(), want[:3]))
    x = _cuda(np.random.default_rng(33).uniform(0, 1, 5000))
    assert torch.equal(host.spmv_transpose(A, x), T.spmv(x))
    assert torch.equal(host.spmv_semiring_transpose(A, x, semiring="max_plus"), T.spmv_semiring(x, semiring="max_plus"))
    with pytest.raises(ValueError):
        host.spmv_semiring_transpose(A, x, semiring="plus-times")


# ------------------------------------------------------------------------------------------------ 5. graph algorithms on the forward handle
def _rmat_graph(n=1 << 16, seed=9):
    from g4s_amd import capi, host
    import scipy.sparse as sp
    R = host.rmat_csr(n, 16, 10 * n, seed)
    rp, ci, _ = R.to_host()
    w = np.random.default_rng(seed).integers(1, 11, len(ci)).astype(np.float64)    # integer weights: exact sums
    G = sp.csr_matrix((w, ci, rp), shape=(n, n))
    A = host.CSR.from_host(rp, ci, w, n, n, spmv_flags=capi.SPMV_BLOCKED)          # stored by out-edges; no host transpose
    return G, A


def test_bellman_ford_on_out_edges_equals_scipy():
    from scipy.sparse.csgraph import shortest_path
    G, A = _rmat_graph()
    n = G.shape[0]
    src = int(np.argmax(np.diff(G.indptr)))
    d = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
    d[src] = 0.0
    for it in range(n):
        prev = d.clone()
        A.spmv_semiring_transpose(prev, d, semiring="min_plus", accumulate=True)   # d := d ⊕ (Aᵀ ⊗ d_prev)
        if torch.equal(d, prev):
            break
    assert A.transpose_info()["spmv_path"] == BLOCKED
    want = shortest_path(G, method="D", directed=True, indices=src)
    assert it > 2
    assert ref.same_values(d.cpu().numpy(), want)


def test_bfs_levels_on_out_edges_equal_scipy():
    from scipy.sparse.csgraph import shortest_path
    G, A = _rmat_graph(seed=10)
    n = G.shape[0]
    src = int(np.argmax(np.diff(G.indptr)))
    level = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
    frontier = torch.zeros(n, dtype=torch.float64, device="cuda")
    frontier[src] = 1.0
    visited = frontier.clone()
    level[src] = 0.0
    depth = 0
    while bool(frontier.any()):
        depth += 1
        reach = A.spmv_semiring_transpose(frontier, semiring="or_and")             # vertices with an edge from the frontier
        frontier = reach * (1.0 - visited)
        level[frontier != 0] = float(depth)
        visited = torch.maximum(visited, frontier)
    want = shortest_path(G, directed=True, unweighted=True, indices=src)
    assert depth > 2
    assert ref.same_values(level.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 6. new values after a reserve
class _Owned:
    """A handle created from host arrays (the handle owns device copies), driven through the C-ABI."""

    def __init__(self, rp, ci, va, rows, cols, flags):
        from g4s_amd import capi
        self.lib, self.capi = capi.load(), capi
        self.rows, self.cols = rows, cols
        self.h = C.c_void_p()
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.g4s_csr_create(C.byref(self.h), rows, cols, len(ci), P(rp), P(ci), P(va), capi.HOST_POINTERS | flags))

    def update_values(self, v):
        self.capi.check(self.lib.g4s_csr_update_values(self.h, C.c_void_p(v.data_ptr()), self.capi.DEVICE_POINTERS, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def transpose_reserve(self):
        self.capi.check(self.lib.g4s_csr_transpose_reserve(self.h))

    def spmv_transpose(self, x):
        y = torch.empty(self.cols, dtype=torch.float64, device="cuda")
        self.capi.check(self.lib.g4s_spmv_transpose(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), 1.0, 0.0,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return y

    def spmv_semiring_transpose(self, x, semiring):
        from g4s_amd import host
        y = torch.empty(self.cols, dtype=torch.float64, device="cuda")
        self.capi.check(self.lib.g4s_spmv_semiring_transpose(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), host.SEMIRINGS[semiring],
                                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return y

    def close(self):
        self.lib.g4s_csr_destroy(self.h)


@pytest.mark.parametrize("owned", [False, True])
@pytest.mark.parametrize("updatable", [False, True])
def test_update_values_refreshes_the_transpose(owned, updatable):
    from g4s_amd import capi, host
    rng = np.random.default_rng(40 + 2 * owned + updatable)
    upd = capi.SPMV_UPDATABLE if updatable else 0
    for name, A0, path, (rp, ci, va) in _path_cases():
        flags = A0._spmv_flags | upd
        A = _Owned(rp, ci, va, A0.rows, A0.cols, flags) if owned else host.CSR.from_host(rp, ci, va, A0.rows, A0.cols, spmv_flags=flags)
        A.transpose_reserve()
        x = _cuda(rng.uniform(-1, 1, A0.rows))
        A.spmv_transpose(x)
        for step in range(2):
            vnew = rng.uniform(-3, 3, len(ci))
            A.update_values(_cuda(vnew))
            fresh = host.CSR.from_host(rp, ci, vnew, A0.rows, A0.cols, spmv_flags=flags)
            F = _forward_of_transpose(fresh)
            absx = np.abs(vnew) @ np.abs(x.cpu().numpy())[np.repeat(np.arange(A0.rows), np.diff(rp))]
            _same(A.spmv_transpose(x), F.spmv(x), path, absx)
            for semiring in NEW:
                assert torch.equal(A.spmv_semiring_transpose(x, semiring=semiring), F.spmv_semiring(x, semiring=semiring)), (name, semiring, owned, updatable)
            F.close()
            fresh.close()
        A.close()


# ------------------------------------------------------------------------------------------------ 7. capture
@pytest.mark.parametrize("path", ["stream", "blocked", "diagonal"])
def test_captured_transpose_replays_the_eager_call(path):
    from g4s_amd import capi, host
    if path == "diagonal":
        A = host.laplacian_csr(7, 30, 30, 30)
    else:
        rp, ci, va = power_law_csr(50000, 40000, 50, 2000)
        A = host.CSR.from_host(rp, ci, va, 50000, 40000, spmv_flags=capi.SPMV_STREAM if path == "stream" else capi.SPMV_BLOCKED)
    A.transpose_reserve()
    rng = np.random.default_rng(51)
    x = _cuda(rng.uniform(-1, 1, A.rows))
    y0 = _cuda(rng.uniform(-1, 1, A.cols))
    d0 = _cuda(rng.uniform(0, 1, A.cols))

    def seq(y, d):
        A.spmv_transpose(x, y, 0.5, 2.0)
        A.spmv_semiring_transpose(x, d, semiring="min_plus", accumulate=True)

    y_e, d_e = y0.clone(), d0.clone()
    seq(y_e, d_e)
    torch.cuda.synchronize()
    y_g, d_g = y0.clone(), d0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            seq(y_g, d_g)
    torch.cuda.current_stream().wait_stream(side)
    y_g.copy_(y0)
    d_g.copy_(d0)
    g.replay()
    torch.cuda.synchronize()
    if path == "blocked":
        assert float((y_g - y_e).abs().max()) <= 1e-10 * max(float(y_e.abs().max()), 1.0)
    else:
        assert torch.equal(y_g, y_e)
    assert torch.equal(d_g, d_e)


def test_unreserved_call_on_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    rp, ci, va = random_csr(2000, 1500, 0.01, 52)
    A = host.CSR.from_host(rp, ci, va, 2000, 1500)
    h = A.handle
    x = _cuda(np.ones(2000))
    y = torch.full((1500,), 3.0, dtype=torch.float64, device="cuda")
    z = torch.zeros(4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    codes = []
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s = C.c_void_p(side.cuda_stream)
            codes.append(lib.g4s_spmv_transpose(h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), 1.0, 0.0, s))
            codes.append(lib.g4s_spmv_semiring_transpose(h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), capi.SEMIRING_MIN_PLUS, s))
            z.add_(1.0)                                              # the capture itself goes on
    torch.cuda.current_stream().wait_stream(side)
    assert codes == [capi.ERR_INVALID, capi.ERR_INVALID], codes
    assert "capturing" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((z == 1.0).all())         # nothing of the refused calls was enqueued
    with pytest.raises(RuntimeError):
        A.transpose_info()                                           # and nothing was reserved
    A.spmv_transpose(x, y)                                           # outside the capture the first call reserves
    assert A.transpose_info()["nnz"] == A.nnz


# ------------------------------------------------------------------------------------------------ 8. oneMKL pin (where the runtime exists)
def test_spmv_transpose_equals_mkl_sparse_d_mv_transpose():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import mkl_ref
    if not mkl_ref.available():
        pytest.skip("oneMKL runtime not on this box (oracle/mkl_ref.py)")
    from g4s_amd import host
    lib = mkl_ref.load()

    class Descr(C.Structure):
        _fields_ = [("type", C.c_int), ("mode", C.c_int), ("diag", C.c_int)]

    lib.mkl_sparse_d_mv.argtypes = [C.c_int, C.c_double, C.c_void_p, Descr, C.c_void_p, C.c_double, C.c_void_p]
    rows, cols = 20000, 15000
    rp, ci, va = power_law_csr(rows, cols, 60, 2000)
    rng = np.random.default_rng(60)
    x = rng.uniform(-1, 1, rows)
    y0 = rng.uniform(-1, 1, cols)
    h = C.c_void_p()
    rs, re = np.ascontiguousarray(rp[:-1]), np.ascontiguousarray(rp[1:])
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mkl_sparse_d_create_csr(C.byref(h), mkl_ref.SPARSE_INDEX_BASE_ZERO, rows, cols, P(rs), P(re), P(ci), P(va)) == 0
    want = y0.copy()
    SPARSE_OPERATION_TRANSPOSE, SPARSE_MATRIX_TYPE_GENERAL, SPARSE_FILL_MODE_LOWER, SPARSE_DIAG_NON_UNIT = 11, 20, 40, 50
    st = lib.mkl_sparse_d_mv(SPARSE_OPERATION_TRANSPOSE, 1.5, h, Descr(SPARSE_MATRIX_TYPE_GENERAL, SPARSE_FILL_MODE_LOWER, SPARSE_DIAG_NON_UNIT),
                             P(x), 0.25, P(want))
    lib.mkl_sparse_destroy(h)
    assert st == 0
    A = host.CSR.from_host(rp, ci, va, rows, cols)
    got = A.spmv_transpose(_cuda(x), _cuda(y0), 1.5, 0.25).cpu().numpy()
    scale = np.zeros(cols)
    np.add.at(scale, ci, np.abs(va * x[np.repeat(np.arange(rows), np.diff(rp))]))
    assert np.all(np.abs(got - want) <= 1e-10 * (1.5 * scale + 0.25 * np.abs(y0)) + 1e-300)
