"""GPU parity of g4s_spmm (Y = alpha·A·X + beta·Y, X: cols × k) against the oracle's SpMV run column by column.

Tolerance (fp64), per element: |Y_gpu − Y_oracle|_ij ≤ 1e-10 · (|alpha|·Σ_k |a_ik x_kj| + |beta|·|y0_ij|), as in test_spmv_gpu._check. Rows of at most 2048
entries are summed in stored order on every handle, so they must be BIT-identical to the oracle; rows split into chunks are within the tolerance and
equal run to run."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import power_law_csr, random_csr

pytestmark = pytest.mark.gpu
TOL = 1e-10
NAN = float("nan")


def _oracle_block(oracle, rp, ci, va, X, alpha=1.0, beta=0.0, Y0=None):
    """(want, scale): the oracle's SpMV per column of X, and the tolerance scale of every element."""
    rows, k = len(rp) - 1, X.shape[1]
    want, scale = np.zeros((rows, k)), np.zeros((rows, k))
    for j in range(k):
        x = np.ascontiguousarray(X[:, j])
        want[:, j] = oracle.spmv(rp, ci, va, x, None if Y0 is None else Y0[:, j], alpha, beta)
        scale[:, j] = abs(alpha) * oracle.spmv_ld(rp, ci, va, x)[1] + (0.0 if Y0 is None else abs(beta) * np.abs(Y0[:, j]))
    return want, scale


def _device_block(M, col_major, ld=None, offset=0, fill=NAN):
    """A strided device view of the host block M (r × k) inside a larger buffer filled with `fill`: leading dimension ld, `offset` doubles in."""
    r, k = M.shape
    ld = ld or (r if col_major else k)
    extent = ((k - 1) * ld + r if col_major else (r - 1) * ld + k) if r and k else 0
    buf = torch.full((offset + extent + 3,), fill, dtype=torch.float64, device="cuda")
    stride = (1, ld) if col_major else (ld, 1)
    view = torch.as_strided(buf, (r, k), stride, offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(M)).cuda())
    return buf, view


def _check(oracle, A, rp, ci, va, X, alpha=1.0, beta=0.0, Y0=None, col_major=False, ld_pad=0, offset=0, exact=False):
    rows, k = len(rp) - 1, X.shape[1]
    _, xd = _device_block(X, col_major, (A.cols if col_major else k) + ld_pad, offset)
    y_init = Y0 if Y0 is not None else np.full((rows, k), NAN)              # beta == 0: NaN in Y must not leak
    ybuf, yd = _device_block(y_init, col_major, (rows if col_major else k) + ld_pad, offset, fill=-7.25)
    pad_before = ybuf.clone()
    A.spmm(xd, yd, alpha, beta)
    torch.cuda.synchronize()
    got = yd.cpu().numpy()
    want, scale = _oracle_block(oracle, rp, ci, va, X, alpha, beta, Y0)
    err = np.abs(got - want)
    assert np.all(err <= TOL * scale + 1e-300), f"max rel err {np.max(err / (scale + 1e-300))}"
    if exact:
        assert np.array_equal(got, want)
    mask = torch.ones_like(ybuf, dtype=torch.bool)
    torch.as_strided(mask, yd.shape, yd.stride(), offset).fill_(False)
    assert torch.equal(ybuf[mask], pad_before[mask]), "padding of Y was touched"
    return got


def _rmat(path):
    from g4s_amd import capi, host
    n = 1 << 16
    R = host.rmat_csr(n, 16, 12 * n, 5)
    A = host.CSR(R.rowptr, R.colids, R.values, n, n, spmv_flags=capi.SPMV_STREAM if path == "stream" else capi.SPMV_BLOCKED)
    assert A.info()["spmv_path"] == (0 if path == "stream" else 1)
    return A


def _fe_matrix():
    from tests.helpers import assemble_csr, hex_mesh, spd_blocks
    ien, idmap, nno, neq = hex_mesh(12, 10, 6)
    K = spd_blocks(len(ien), 24, 3)
    return assemble_csr(ien, idmap, K, neq), neq


def _handle(path):
    from g4s_amd import host
    if path in ("stream", "blocked"):
        A = _rmat(path)
    elif path == "diagonal":
        A = host.laplacian_csr(7, 24, 20, 16)
        assert A.info()["spmv_path"] == 3
    else:
        (rp, ci, va), neq = _fe_matrix()
        A = host.CSR.from_host(rp, ci, va, neq, neq)
        assert A.info()["spmv_path"] == 4
    return A


@pytest.mark.parametrize("path", ["stream", "blocked", "diagonal", "block_row"])
def test_spmm_every_handle_path(oracle, path):
    A = _handle(path)
    rp, ci, va = A.to_host()
    rng = np.random.default_rng(1)
    for k, cm in ((1, False), (8, False), (8, True), (33, False)):
        X = rng.uniform(-1, 1, (A.cols, k))
        _check(oracle, A, rp, ci, va, X, col_major=cm, exact=path in ("diagonal", "block_row"))
        Y0 = rng.uniform(-1, 1, (A.rows, k))
        _check(oracle, A, rp, ci, va, X, -2.5, 0.75, Y0, col_major=cm, exact=path in ("diagonal", "block_row"))
    assert A.info()["spmv_path"] == {"stream": 0, "blocked": 1, "diagonal": 3, "block_row": 4}[path]


@pytest.mark.parametrize("col_major", [False, True])
def test_spmm_shapes_of_k_rectangular(oracle, col_major):
    from g4s_amd import host
    rows, cols = 3000, 2100
    rp, ci, va = random_csr(rows, cols, 0.004, 11, empty_rows=[0, 5, 1700])
    A = host.CSR.from_host(rp, ci, va, rows, cols)
    rng = np.random.default_rng(2)
    for k in (1, 2, 3, 5, 8, 16, 31, 32, 33, 64, 65):
        X = rng.uniform(-1, 1, (cols, k))
        _check(oracle, A, rp, ci, va, X, col_major=col_major, exact=True)
        _check(oracle, A, rp, ci, va, X, -2.5, 0.75, rng.uniform(-1, 1, (rows, k)), col_major=col_major, exact=True)


@pytest.mark.parametrize("col_major", [False, True])
@pytest.mark.parametrize("k,ld_pad,offset", [(8, 3, 0), (8, 0, 1), (5, 2, 1), (16, 1, 1), (33, 5, 0)])
def test_spmm_layout_edge_cases(oracle, col_major, k, ld_pad, offset):
    """ld > k (odd ld among them), bases one double off the 16-byte grid, sentinel padding of Y that must come back unchanged."""
    from g4s_amd import host
    rows, cols = 1500, 1300
    rp, ci, va = random_csr(rows, cols, 0.01, 3)
    A = host.CSR.from_host(rp, ci, va, rows, cols)
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (cols, k))
    _check(oracle, A, rp, ci, va, X, col_major=col_major, ld_pad=ld_pad, offset=offset, exact=True)
    _check(oracle, A, rp, ci, va, X, -2.5, 0.75, rng.uniform(-1, 1, (rows, k)), col_major=col_major, ld_pad=ld_pad, offset=offset, exact=True)


def test_spmm_row_shapes(oracle):
    """Empty rows, an nnz == 0 matrix (Y = beta·Y), rows == 0, k == 0, and rows longer than 2048 entries (long-row chunks + fix-up)."""
    from g4s_amd import capi, host
    rng = np.random.default_rng(6)
    rp, ci, va = power_law_csr(6000, 9000, 7, 7000)
    A = host.CSR.from_host(rp, ci, va, 6000, 9000, spmv_flags=capi.SPMV_STREAM)
    assert A.info()["long_rows"] > 0 and (np.diff(rp) == 0).any()
    for k, cm in ((1, False), (3, False), (8, True), (40, False)):
        X = rng.uniform(-1, 1, (9000, k))
        _check(oracle, A, rp, ci, va, X, col_major=cm)
        _check(oracle, A, rp, ci, va, X, 0.5, -1.25, rng.uniform(-1, 1, (6000, k)), col_major=cm)
        xd = torch.from_numpy(X).cuda()
        assert torch.equal(A.spmm(xd), A.spmm(xd))                            # chunk partials added in a fixed order
    # nnz == 0
    Z = host.CSR.from_host(np.zeros(51, np.int32), np.zeros(0, np.int32), np.zeros(0), 50, 40)
    Y0 = rng.uniform(-1, 1, (50, 4))
    _check(oracle, Z, np.zeros(51, np.int32), np.zeros(0, np.int32), np.zeros(0), rng.uniform(-1, 1, (40, 4)), 2.0, 0.5, Y0)
    _check(oracle, Z, np.zeros(51, np.int32), np.zeros(0, np.int32), np.zeros(0), rng.uniform(-1, 1, (40, 4)))
    # rows == 0
    E = host.CSR.from_host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, 7)
    assert E.spmm(torch.ones(7, 3, dtype=torch.float64, device="cuda")).shape == (0, 3)
    # k == 0: a no-op through the C-ABI, Y untouched
    lib = capi.load()
    y = torch.full((6000, 2), 3.0, dtype=torch.float64, device="cuda")
    capi.check(lib.g4s_spmm(A.handle, 0, C.c_void_p(0), 0, C.c_void_p(y.data_ptr()), 0, 1.0, 0.0, 0, None))
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


def test_spmm_bit_exact_and_reproducible(oracle):
    from g4s_amd import capi, host
    rng = np.random.default_rng(8)
    rp, ci, va = oracle.laplacian5(200, 150)
    A = host.CSR.from_host(rp, ci, va, 30000, 30000)
    for k in (1, 4, 8, 32):
        _check(oracle, A, rp, ci, va, rng.uniform(-1, 1, (30000, k)), exact=True)
    for seed in (1, 2):
        rp, ci, va = random_csr(20000, 15000, 0.002, seed)
        S = host.CSR.from_host(rp, ci, va, 20000, 15000, spmv_flags=capi.SPMV_STREAM)
        for k in (2, 8, 17):
            _check(oracle, S, rp, ci, va, rng.uniform(-1, 1, (15000, k)), exact=True)
            _check(oracle, S, rp, ci, va, rng.uniform(-1, 1, (15000, k)), -2.5, 0.75, rng.uniform(-1, 1, (20000, k)), col_major=True, exact=True)
    B = _rmat("blocked")
    for k in (1, 8):
        X = host.synth_vector(9, B.cols * k).view(B.cols, k)
        assert torch.equal(B.spmm(X), B.spmm(X))


def test_spmm_column_equals_spmv(oracle):
    A = _rmat("stream")
    X = torch.from_numpy(np.random.default_rng(10).uniform(-1, 1, (A.cols, 6))).cuda()
    Y = A.spmm(X)
    rp, ci, va = A.to_host()
    for j in range(6):
        y = A.spmv(X[:, j].contiguous())
        _, asum = oracle.spmv_ld(rp, ci, va, X[:, j].cpu().numpy())
        assert np.all(np.abs((Y[:, j] - y).cpu().numpy()) <= 2 * TOL * asum + 1e-300)


def test_spmm_after_update_values(oracle):
    from g4s_amd import capi, host
    rng = np.random.default_rng(12)
    lib = capi.load()
    # borrowed: stream, blocked + updatable, diagonal
    n = 1 << 14
    R = host.rmat_csr(n, 14, 10 * n, 3)
    for flags in (capi.SPMV_STREAM, capi.SPMV_BLOCKED | capi.SPMV_UPDATABLE, capi.SPMV_BLOCKED):
        A = host.CSR(R.rowptr, R.colids, R.values.clone(), n, n, spmv_flags=flags)
        rp, ci, _ = A.to_host()
        X = rng.uniform(-1, 1, (n, 8))
        A.spmm(torch.from_numpy(X).cuda())
        vnew = rng.uniform(-1, 1, A.nnz)
        A.update_values(torch.from_numpy(vnew).cuda())
        _check(oracle, A, rp, ci, vnew, X)
    D = host.laplacian_csr(7, 20, 20, 10)
    rp, ci, va = D.to_host()
    D.spmm(torch.ones(D.cols, 4, dtype=torch.float64, device="cuda"))
    vnew = rng.uniform(-1, 1, D.nnz)
    D.update_values(torch.from_numpy(vnew).cuda())
    _check(oracle, D, rp, ci, vnew, rng.uniform(-1, 1, (D.cols, 4)), exact=True)
    # owned copy (host pointers at create, host values at update)
    rp, ci, va = random_csr(4000, 3000, 0.003, 5)
    h = C.c_void_p()
    capi.check(lib.g4s_csr_create(C.byref(h), 4000, 3000, len(ci), rp.ctypes.data, ci.ctypes.data, va.ctypes.data, capi.HOST_POINTERS))
    try:
        X = rng.uniform(-1, 1, (3000, 5))
        xd = torch.from_numpy(X).cuda()
        yd = torch.empty(4000, 5, dtype=torch.float64, device="cuda")
        vnew = rng.uniform(-1, 1, len(ci))
        for v in (va, vnew):
            if v is vnew:
                capi.check(lib.g4s_csr_update_values(h, vnew.ctypes.data, capi.HOST_POINTERS, None))
            capi.check(lib.g4s_spmm(h, 5, C.c_void_p(xd.data_ptr()), 5, C.c_void_p(yd.data_ptr()), 5, 1.0, 0.0, 0, None))
            torch.cuda.synchronize()
            want, _ = _oracle_block(oracle, rp, ci, v, X)
            assert np.array_equal(yd.cpu().numpy(), want)
    finally:
        lib.g4s_csr_destroy(h)


@pytest.mark.parametrize("col_major", [False, True])
def test_spmm_one_shot_form(oracle, col_major):
    from g4s_amd import capi
    lib = capi.load()
    rows, cols, k = 2500, 1800, 6
    rp, ci, va = random_csr(rows, cols, 0.005, 13)
    rng = np.random.default_rng(14)
    X, Y0 = rng.uniform(-1, 1, (cols, k)), rng.uniform(-1, 1, (rows, k))
    want, scale = _oracle_block(oracle, rp, ci, va, X, -1.5, 0.25, Y0)
    flags = capi.SPMM_COL_MAJOR if col_major else 0
    # host pointers, padded leading dimensions: the padding comes back as it was
    ldx, ldy = (cols + 3, rows + 1) if col_major else (k + 3, k + 1)
    hx = np.full((k, ldx) if col_major else (cols, ldx), NAN)
    hy = np.full((k, ldy) if col_major else (rows, ldy), -3.0)
    if col_major:
        hx[:, :cols], hy[:, :rows] = X.T, Y0.T
    else:
        hx[:, :k], hy[:, :k] = X, Y0
    capi.check(lib.g4s_spmm_csr_i32_f64(rows, cols, k, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, hx.ctypes.data, ldx, hy.ctypes.data, ldy,
                                        -1.5, 0.25, flags | capi.HOST_POINTERS))
    got = hy[:, :rows].T if col_major else hy[:, :k]
    assert np.array_equal(got, want)
    assert np.all((hy[:, rows:] if col_major else hy[:, k:]) == -3.0)
    # device pointers
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    drp, dci, dva = dev(rp), dev(ci), dev(va)
    dx = dev(X.T if col_major else X)
    dy = dev(Y0.T if col_major else Y0)
    capi.check(lib.g4s_spmm_csr_i32_f64(rows, cols, k, C.c_void_p(drp.data_ptr()), C.c_void_p(dci.data_ptr()), C.c_void_p(dva.data_ptr()),
                                        C.c_void_p(dx.data_ptr()), cols if col_major else k, C.c_void_p(dy.data_ptr()), rows if col_major else k,
                                        -1.5, 0.25, flags | capi.DEVICE_POINTERS))
    got = dy.cpu().numpy()
    got = got.T if col_major else got
    assert np.all(np.abs(got - want) <= TOL * scale + 1e-300)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("path", ["stream", "blocked"])
def test_spmm_chain_in_a_hipgraph(path):
    """Reserve, then record Y = A·X three times and Z = A·Y on a side stream; replays reproduce the eager result bit for bit."""
    A = _rmat(path)
    k = 8
    A.spmm_reserve(k)
    from g4s_amd import host
    X = host.synth_vector(3, A.cols * k).view(A.cols, k)
    Y = torch.zeros(A.rows, k, dtype=torch.float64, device="cuda")
    Z = torch.zeros_like(Y)
    A.spmm(X, Y)
    eager_y = Y.clone()
    eager_z = A.spmm(eager_y)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(3):
                A.spmm(X, Y)
            A.spmm(Y, Z)
    torch.cuda.current_stream().wait_stream(side)
    Y.zero_()
    Z.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Y, eager_y) and torch.equal(Z, eager_z)
    Z.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Z, eager_z)


def test_spmm_unreserved_handle_refuses_capture():
    """A handle that still needs workspace refuses a g4s_spmm inside a capture (G4S_ERR_INVALID, nothing enqueued) and works eagerly afterwards."""
    from g4s_amd import capi, host
    A = _rmat("blocked")                                             # never reserved, never used for SpMM
    lib = capi.load()
    k = 4
    X = host.synth_vector(5, A.cols * k).view(A.cols, k)
    Y = torch.zeros(A.rows, k, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    status, msg = None, ""
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            Y.add_(1.0)
            status = lib.g4s_spmm(A.handle, k, C.c_void_p(X.data_ptr()), k, C.c_void_p(Y.data_ptr()), k, 1.0, 0.0, 0, C.c_void_p(side.cuda_stream))
            msg = lib.g4s_last_error().decode()
    torch.cuda.current_stream().wait_stream(side)
    assert status == capi.ERR_INVALID and "g4s_csr_spmm_reserve" in msg
    g.replay()
    torch.cuda.synchronize()
    assert bool((Y == 1.0).all())                                    # the graph holds the add only
    first = A.spmm(X)                                                # eager: reserves on the spot
    assert torch.equal(first, A.spmm(X))


def test_spmm_medium_rmat(oracle):
    """R-MAT 2^20 on the blocked path, device pointers: large enough that g4s_csr_create defers the row-streaming plan, so the first SpMM builds it
    (and adds it to plan_bytes, next to the blocked plan's bytes)."""
    from g4s_amd import capi, host
    n = 1 << 20
    A = host.rmat_csr(n, 20, 16 * n, 21, spmv_flags=capi.SPMV_BLOCKED)
    assert A.nnz > 10_000_000
    before = A.info()
    assert before["spmv_path"] == 1 and before["stream_blocks"] == 0        # no streaming plan yet
    rp, ci, va = A.to_host()
    X = np.random.default_rng(15).uniform(-1, 1, (n, 8))
    Y = A.spmm(torch.from_numpy(X).cuda()).cpu().numpy()
    want, scale = _oracle_block(oracle, rp, ci, va, X)
    assert np.all(np.abs(Y - want) <= TOL * scale + 1e-300)
    after = A.info()
    assert after["spmv_path"] == 1 and after["stream_blocks"] > 0          # built on demand by the first SpMM
    assert after["plan_bytes"] >= before["plan_bytes"] + 16 * after["stream_blocks"]
