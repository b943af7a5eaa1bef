"""Semiring SpMV (include/g4s.h, g4s_spmv_semiring): min-plus, max-plus and or-and, with and without G4S_SPMV_ACCUMULATE, on all four SpMV paths
(row-streaming 0, blocked 1, diagonal 3, block-row 4). Values must equal the numpy reference (tests/spmv_semiring_ref.py) bit for bit: min, max and or do
not depend on the order in which the products arrive, so every path — the blocked one with its LDS atomics included — is exact and deterministic.

The blocked-path cases choose x so that a stray 0.0 shows (a pad product, a DPP lane past its row, a consumer pad slot): min-plus with entries in [1, 2]
and x >= 0 (every product >= 1), max-plus with x <= −2.5 (every product < 0)."""
import numpy as np
import pytest
import torch

from tests import spmv_semiring_ref as ref
from tests.helpers import power_law_csr, random_csr

pytestmark = pytest.mark.gpu
NEW = ref.NEW
WIDE, NARROW = 20448, 16384
STREAM, BLOCKED, DIAGONAL, BLOCKROW = 0, 1, 3, 4


def _handle(rp, ci, va, rows, cols, flags=0, path=None):
    from g4s_amd import host
    A = host.CSR.from_host(rp, ci, va, rows, cols, spmv_flags=flags)
    if path is not None:
        assert A.info()["spmv_path"] == path, A.info()
    return A


def _x_for(semiring, cols, rng, trap=False):
    """x for a semiring; trap=True: the distributions of the module docstring (a stray 0.0 changes the result)"""
    if semiring == "min_plus":
        return rng.uniform(0.0, 1.0, cols) if trap else rng.uniform(-1, 1, cols)
    if semiring == "max_plus":
        return rng.uniform(-3.0, -2.5, cols) if trap else rng.uniform(-1, 1, cols)
    x = rng.uniform(-1, 1, cols)
    x[rng.random(cols) < 0.5] = 0.0                                  # or-and: half of x is "false"
    return x


def _y0_for(semiring, rows, rng):
    y = rng.uniform(-2, 2, rows)
    if semiring == "or_and":
        y = np.where(rng.random(rows) < 0.7, 0.0, 5.0)               # 5.0 must come back as 1.0
    return y


def _check(A, rp, ci, va, x, semiring, accumulate, y0=None, y_dev=None):
    """One product on the device against the reference, bit for bit; returns the device result."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if accumulate:
        yd = torch.from_numpy(y0.copy()).cuda() if y_dev is None else y_dev.copy_(torch.from_numpy(y0))
    else:
        yd = y_dev
        if yd is not None:
            yd.fill_(float("nan"))                                   # never read without ACCUMULATE
    out = A.spmv_semiring(xd, yd, semiring=semiring, accumulate=accumulate).cpu().numpy()
    want = ref.spmv(rp, ci, va, x, semiring, y0 if accumulate else None)
    bad = np.flatnonzero((out + 0.0) != (want + 0.0))
    assert bad.size == 0, (f"{semiring} acc={accumulate}: {bad.size} rows differ, first {bad[0]}: {out[bad[0]]!r} vs {want[bad[0]]!r} "
                           f"(row length {rp[bad[0] + 1] - rp[bad[0]]})")
    return out


def _all(A, rp, ci, va, seed, trap=False, y_dev=None):
    rng = np.random.default_rng(seed)
    for semiring in NEW:
        x = _x_for(semiring, A.cols, rng, trap)
        y0 = _y0_for(semiring, A.rows, rng)
        for accumulate in (False, True):
            _check(A, rp, ci, va, x, semiring, accumulate, y0, y_dev)


# ------------------------------------------------------------------------------------------------ row-streaming path
def test_streaming_short_rows():
    rp, ci, va = random_csr(3000, 2000, 0.003, 1, empty_rows=(0, 5, 2999))
    _all(_handle(rp, ci, va, 3000, 2000, path=STREAM), rp, ci, va, 1)


def test_streaming_long_rows_chunks_and_fixup():
    from g4s_amd import capi
    rp, ci, va = random_csr(4000, 9000, 0.001, 2, dense_rows=(3, 1000, 3999))   # 9 000 entries: five chunks of 2 048, added by the fix-up
    A = _handle(rp, ci, va, 4000, 9000, flags=capi.SPMV_STREAM, path=STREAM)
    assert A.info()["long_rows"] == 3
    _all(A, rp, ci, va, 2)


def test_streaming_heavy_row_in_a_many_row_block():
    from g4s_amd import capi
    rp, ci, va = power_law_csr(30000, 30000, 3, 1500)               # hundreds of short rows per block and rows of > 64 entries among them
    lens = np.diff(rp)
    assert (lens > 64).any() and (lens == 0).any()
    _all(_handle(rp, ci, va, 30000, 30000, flags=capi.SPMV_STREAM, path=STREAM), rp, ci, va, 3)


def test_streaming_lanes_per_row_branch():
    from g4s_amd import capi
    rp, ci, va = random_csr(300, 6000, 0.05, 4)                     # ~300 entries per row: a handful of rows per block, several lanes per row
    _all(_handle(rp, ci, va, 300, 6000, flags=capi.SPMV_STREAM, path=STREAM), rp, ci, va, 4)


# ------------------------------------------------------------------------------------------------ diagonal path
def test_diagonal_laplacian_with_boundary_rows():
    from g4s_amd import host
    A = host.laplacian_csr(7, 21, 19, 17)                           # odd row count; boundary rows have fewer diagonals
    assert A.info()["spmv_path"] == DIAGONAL and A.rows % 2 == 1
    rp, ci, va = A.to_host()
    _all(A, rp, ci, va, 5)


def test_diagonal_banded_odd_rows_and_unaligned_y():
    from g4s_amd import host
    A = host.banded_csr(5001, 3, 11)
    assert A.info()["spmv_path"] == DIAGONAL
    rp, ci, va = A.to_host()
    _all(A, rp, ci, va, 6)
    buf = torch.empty(A.rows + 1, dtype=torch.float64, device="cuda")
    y_odd = buf[1:]                                                 # 8-byte but not 16-byte aligned: the one-row kernel takes every row
    assert y_odd.data_ptr() % 16 == 8
    _all(A, rp, ci, va, 7, y_dev=y_odd)


# ------------------------------------------------------------------------------------------------ block-row path
def _block_csr(nbr, nbc, b, per_row, seed):
    """aligned b×b blocks, per_row sorted block columns per block-row, values U(−1, 1) with some stored zeros"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(nbr):
        bc = np.sort(rng.choice(nbc, per_row, replace=False))
        rows.append(bc)
    rp = [0]
    ci = []
    for n in range(nbr):
        for d in range(b):
            for bc in rows[n]:
                ci.extend(range(bc * b, bc * b + b))
            rp.append(len(ci))
    va = rng.uniform(-1, 1, len(ci))
    va[rng.random(len(ci)) < 0.05] = 0.0
    return np.array(rp, np.int32), np.array(ci, np.int32), va


@pytest.mark.parametrize("b", [2, 3, 4])
def test_block_row(b):
    nbr = 700
    rp, ci, va = _block_csr(nbr, 900, b, 5, 20 + b)
    A = _handle(rp, ci, va, nbr * b, 900 * b, path=BLOCKROW)
    _all(A, rp, ci, va, 8 + b)


# ------------------------------------------------------------------------------------------------ blocked path
@pytest.fixture(params=["device", "16384"])
def band(request, monkeypatch):
    if request.param == "16384":
        monkeypatch.setenv("G4S_PB_BAND", "16384")
    else:
        monkeypatch.delenv("G4S_PB_BAND", raising=False)
    return NARROW if request.param == "16384" else WIDE


def _blocked(rp, ci, va, rows, cols, updatable=False):
    from g4s_amd import capi
    return _handle(rp, ci, va, rows, cols, flags=capi.SPMV_BLOCKED | (capi.SPMV_UPDATABLE if updatable else 0), path=BLOCKED)


def _trap_values(n, rng):
    return rng.uniform(1.0, 2.0, n)


@pytest.mark.parametrize("shape", [(0, 1, 2, 1), (1, 1, 3, -1), (3, 0, 3, 0)])
def test_blocked_shapes_around_band_multiples(band, shape):
    rows, cols = shape[0] * band + shape[1] * 7 + 50, shape[2] * band + shape[3]
    rp, ci, va = power_law_csr(rows, cols, rows + cols, 3000)
    ci = ci.copy()
    if rp[-1] > rp[-2]:
        ci[rp[-1] - 1] = cols - 1                                   # the last column and the last row are populated
    va = _trap_values(len(ci), np.random.default_rng(rows))
    _all(_blocked(rp, ci, va, rows, cols), rp, ci, va, 12, trap=True)


@pytest.mark.parametrize("hot", ["0", "64"])
def test_blocked_hot_bands(band, monkeypatch, hot):
    monkeypatch.setenv("G4S_PB_HOT_BANDS", hot)
    rng = np.random.default_rng(13)
    rows, cols = 60000, (130 * band if hot == "64" else 200000)
    popular = rng.choice(cols, 64 * band + 1000 if hot == "64" else 3000, replace=False)
    lens = rng.integers(0, 12, rows)
    lens[7] = 30000
    k = int(lens.sum())
    c = np.where(rng.random(k) < 0.6, popular[rng.integers(0, len(popular), k)], rng.integers(0, cols, k)).astype(np.int64)
    key = np.unique(np.repeat(np.arange(rows), lens) * cols + c)
    r, c = key // cols, key % cols
    rp = np.zeros(rows + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    rp, ci = np.cumsum(rp).astype(np.int32), c.astype(np.int32)
    va = _trap_values(len(ci), rng)
    _all(_blocked(rp, ci, va, rows, cols), rp, ci, va, 14, trap=True)


def test_blocked_split_row_bands(band, monkeypatch):
    monkeypatch.setenv("G4S_PB_CCHUNK", "2048")                      # every band of > 2 048 micro-runs is split: y starts from the identity / old y
    rows, cols = 2 * band + 100, 3 * band
    rp, ci, va = power_law_csr(rows, cols, 31, 6000)
    va = _trap_values(len(ci), np.random.default_rng(15))
    _all(_blocked(rp, ci, va, rows, cols), rp, ci, va, 15, trap=True)


def test_blocked_consumer_pad_slots(band):
    # Several row bands whose micro-run counts are not multiples of 4, local row 0 of every band populated: a band's pad slots (value 0 for local row 0)
    # must not enter a min (true result >= 1) or a max (true result < 0)
    rows, cols = 4 * band + 10, 2 * band + 3
    for seed in (41, 42, 43):
        rp, ci, va = power_law_csr(rows, cols, seed, 500)
        rng = np.random.default_rng(seed)
        per_row = np.split(ci, rp[1:-1])
        for r0 in range(0, rows, band):
            per_row[r0] = np.sort(rng.choice(cols, 3 + seed % 3, replace=False)).astype(np.int32)   # local row 0 of each band: a few entries
        lens = np.array([len(c) for c in per_row])
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ci = np.concatenate(per_row).astype(np.int32)
        va = _trap_values(len(ci), rng)
        A = _blocked(rp, ci, va, rows, cols)
        for semiring in ("min_plus", "max_plus"):
            x = _x_for(semiring, cols, rng, trap=True)
            y = _check(A, rp, ci, va, x, semiring, False)
            for r0 in range(0, rows, band):
                assert (y[r0] >= 1.0) if semiring == "min_plus" else (y[r0] < 0.0)
            _check(A, rp, ci, va, x, semiring, True, _y0_for(semiring, rows, rng))


def test_blocked_producer_pads_never_read_x(band):
    # +inf / −inf / NaN in every empty column and in the band-edge columns a pad's local column could alias: pads read the word behind the band of x,
    # never x, so every row (none of them touches those columns) is exact
    rows, half = 50000, 2 * band + 6
    rp, ci, va = power_law_csr(rows, half, 29, 4000)
    ci, cols = 2 * ci, 2 * half                                      # every odd column is empty
    rng = np.random.default_rng(4)
    va = _trap_values(len(ci), rng)
    empty = np.setdiff1d(np.arange(cols), ci)
    edges = np.array([c for c in (0, band - 1, band, 2 * band - 1, 2 * band, cols - 1) if c in set(empty.tolist())])
    A = _blocked(rp, ci, va, rows, cols)
    for semiring in NEW:
        x = _x_for(semiring, cols, rng, trap=True)
        x[empty] = np.array([np.inf, -np.inf, np.nan])[np.arange(len(empty)) % 3]
        x[edges] = np.nan
        for accumulate in (False, True):
            y = _check(A, rp, ci, va, x, semiring, accumulate, _y0_for(semiring, rows, rng))
            assert not np.isnan(y).any()


def test_blocked_dpp_row_ends_and_single_run_windows(band):
    # row 3 holds every column of the first two bands (windows that are one run); rows 4–40 hold runs of 1–37 consecutive columns starting at every offset
    # of a window, so runs end on every lane of a 16-lane DPP row, the last one included
    rows, cols = 3 * band + 5, 3 * band + 7
    rng = np.random.default_rng(3)
    per_row = [np.array([], np.int64)] * rows
    per_row[3] = np.arange(0, 2 * band + 300)
    for r in range(4, 41):
        s = int(rng.integers(0, cols - 40))
        per_row[r] = np.arange(s, s + r - 3)
    for r in range(41, 73):                                          # 32 rows of 16 entries each in a row: every run fills exactly half a window
        per_row[r] = np.arange(16 * (r - 41), 16 * (r - 40)) + band
    per_row[rows - 1] = np.array([0, band - 1, band, cols - 1])
    for r in range(73, rows - 1, 7):
        per_row[r] = np.unique(rng.integers(0, cols, 5))
    lens = np.array([len(c) for c in per_row])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(per_row).astype(np.int32)
    va = _trap_values(len(ci), rng)
    _all(_blocked(rp, ci, va, rows, cols), rp, ci, va, 16, trap=True)


# ------------------------------------------------------------------------------------------------ edge values
@pytest.mark.parametrize("path", ["stream", "blocked"])
def test_edge_values(path):
    from g4s_amd import capi
    rows = cols = 50000
    rp, ci, va = power_law_csr(rows, cols, 51, 3000)
    rng = np.random.default_rng(51)
    va = va.copy()
    va[rng.random(len(va)) < 0.1] = 0.0                              # stored zeros
    va[rng.random(len(va)) < 0.01] = np.nan                          # NaN counts as nonzero for or-and
    lens = np.diff(rp)
    assert (lens == 0).sum() > 100
    A = _handle(rp, ci, va, rows, cols, flags=capi.SPMV_STREAM if path == "stream" else capi.SPMV_BLOCKED, path=STREAM if path == "stream" else BLOCKED)
    x = rng.uniform(-1, 1, cols)
    x[rng.random(cols) < 0.3] = 0.0
    y0 = np.where(rng.random(rows) < 0.5, 0.0, 5.0)
    y = _check(A, rp, ci, va, x, "or_and", False)
    assert set(np.unique(y)) <= {0.0, 1.0} and np.all(y[lens == 0] == 0.0)
    y = _check(A, rp, ci, va, x, "or_and", True, y0)
    assert set(np.unique(y)) <= {0.0, 1.0} and np.array_equal(y[lens == 0], (y0[lens == 0] != 0).astype(float))
    # min/max-plus: NaN-free values, +inf in x; empty rows get the identity or keep y
    va2 = np.where(np.isnan(va), 0.5, va)
    A.update_values(torch.from_numpy(va2).cuda())
    x2 = rng.uniform(-1, 1, cols)
    x2[rng.random(cols) < 0.2] = np.inf
    for semiring, ident in (("min_plus", np.inf), ("max_plus", -np.inf)):
        y = _check(A, rp, ci, va2, x2, semiring, False)
        assert np.all(y[lens == 0] == ident)
        y0 = rng.uniform(-2, 2, rows)
        y = _check(A, rp, ci, va2, x2, semiring, True, y0)
        assert np.array_equal(y[lens == 0], y0[lens == 0])


# ------------------------------------------------------------------------------------------------ consistency
def _path_cases():
    from g4s_amd import capi, host
    rp, ci, va = power_law_csr(60000, 60000, 61, 3000)
    yield "stream", _handle(rp, ci, va, 60000, 60000, flags=capi.SPMV_STREAM, path=STREAM), (rp, ci, va)
    yield "blocked", _handle(rp, ci, va, 60000, 60000, flags=capi.SPMV_BLOCKED, path=BLOCKED), (rp, ci, va)
    D = host.laplacian_csr(7, 30, 30, 30)
    assert D.info()["spmv_path"] == DIAGONAL
    yield "diagonal", D, D.to_host()
    brp, bci, bva = _block_csr(600, 800, 3, 4, 62)
    yield "blockrow", _handle(brp, bci, bva, 1800, 2400, path=BLOCKROW), (brp, bci, bva)


def test_plus_times_is_g4s_spmv():
    rng = np.random.default_rng(70)
    for name, A, _ in _path_cases():
        x = torch.from_numpy(rng.uniform(-1, 1, A.cols)).cuda()
        y0 = torch.from_numpy(rng.uniform(-1, 1, A.rows)).cuda()
        for accumulate in (False, True):
            a = A.spmv_semiring(x, y0.clone() if accumulate else None, semiring="plus_times", accumulate=accumulate)
            b = A.spmv(x, y0.clone(), 1.0, 1.0 if accumulate else 0.0)
            if name == "blocked":                                    # LDS atomic sums: within the SpMV tolerance
                assert float((a - b).abs().max()) <= 1e-10 * max(float(b.abs().max()), 1.0)
            else:
                assert torch.equal(a, b), name


def test_blocked_repeated_calls_are_bit_identical():
    rng = np.random.default_rng(71)
    _, A, (rp, ci, va) = next((c for c in _path_cases() if c[0] == "blocked"))
    for semiring in NEW:
        x = torch.from_numpy(_x_for(semiring, A.cols, rng)).cuda()
        outs = [A.spmv_semiring(x, semiring=semiring).cpu().numpy() for _ in range(3)]
        assert all(np.array_equal(outs[0], o, equal_nan=True) for o in outs[1:]), semiring


@pytest.mark.parametrize("updatable", [False, True])
def test_update_values_then_semiring(updatable):
    from g4s_amd import capi
    rows = cols = 60000
    rp, ci, va = power_law_csr(rows, cols, 72, 3000)
    flags = capi.SPMV_BLOCKED | (capi.SPMV_UPDATABLE if updatable else 0)
    A = _handle(rp, ci, va, rows, cols, flags=flags, path=BLOCKED)
    rng = np.random.default_rng(72)
    _all(A, rp, ci, va, 73)
    vnew = rng.uniform(-3, 3, len(ci))
    A.update_values(torch.from_numpy(vnew).cuda())
    _all(A, rp, ci, vnew, 74)
    # the other paths read their own copy of the values too
    for name, B, (brp, bci, bva) in _path_cases():
        if name in ("diagonal", "blockrow"):
            v2 = rng.uniform(-3, 3, len(bci))
            B.update_values(torch.from_numpy(v2).cuda())
            _all(B, brp, bci, v2, 75)


def test_graph_capture_replays_eager_on_every_path():
    rng = np.random.default_rng(76)
    for name, A, _ in _path_cases():
        x = torch.from_numpy(rng.uniform(0, 1, A.cols)).cuda()
        d = torch.from_numpy(rng.uniform(0, 1, A.rows)).cuda()
        e = torch.zeros(A.rows, dtype=torch.float64, device="cuda")
        A.spmv_semiring(x, d.clone(), semiring="min_plus", accumulate=True)     # plans and workspaces exist before the capture
        torch.cuda.synchronize()

        def seq(d, e):                                               # a dependent chain: d feeds the second product's x where the shapes allow
            A.spmv_semiring(x, d, semiring="min_plus", accumulate=True)
            A.spmv_semiring(d if A.cols == A.rows else x, e, semiring="max_plus")
            A.spmv_semiring(x, d, semiring="or_and", accumulate=True)

        d_eager, e_eager = d.clone(), e.clone()
        seq(d_eager, e_eager)
        torch.cuda.synchronize()
        d_g, e_g = d.clone(), e.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                seq(d_g, e_g)
        torch.cuda.current_stream().wait_stream(side)
        d_g.copy_(d)
        e_g.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d_g, d_eager) and torch.equal(e_g, e_eager), name


@pytest.mark.parametrize("pointers", ["host", "device"])
def test_one_shot_form(pointers):
    import ctypes as C
    from g4s_amd import capi, host
    lib = capi.load()
    rows, cols = 5000, 4000
    rp, ci, va = random_csr(rows, cols, 0.002, 77, empty_rows=(1, 7))
    rng = np.random.default_rng(77)
    for semiring in NEW:
        x = _x_for(semiring, cols, rng)
        y0 = _y0_for(semiring, rows, rng)
        for accumulate in (False, True):
            flags = host.SEMIRINGS[semiring] | (capi.SPMV_ACCUMULATE if accumulate else 0)
            want = ref.spmv(rp, ci, va, x, semiring, y0 if accumulate else None)
            if pointers == "host":
                y = y0.copy()
                P = lambda a: a.ctypes.data_as(C.c_void_p)
                capi.check(lib.g4s_spmv_semiring_csr_i32_f64(rows, cols, P(rp), P(ci), P(va), P(x), P(y), flags))
            else:
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                drp, dci, dva, dx, dy = t(rp), t(ci), t(va), t(x), t(y0.copy())
                torch.cuda.synchronize()
                P = lambda a: C.c_void_p(a.data_ptr())
                capi.check(lib.g4s_spmv_semiring_csr_i32_f64(rows, cols, P(drp), P(dci), P(dva), P(dx), P(dy), flags | capi.DEVICE_POINTERS))
                y = dy.cpu().numpy()
            assert ref.same_values(y, want), (semiring, accumulate)


# ------------------------------------------------------------------------------------------------ end to end on a weighted R-MAT graph (blocked path)
def _rmat_graph(n=1 << 16, seed=9):
    from g4s_amd import capi, host
    import scipy.sparse as sp
    R = host.rmat_csr(n, 16, 10 * n, seed)
    rp, ci, _ = R.to_host()
    w = np.random.default_rng(seed).integers(1, 11, len(ci)).astype(np.float64)    # integer weights: exact sums
    G = sp.csr_matrix((w, ci, rp), shape=(n, n))
    GT = G.T.tocsr()
    GT.sort_indices()
    AT = host.CSR.from_host(GT.indptr, GT.indices, GT.data, n, n, spmv_flags=capi.SPMV_BLOCKED)   # the CSR of Aᵀ: pull-style relaxation
    assert AT.info()["spmv_path"] == BLOCKED
    return G, AT


def test_bellman_ford_equals_scipy():
    from scipy.sparse.csgraph import shortest_path
    G, AT = _rmat_graph()
    n = G.shape[0]
    src = int(np.argmax(np.diff(G.indptr)))                          # a hub: most of the graph is reachable
    d = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
    d[src] = 0.0
    for it in range(n):
        prev = d.clone()
        AT.spmv_semiring(prev, d, semiring="min_plus", accumulate=True)   # d := d ⊕ (Aᵀ ⊗ d_prev)
        if torch.equal(d, prev):
            break
    want = shortest_path(G, method="D", directed=True, indices=src)
    assert it > 2
    assert ref.same_values(d.cpu().numpy(), want)


def test_bfs_levels_equal_scipy():
    from scipy.sparse.csgraph import shortest_path
    G, AT = _rmat_graph(seed=10)
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
        reach = AT.spmv_semiring(frontier, semiring="or_and")        # vertices with an edge from the frontier
        frontier = reach * (1.0 - visited)
        level[frontier != 0] = float(depth)
        visited = torch.maximum(visited, frontier)
    want = shortest_path(G, directed=True, unweighted=True, indices=src)
    assert depth > 2
    assert ref.same_values(level.cpu().numpy(), want)
