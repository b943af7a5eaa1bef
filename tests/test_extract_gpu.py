"""g4s_csr_extract_* on the device against tests/extract_ref.py: every comparison is == on the row pointers, the column ids and the int64 view of the
values. Values are distinct doubles (a permutation + 1), so a wrong gather shows. Shapes are the smallest at which a path can go wrong: the unit edges
(0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 200 stored entries), the three sort classes at their thresholds (64 | 65, lds_sort_max | lds_sort_max + 1), every
kind of J, a multiplicity hub, non-canonical rows, the device-side refusals each followed by an exact call, and the int32 overflow."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import extract_ref as ref

pytestmark = pytest.mark.gpu

GUARD_I, GUARD_D = -77, -77.5


def _mods():
    from g4s_amd import capi, host
    return capi, host


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _Q(t):
    """never NULL for a tensor (an empty one gets a pointer nobody reads); NULL for None"""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() if t.numel() else _PLACE.data_ptr())


_PLACE = None


@pytest.fixture(autouse=True, scope="module")
def _placeholder():
    global _PLACE
    _PLACE = torch.zeros(4, dtype=torch.float64, device="cuda")
    yield
    _PLACE = None


def _rows_of(lengths, cols, seed, canonical=True):
    """(rowptr, colids, values): row r holds lengths[r] distinct columns, ascending when canonical"""
    rng = np.random.default_rng(seed)
    ci = [rng.choice(cols, n, replace=False) for n in lengths]
    ci = [np.sort(c) if canonical else c for c in ci]
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate(ci).astype(np.int32) if len(lengths) else np.zeros(0, np.int32)
    return rp, ci, rng.permutation(ci.size).astype(np.float64) + 1.0


def _csr(A, rows, cols):
    _, host = _mods()
    return host.CSR.from_host(A[0], A[1], A[2], rows, cols)


def _same(c, want, src=None, A=None, J=None):
    rp, ci, va = c.to_host()
    assert np.array_equal(rp, want[0]) and np.array_equal(ci, want[1]) and np.array_equal(_bits(va), _bits(want[2]))
    if src is not None:
        s = src.cpu().numpy()
        assert np.array_equal(s, want[3])
        assert np.array_equal(_bits(A[2][s]), _bits(va)) and np.array_equal(A[1][s], (np.arange(c.cols) if J is None else np.asarray(J))[ci])


def _check(A, rows, cols, I, J, **kw):
    """host.csr_extract against the reference; returns the info dict"""
    _, host = _mods()
    c, src, info = host.csr_extract(_csr(A, rows, cols), _t(I, np.int32), _t(J, np.int32), return_src=True, return_info=True, **kw)
    want = ref.extract(A[0], A[1], A[2], rows, cols, I, J)
    assert (c.rows, c.cols) == (rows if I is None else len(I), cols if J is None else len(J))
    _same(c, want, src, A, J)
    assert info["nnz_a"] == len(A[1]) and info["nnz_c"] == len(want[1]) and info["unit_entries"] == 64
    assert info["j_kind"] == (0 if J is None else (1 if np.all(np.diff(np.asarray(J, np.int64)) >= 0) else 2))
    assert info["rows_in_order"] + info["rows_sorted_wave"] + info["rows_sorted_lds"] + info["rows_sorted_radix"] == c.rows
    return info


# ------------------------------------------------------------------------------------------------ 1. unit edges × every kind of I and J
UNIT_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 0, 200]
COLS = 256


def _j_variants(rng):
    return {"null": None, "identity": np.arange(COLS), "subset": np.sort(rng.choice(COLS, 100, replace=False)),
            "ascending_repeats": np.sort(rng.integers(0, COLS, 400)), "reversed": np.arange(COLS)[::-1].copy(), "permutation": rng.permutation(COLS),
            "random_repeats": rng.integers(0, COLS, 400)}


def _i_variants(rng):
    return {"null": None, "permutation": rng.permutation(12), "repeats": rng.integers(0, 12, 30), "none": np.zeros(0, np.int64)}


@pytest.mark.parametrize("jname", ["null", "identity", "subset", "ascending_repeats", "reversed", "permutation", "random_repeats"])
def test_unit_edges(jname):
    A = _rows_of(UNIT_LENGTHS, COLS, 1)
    rng = np.random.default_rng(2)
    J = _j_variants(rng)[jname]
    for iname, I in _i_variants(rng).items():
        info = _check(A, 12, COLS, I, J)
        ni = 12 if I is None else len(I)
        lens = np.diff(A[0])[np.arange(12) if I is None else I]
        assert info["nnz_rows"] == lens.sum() and info["units"] == np.sum((lens + 63) // 64), iname
        if jname in ("null", "identity", "subset", "ascending_repeats"):
            assert info["rows_in_order"] == ni and info["host_waits"] == 2, iname   # canonical A, J never decreases: nothing is sorted


def test_no_columns_and_no_rows():
    A = _rows_of(UNIT_LENGTHS, COLS, 1)
    for I in (None, np.array([11, 3])):
        info = _check(A, 12, COLS, I, np.zeros(0, np.int64))
        assert info["nnz_c"] == 0
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    _check(empty, 0, 7, None, np.array([3, 3, 0]))
    _check(empty, 0, 0, None, None)
    _check((np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)), 5, 4, np.array([4, 4, 0]), np.array([1, 0]))


# ------------------------------------------------------------------------------------------------ 2. the sort classes at their thresholds
def _lds_sort_max():
    return _check(_rows_of([3], 8, 0), 1, 8, None, None)["lds_sort_max"]


def _one_row_of(length, seed):
    """A: row 0 holds k = min(length, 70) columns, row 1 none. J: a shuffled list of `length` ids over those k columns, each at least once — output row 0 has
    exactly `length` entries and comes out of the fill unordered."""
    rng = np.random.default_rng(seed)
    k = min(length, 70)
    A = _rows_of([k, 0], 100, seed)
    J = np.concatenate([A[1], rng.choice(A[1], length - k)])
    for _ in range(8):
        J = rng.permutation(J)
        if np.any(np.diff(J) < 0):
            break
    return A, J


def test_sort_class_edges():
    lmax = _lds_sort_max()
    assert 64 < lmax <= 1 << 16
    for length, cls in ((64, "rows_sorted_wave"), (65, "rows_sorted_lds"), (lmax, "rows_sorted_lds"), (lmax + 1, "rows_sorted_radix")):
        A, J = _one_row_of(length, length)
        info = _check(A, 2, 100, None, J)
        assert info["nnz_c"] == length and info["j_kind"] == 2
        for name in ("rows_sorted_wave", "rows_sorted_lds", "rows_sorted_radix"):
            assert info[name] == (1 if name == cls else 0), (length, name, info)
        assert info["rows_in_order"] == 1                               # the empty row
        assert info["host_waits"] == 3 if cls != "rows_sorted_radix" else info["host_waits"] >= 4


def test_all_three_classes_in_one_call():
    lmax = _lds_sort_max()
    rng = np.random.default_rng(5)
    J = rng.permutation(np.concatenate([np.full(30, 0), np.full(30, 3), np.full(lmax - 100, 1), np.full(lmax + 200, 2)]))
    first, last = [int(np.flatnonzero(J == c)[0]) for c in range(4)], [int(np.flatnonzero(J == c)[-1]) for c in range(4)]
    assert first[3] < last[0] and first[1] < last[0] and first[2] < last[1]   # the q's of the columns interleave: every row below leaves the fill unordered
    rp = np.array([0, 2, 4, 7, 7, 8], np.int32)
    ci = np.array([0, 3, 0, 1, 0, 1, 2, 4], np.int32)                 # rows of 60, lmax − 70 and 2·lmax + 130 entries, an empty one, one that J does not name
    A = (rp, ci, rng.permutation(8).astype(np.float64) + 1.0)
    info = _check(A, 5, 5, np.array([2, 4, 1, 0, 3, 2]), J)
    assert (info["rows_sorted_wave"], info["rows_sorted_lds"], info["rows_sorted_radix"], info["rows_in_order"]) == (1, 1, 2, 2)


def test_canonical_input_sorts_nothing():
    A = _rows_of([40, 0, 90, 300, 7], 512, 6)
    rng = np.random.default_rng(6)
    for J in (None, np.sort(rng.integers(0, 512, 2000))):
        info = _check(A, 5, 512, np.array([3, 3, 0, 4, 1, 2]), J)
        assert (info["rows_in_order"], info["rows_sorted_wave"], info["rows_sorted_lds"], info["rows_sorted_radix"], info["host_waits"]) == (6, 0, 0, 0, 2)


# ------------------------------------------------------------------------------------------------ 3. multiplicity hub, non-canonical rows
def test_multiplicity_hub():
    A = _rows_of([20, 5, 0, 33], 64, 7)
    hub = int(A[1][3])
    info = _check(A, 4, 64, None, np.full(5000, hub))
    assert info["j_kind"] == 1 and info["nnz_c"] == 5000 * int(np.sum(A[1] == hub)) and info["rows_in_order"] == 4


@pytest.mark.parametrize("jname", ["null", "ascending_repeats", "permutation", "random_repeats"])
def test_non_canonical_rows(jname):
    rng = np.random.default_rng(8)
    lengths = [0, 9, 70, 130, 33]
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = rng.integers(0, 24, rp[-1]).astype(np.int32)                 # 24 columns: every longer row repeats columns, in no order
    A = (rp, ci, rng.permutation(ci.size).astype(np.float64) + 1.0)
    J = {"null": None, "ascending_repeats": np.sort(rng.integers(0, 24, 50)), "permutation": rng.permutation(24), "random_repeats": rng.integers(0, 24, 50)}[jname]
    info = _check(A, 5, 24, np.array([3, 1, 2, 2, 0, 4]), J)
    assert info["rows_in_order"] < 6                                     # unordered source rows are sorted, ties by stored position


# ------------------------------------------------------------------------------------------------ 4. the raw C ABI
def _raw(A, rows, cols, I, J, stream=None, **kw):
    """Both calls through ctypes, on `stream` (torch's own work — uploads, guard fills, copies back — goes on the same stream) or on the current one. Returns
    (status of symbolic, status of numeric, crpt, ccol, cval, src, cnnz); arrays as numpy, guards where unwritten."""
    if stream is None:
        return _raw_on_current(A, rows, cols, I, J, **kw)
    with torch.cuda.stream(stream):
        return _raw_on_current(A, rows, cols, I, J, **kw)


def _raw_on_current(A, rows, cols, I, J, pattern=False, want_src=True, device=True, crpt=None, symbolic_only=False):
    capi, _ = _mods()
    lib = capi.load()
    ni, nj = (rows if I is None else len(I)), (cols if J is None else len(J))
    sp_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cnnz, info = C.c_int64(-5), capi.ExtractInfo()
    if device:
        rp, ci, va, ti, tj = _t(A[0], np.int32), _t(A[1], np.int32), _t(A[2], np.float64), _t(I, np.int32), _t(J, np.int32)
        crp = torch.full((ni + 1,), GUARD_I, dtype=torch.int32, device="cuda")
        P, flags = _Q, capi.DEVICE_POINTERS
    else:
        cast = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        rp, ci, va, ti, tj = cast(A[0], np.int32), cast(A[1], np.int32), cast(A[2], np.float64), cast(I, np.int32), cast(J, np.int32)
        crp = np.full(ni + 1, GUARD_I, np.int32)
        spare = np.zeros(4, np.float64)
        P, flags = (lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)), capi.HOST_POINTERS
    st1 = lib.g4s_csr_extract_symbolic(rows, cols, P(rp), P(ci), ni, P(ti), nj, P(tj), P(crp), C.byref(cnnz), flags, C.byref(info), sp_)
    host_of = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    if st1 != 0 or symbolic_only:
        return st1, None, host_of(crp), None, None, None, cnnz.value
    n = cnnz.value
    if crpt is not None:
        crp = _t(crpt, np.int32) if device else np.ascontiguousarray(crpt, np.int32)
    if device:
        cci, cva = torch.full((n,), GUARD_I, dtype=torch.int32, device="cuda"), torch.full((n,), GUARD_D, dtype=torch.float64, device="cuda")
        src = torch.full((n,), GUARD_I, dtype=torch.int32, device="cuda") if want_src else None
    else:
        cci, cva, src = np.full(n, GUARD_I, np.int32), np.full(n, GUARD_D, np.float64), (np.full(n, GUARD_I, np.int32) if want_src else None)
    st2 = lib.g4s_csr_extract_numeric(rows, cols, P(rp), P(ci), C.c_void_p(0) if pattern else P(va), ni, P(ti), nj, P(tj), P(crp), P(cci),
                                      C.c_void_p(0) if pattern else P(cva), P(src), flags, C.byref(info), sp_)
    return st1, st2, host_of(crp), host_of(cci), host_of(cva), (None if src is None else host_of(src)), n


def _exact(out, want, pattern=False):
    st1, st2, crp, cci, cva, src, n = out
    assert st1 == 0 and st2 == 0 and n == len(want[1])
    assert np.array_equal(crp, want[0]) and np.array_equal(cci, want[1])
    assert np.all(cva == GUARD_D) if pattern else np.array_equal(_bits(cva), _bits(want[2]))
    assert src is None or np.array_equal(src, want[3])


@pytest.fixture(scope="module")
def case():
    """one matrix and one pair of lists for the ABI tests: 40 × 60, rows of 0 … 150 entries in no order, lists with repeats; the reference computed once"""
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 60, 40)
    lengths[[3, 17]] = 0
    A = _rows_of(lengths.tolist(), 60, 9, canonical=False)
    I, J = rng.integers(0, 40, 55), rng.integers(0, 60, 150)
    return A, I, J, ref.extract(A[0], A[1], A[2], 40, 60, I, J)


def test_src_pattern_only_and_host_pointers(case):
    A, I, J, want = case
    _exact(_raw(A, 40, 60, I, J), want)
    assert np.array_equal(_bits(A[2][want[3]]), _bits(want[2])) and np.array_equal(A[1][want[3]], J[want[1]])
    _exact(_raw(A, 40, 60, I, J, want_src=False), want)
    _exact(_raw(A, 40, 60, I, J, pattern=True), want, pattern=True)       # the same crpt and ccol, no value touched
    _exact(_raw(A, 40, 60, I, J, device=False), want)
    _exact(_raw(A, 40, 60, I, J, device=False, pattern=True, want_src=False), want, pattern=True)
    _exact(_raw(A, 40, 60, None, None, device=False), ref.extract(A[0], A[1], A[2], 40, 60))


def test_twice_on_two_streams_the_same_bits(case):
    A, I, J, want = case
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = _raw(A, 40, 60, I, J, stream=s1), _raw(A, 40, 60, I, J, stream=s2)
    _exact(a, want)
    _exact(b, want)
    for x, y in zip(a[2:6], b[2:6]):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)


def test_refusals_on_the_device_each_followed_by_an_exact_call(case):
    capi, _ = _mods()
    lib = capi.load()
    A, I, J, want = case
    INVALID = capi.ERR_INVALID

    def bad_i():
        i2 = I.copy()
        i2[7] = 40
        return _raw(A, 40, 60, i2, J)
    def bad_j():
        j2 = J.copy()
        j2[-1] = -1
        return _raw(A, 40, 60, I, j2)
    def bad_rowptr():
        rp = A[0].copy()
        rp[20] = rp[19] - 1 if rp[19] > 0 else rp[21] + 1
        assert np.any(np.diff(rp) < 0)
        return _raw((rp, A[1], A[2]), 40, 60, I, J)
    def bad_column():
        ci = A[1].copy()
        ci[A[0][next(r for r in I if A[0][r + 1] > A[0][r])]] = 60          # the first entry of a row that I does select
        return _raw((A[0], ci, A[2]), 40, 60, I, J)
    for call, word in ((bad_i, "id of I or J"), (bad_j, "id of I or J"), (bad_rowptr, "rpt"), (bad_column, "column id of A")):
        out = call()
        assert out[0] == INVALID and out[1] is None and word in lib.g4s_last_error().decode(), call.__name__
        _exact(_raw(A, 40, 60, I, J), want)
    for k in (0, 11, len(want[0]) - 2, len(want[0]) - 1):                 # one element of crpt altered: the first, inner ones, the last
        crp = want[0].copy()
        crp[k] += 1
        if k == len(crp) - 1:
            crp[k] -= 2                                                   # (the outputs hold crpt[ni] entries: never claim more than were allocated)
        out = _raw(A, 40, 60, I, J, crpt=crp)
        assert out[0] == 0 and out[1] == INVALID and "crpt" in lib.g4s_last_error().decode(), k
        _exact(_raw(A, 40, 60, I, J), want)


def test_a_capturing_stream_is_refused(case):
    capi, _ = _mods()
    lib = capi.load()
    A, I, J, want = case
    rp, ci, va, ti, tj, tcrp = _t(A[0], np.int32), _t(A[1], np.int32), _t(A[2], np.float64), _t(I, np.int32), _t(J, np.int32), _t(want[0], np.int32)
    n = len(want[1])
    crp = torch.full((len(I) + 1,), GUARD_I, dtype=torch.int32, device="cuda")
    cci, cva = torch.full((n,), GUARD_I, dtype=torch.int32, device="cuda"), torch.full((n,), GUARD_D, dtype=torch.float64, device="cuda")
    cnnz, info = C.c_int64(-5), capi.ExtractInfo()
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        sp_ = C.c_void_p(stream.cuda_stream)
        st1 = lib.g4s_csr_extract_symbolic(40, 60, _Q(rp), _Q(ci), len(I), _Q(ti), len(J), _Q(tj), _Q(crp), C.byref(cnnz), capi.DEVICE_POINTERS, C.byref(info), sp_)
        e1 = lib.g4s_last_error().decode()
        st2 = lib.g4s_csr_extract_numeric(40, 60, _Q(rp), _Q(ci), _Q(va), len(I), _Q(ti), len(J), _Q(tj), _Q(tcrp), _Q(cci), _Q(cva), None, capi.DEVICE_POINTERS,
                                          C.byref(info), sp_)
        g.capture_end()
    assert st1 == st2 == capi.ERR_INVALID and "captur" in e1 and "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(crp == GUARD_I) and torch.all(cci == GUARD_I) and torch.all(cva == GUARD_D) and cnnz.value == -5   # the graph holds nothing of the two calls
    _exact(_raw(A, 40, 60, I, J), want)


def test_more_than_int32_entries_overflow():
    capi, _ = _mods()
    n = 32769                                                             # 65 536 copies of a row of 32 769 entries: 2^31 + 65 536
    A = (np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    free = torch.cuda.mem_get_info()[0]                                  # the device's own figure: it sees the library's allocator too
    out = _raw(A, 1, n, np.zeros(65536, np.int32), None, symbolic_only=True)
    assert out[0] == capi.ERR_OVERFLOW and "exceed" in capi.load().g4s_last_error().decode()
    assert out[6] == 65536 * n > 2**31 - 1
    assert free - torch.cuda.mem_get_info()[0] < 4 << 30                 # the ids of 2^31 entries alone would be 8 GiB: nothing of that size was allocated
    _check(_rows_of([5, 2], 9, 0), 2, 9, np.array([1, 0, 1]), None)


# ------------------------------------------------------------------------------------------------ 5. compositions
def _rmat_like(n, m, seed):
    """a square canonical pattern with skewed degrees: m draws, both ends squared towards 0, repeats merged"""
    rng = np.random.default_rng(seed)
    r, c = (rng.random(m) ** 2 * n).astype(np.int64), (rng.random(m) ** 2 * n).astype(np.int64)
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp).astype(np.int32), c.astype(np.int32), rng.permutation(key.size).astype(np.float64) + 1.0


def test_permute_and_back():
    _, host = _mods()
    A = _rmat_like(200, 3000, 10)
    a = _csr(A, 200, 200)
    p = np.random.default_rng(10).permutation(200)
    b = a.permute(_t(p, np.int32))
    _same(b, ref.extract(A[0], A[1], A[2], 200, 200, p, p))
    back = host.csr_permute(b, _t(np.argsort(p), np.int32))
    _same(back, (A[0], A[1], A[2]))


def test_submatrix_against_slicing():
    import scipy.sparse as sp
    A = _rmat_like(120, 2500, 11)
    a = _csr(A, 120, 120)
    m = sp.csr_matrix((A[2], A[1], A[0]), shape=(120, 120))
    for M, N, r0, c0 in ((50, 70, 0, 0), (33, 21, 60, 17), (120, 120, 0, 0), (0, 5, 3, 3), (7, 0, 100, 120)):
        want = m[r0:r0 + M, c0:c0 + N].tocsr()
        want.sort_indices()
        c = a.submatrix(M, N, r0, c0)
        assert (c.rows, c.cols) == (M, N)
        _same(c, (want.indptr, want.indices, want.data))


def test_induced_subgraph_by_mask_and_by_ids():
    A = _rmat_like(150, 2500, 12)
    a = _csr(A, 150, 150)
    rng = np.random.default_rng(12)
    mask = rng.random(150) < 0.5
    sub, ids = a.induced_subgraph(torch.from_numpy(mask).cuda())
    assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), np.flatnonzero(mask))
    _same(sub, ref.extract(A[0], A[1], A[2], 150, 150, np.flatnonzero(mask), np.flatnonzero(mask)))
    order = rng.permutation(np.flatnonzero(mask))                          # ids are used in the order given
    sub2, ids2 = a.induced_subgraph(_t(order, np.int32))
    assert np.array_equal(ids2.cpu().numpy(), order)
    _same(sub2, ref.extract(A[0], A[1], A[2], 150, 150, order, order))


def test_the_largest_component_extracted_is_one_component():
    _, host = _mods()
    rng = np.random.default_rng(13)
    n, big = 90, 60                                                       # a ring of 60 and a ring of 30 vertices, numbered at random
    name = rng.permutation(n)
    edges = [(name[i], name[(i + 1) % big]) for i in range(big)] + [(name[big + i], name[big + (i + 1) % (n - big)]) for i in range(n - big)]
    r = np.array([e[0] for e in edges] + [e[1] for e in edges], np.int32)
    c = np.array([e[1] for e in edges] + [e[0] for e in edges], np.int32)
    a = host.CSR.from_coo(_t(r, np.int32), _t(c, np.int32), rows=n, cols=n)
    labels, info = a.connected_components(symmetric=True, return_info=True)
    assert info["components"] == 2 and info["largest"] == big
    sub, ids = a.induced_subgraph(labels == info["largest_label"])
    assert sub.rows == big and sub.nnz == 2 * big and set(ids.cpu().numpy().tolist()) == set(name[:big].tolist())
    sub_labels, sub_info = sub.connected_components(symmetric=True, return_info=True)
    assert sub_info["components"] == 1 and torch.all(sub_labels == 0)


def test_against_the_two_spgemm_route():
    """P_I · A · P_Jᵀ with selection matrices from csr_from_coo: the only device route before this call. I and J have no repeats, so every entry of the
    product is one value of A times 1.0 times 1.0 — the same bits."""
    _, host = _mods()
    A = _rmat_like(300, 6000, 14)
    a = _csr(A, 300, 300)
    rng = np.random.default_rng(14)
    I, J = rng.permutation(300)[:180], rng.permutation(300)[:220]
    ti, tj = _t(I, np.int32), _t(J, np.int32)
    pi = host.CSR.from_coo(torch.arange(180, dtype=torch.int32, device="cuda"), ti, rows=180, cols=300)       # P_I(p, I[p]) = 1
    pjt = host.CSR.from_coo(tj, torch.arange(220, dtype=torch.int32, device="cuda"), rows=300, cols=220)      # P_Jᵀ(J[q], q) = 1
    algebraic = host.HashSpGEMM(host.HashSpGEMM(pi, a), pjt)
    c = host.csr_extract(a, ti, tj)
    assert torch.equal(c.rowptr, algebraic.rowptr) and torch.equal(c.colids, algebraic.colids)
    assert torch.equal(c.values.view(torch.int64), algebraic.values.view(torch.int64))
    _same(c, ref.extract(A[0], A[1], A[2], 300, 300, I, J))
