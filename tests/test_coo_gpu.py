"""g4s_csr_from_coo_symbolic / _numeric and g4s_csr_row_indices on the device. Every comparison is ==, values through .view(int64), against the numpy
reference of tests/coo_ref.py (pinned to scipy and to a plain dictionary in test_coo_cpu.py). Shapes that depend on the tile size read it from
info.tile_entries. Every output carries one guard element behind its end: nothing is written there."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import coo_ref as ref
from tests import helpers
from tests import traverse_ref

pytestmark = pytest.mark.gpu

INVALID = -1
INT32_MIN = -(1 << 31)
GUARD_I, GUARD_D = -9, -9.0


def _lib():
    from g4s_amd import capi
    return capi.load()


def _P(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _Q(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dup(name):
    from g4s_amd import host
    return host.DUPLICATES[name]


def _info(info):
    from g4s_amd import capi
    return {k: getattr(info, k) for k, _ in capi.CooInfo._fields_ if k != "reserved"}


def _symbolic(row, col, rows, cols, dup, device=True, stream=None):
    """(status, crp, perm, cnnz, info) — numpy arrays whatever `device` is; the guard elements are checked here."""
    from g4s_amd import capi
    lib, n = _lib(), len(row)
    info, cnnz = capi.CooInfo(), C.c_int64(-5)
    sp_ = C.c_void_p(stream.cuda_stream) if stream is not None else None
    row, col = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)
    if device:
        tr, tc = torch.from_numpy(row).cuda(), torch.from_numpy(col).cuda()
        crp = torch.full((rows + 2,), GUARD_I, dtype=torch.int32, device="cuda")
        perm = torch.full((n + 1,), GUARD_I, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        st = lib.g4s_csr_from_coo_symbolic(_dup(dup), rows, cols, n, _Q(tr), _Q(tc), _Q(crp), _Q(perm), C.byref(cnnz), capi.DEVICE_POINTERS, C.byref(info), sp_)
        crp, perm = crp.cpu().numpy(), perm.cpu().numpy()
    else:
        crp, perm = np.full(rows + 2, GUARD_I, np.int32), np.full(n + 1, GUARD_I, np.int32)
        st = lib.g4s_csr_from_coo_symbolic(_dup(dup), rows, cols, n, _P(row), _P(col), _P(crp), _P(perm), C.byref(cnnz), capi.HOST_POINTERS, C.byref(info), sp_)
    assert crp[-1] == GUARD_I and perm[-1] == GUARD_I
    return st, crp[:-1], perm[:-1], cnnz.value, _info(info)


def _numeric(row, col, val, rows, cols, dup, crp, perm, size, device=True, stream=None):
    """(status, cci, cva-or-None): outputs of `size` entries and a guard each."""
    from g4s_amd import capi
    lib, n = _lib(), len(row)
    sp_ = C.c_void_p(stream.cuda_stream) if stream is not None else None
    row, col = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32)
    val = None if val is None else np.ascontiguousarray(val, np.float64)
    crp, perm = np.ascontiguousarray(crp, np.int32), np.append(perm, 0).astype(np.int32)   # (one element more: an empty perm is still an array)
    if device:
        t = lambda a: None if a is None else torch.from_numpy(np.append(a, a.dtype.type(0))).cuda()      # (an empty list is still three arrays)
        tr, tc, tv, tcrp, tperm = t(row), t(col), t(val), t(crp), t(perm)
        cci = torch.full((size + 1,), GUARD_I, dtype=torch.int32, device="cuda")
        cva = None if val is None else torch.full((size + 1,), GUARD_D, dtype=torch.float64, device="cuda")
        torch.cuda.current_stream().synchronize()
        st = lib.g4s_csr_from_coo_numeric(_dup(dup), rows, cols, n, _Q(tr), _Q(tc), _Q(tv), _Q(tcrp), _Q(tperm), _Q(cci), _Q(cva), capi.DEVICE_POINTERS, sp_)
        cci, cva = cci.cpu().numpy(), None if cva is None else cva.cpu().numpy()
    else:
        cci = np.full(size + 1, GUARD_I, np.int32)
        cva = None if val is None else np.full(size + 1, GUARD_D, np.float64)
        st = lib.g4s_csr_from_coo_numeric(_dup(dup), rows, cols, n, _P(row), _P(col), _P(val), _P(crp), _P(perm), _P(cci), _P(cva), capi.HOST_POINTERS, sp_)
    assert cci[-1] == GUARD_I and (cva is None or cva[-1] == GUARD_D)      # nothing written behind cnnz
    return st, cci[:-1], None if cva is None else cva[:-1]


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    if got[2] is not None:
        assert np.array_equal(got[2].view(np.int64), np.asarray(want[2], np.float64).view(np.int64)), what


def _check(row, col, val, rows, cols, dup, want=None, device=True, pattern=False, stream=None):
    """Both calls against the reference (want: its result, when the caller shares one); returns the symbolic info."""
    want = want if want is not None else ref.from_coo(row, col, val, rows, cols, dup)
    what = (dup, device, pattern, len(row), rows, cols)
    st, crp, perm, cnnz, info = _symbolic(row, col, rows, cols, dup, device, stream)
    assert st == 0, what
    assert np.array_equal(crp, want[0]) and np.array_equal(perm, want[3]), what
    assert cnnz == len(want[1]) == info["nnz_out"] and info["nnz_in"] == len(row) and info["longest_run"] == want[4], (what, info)
    assert 1 <= info["host_waits"] <= 2
    st, cci, cva = _numeric(row, col, None if pattern else val, rows, cols, dup, crp, perm, cnnz, device, stream)
    assert st == 0, what
    _same((crp, cci, cva), want, what)
    return info


def _check_all_forms(row, col, val, rows, cols, dup):
    want = ref.from_coo(row, col, val, rows, cols, dup)
    info = None
    for device in (True, False):
        for pattern in (False, True):
            info = _check(row, col, val, rows, cols, dup, want, device, pattern)
    return info


def _random(n, rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, rows, n).astype(np.int32), rng.integers(0, cols, n).astype(np.int32), rng.uniform(-1, 1, n)


@functools.lru_cache(maxsize=None)
def _tile():
    _, _, _, _, info = _symbolic([0], [0], 1, 1, "plus")
    assert info["tile_entries"] >= 64 and info["digit_bits"] == 8
    return info["tile_entries"]


# ------------------------------------------------------------------------------------------------ 1. empty and tiny
def test_empty_and_tiny():
    e = np.zeros(0, np.int32)
    for rows in (0, 5):
        for dup in ("keep", "plus"):
            info = _check_all_forms(e, e, np.zeros(0), rows, 3, dup)
            assert info["longest_run"] == 0 and info["nnz_out"] == 0
    for dup in ("keep", "max"):
        _check_all_forms([3], [2], [0.5], 5, 4, dup)
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 1, 300)
    for dup in ref.DUPLICATES:
        info = _check_all_forms(np.zeros(300, np.int32), np.zeros(300, np.int32), v, 1, 1, dup)
        assert info["longest_run"] == 300 and info["sort_passes"] == 0 and info["row_bits"] == info["col_bits"] == 0


# ------------------------------------------------------------------------------------------------ 2. wave, workgroup and tile edges
@pytest.mark.parametrize("which", range(10))
def test_wave_workgroup_and_tile_edges(which):
    T = _tile()
    n = [63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5][which]
    row, col, val = _random(n, 37, 41, n)
    for dup in ("keep", "plus"):
        info = _check_all_forms(row, col, val, 37, 41, dup)
        assert info["presorted"] == 0 and info["sort_passes"] == 2


# ------------------------------------------------------------------------------------------------ 3. digit edges
@pytest.mark.parametrize("size", [255, 256, 257, 65535, 65536, 65537])
@pytest.mark.parametrize("wide", [True, False])
def test_digit_edges(size, wide):
    rng = np.random.default_rng(size)
    n = 2000
    ids = rng.integers(0, size, n).astype(np.int32)
    tops = [t for t in (size - 1, 255, 256, 65535, 65280, 65536, 0) if t < size]      # the top value of every digit occurs, and the first value behind it
    ids[rng.choice(n, len(tops), replace=False)] = tops
    other = rng.integers(0, 3, n).astype(np.int32)
    row, col, rows, cols = (other, ids, 3, size) if wide else (ids, other, size, 3)
    val = rng.uniform(-1, 1, n)
    for dup in ("keep", "plus"):
        info = _check_all_forms(row, col, val, rows, cols, dup)
        assert info["row_bits"] == (rows - 1).bit_length() and info["col_bits"] == (cols - 1).bit_length() and info["digit_bits"] == 8
        assert info["sort_passes"] == -(-(info["row_bits"] + info["col_bits"]) // info["digit_bits"])


# ------------------------------------------------------------------------------------------------ 4. row-pointer gaps
def test_row_pointer_gaps():
    T = _tile()
    rng = np.random.default_rng(4)
    rows, cols = 1000, 50
    live = np.concatenate([np.arange(5, 40), np.arange(400, 420), np.arange(900, 960)])   # empty at the start, a gap of 360 rows, empty at the end
    row = rng.choice(live, 3000).astype(np.int32)
    col, val = rng.integers(0, cols, 3000).astype(np.int32), rng.uniform(-1, 1, 3000)
    for dup in ("keep", "min"):
        _check_all_forms(row, col, val, rows, cols, dup)
    for r, n in ((rows - 1, 500), (0, 3 * T)):                          # all in the last row; a hub of 3T entries in row 0
        row = np.full(n, r, np.int32)
        col, val = rng.integers(0, cols, n).astype(np.int32), rng.uniform(-1, 1, n)
        for dup in ("keep", "plus"):
            _check_all_forms(row, col, val, rows, cols, dup)


# ------------------------------------------------------------------------------------------------ 5. stability
def test_stability():
    rng = np.random.default_rng(5)
    n = 1000
    row, col = rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32)
    val = rng.permutation(n).astype(np.float64)                         # distinct: a value names its triple
    for device in (True, False):
        st, crp, perm, cnnz, _ = _symbolic(row, col, 4, 4, "keep", device)
        assert st == 0 and cnnz == n and np.array_equal(perm, np.lexsort((np.arange(n), col, row)))
        st, cci, cva = _numeric(row, col, val, 4, 4, "keep", crp, perm, n, device)
        assert st == 0
        for r in range(4):
            for c in range(4):
                mine = cva[crp[r]:crp[r + 1]][cci[crp[r]:crp[r + 1]] == c]
                assert np.array_equal(mine, val[(row == r) & (col == c)])      # input order within a position
        for dup, pick in (("first", 0), ("second", -1)):
            st, crp2, perm2, cnnz2, _ = _symbolic(row, col, 4, 4, dup, device)
            assert st == 0 and cnnz2 == 16 and np.array_equal(perm2, perm)
            st, cci2, cva2 = _numeric(row, col, val, 4, 4, dup, crp2, perm2, 16, device)
            assert st == 0
            want = [val[(row == r) & (col == c)][pick] for r in range(4) for c in range(4)]
            assert cva2.tolist() == want and cci2.tolist() == list(range(4)) * 4


# ------------------------------------------------------------------------------------------------ 6. fold order
def test_fold_order():
    T = _tile()
    rng = np.random.default_rng(6)
    rows, cols = 30, 30
    n = 3 * T + 600
    others = np.stack([rng.integers(0, rows, n), rng.integers(0, cols, n)])
    others[:, (others[0] == 7) & (others[1] == 11)] = 0                  # position (7, 11) belongs to the four triples below
    at = [3, T + 50, 2 * T + 100, 3 * T + 400]                           # more than T input positions apart
    for dup, four in (("plus", [1e16, 1.0, -1e16, 1.0]), ("times", [1e200, 1e-200, 1e-200, 1e200])):
        row, col = others[0].astype(np.int32), others[1].astype(np.int32)
        val = rng.integers(1, 4, n).astype(np.float64)
        row[at], col[at], val[at] = 7, 11, four
        want = ref.fold(dup, four)
        assert want != ref.fold(dup, sorted(four)) and want != ref.fold(dup, four[::-1] if dup == "plus" else [four[1], four[2], four[0], four[3]])
        assert dup != "plus" or want == 1.0
        w = ref.from_coo(row, col, val, rows, cols, dup)
        for device in (True, False):
            _check(row, col, val, rows, cols, dup, w, device)
        got = w[2][w[0][7]:w[0][8]][w[1][w[0][7]:w[0][8]] == 11]
        assert got.view(np.int64).tolist() == np.array([want]).view(np.int64).tolist()


# ------------------------------------------------------------------------------------------------ 7. a long run
def test_long_run():
    T = _tile()
    rng = np.random.default_rng(7)
    L, rows, cols = 70000, 200, 300
    assert L > 8 * T                                                      # the run spans many tiles in sorted order
    xr, xc = rng.integers(0, rows, 1000), rng.integers(0, cols, 1000)
    xc[(xr == 90) & (xc == 123)] = 124                                  # position (90, 123) belongs to the run alone
    row = np.concatenate([np.full(L, 90), xr]).astype(np.int32)
    col = np.concatenate([np.full(L, 123), xc]).astype(np.int32)
    val = np.concatenate([1.0 / (np.arange(L) + 1.0), rng.uniform(-1, 1, 1000)])
    mix = rng.permutation(L + 1000)
    row, col, val = row[mix], col[mix], val[mix]
    w = ref.from_coo(row, col, val, rows, cols, "plus")
    assert w[4] == L
    for device in (True, False):
        assert _check(row, col, val, rows, cols, "plus", w, device)["longest_run"] == 70000
    at = w[0][90] + int(np.searchsorted(w[1][w[0][90]:w[0][91]], 123))
    assert w[2][at] == ref.fold("plus", val[(row == 90) & (col == 123)].tolist())   # the left fold in input order


# ------------------------------------------------------------------------------------------------ 8. every policy on one skewed list; presorted
@functools.lru_cache(maxsize=None)
def _skewed():
    rng = np.random.default_rng(8)
    n, rows, cols = 200000, 5000, 5000
    hot = np.stack([rng.integers(0, rows, 50), rng.integers(0, cols, 50)])
    pick = rng.integers(0, 50, n // 2)
    row = np.concatenate([hot[0][pick], rng.integers(0, rows, n - n // 2)]).astype(np.int32)
    col = np.concatenate([hot[1][pick], rng.integers(0, cols, n - n // 2)]).astype(np.int32)
    mix = rng.permutation(n)
    val = rng.uniform(0.5, 1.5, n)
    return row[mix], col[mix], val, rows, cols


@pytest.mark.parametrize("dup", ref.DUPLICATES)
def test_every_policy_on_a_skewed_list(dup):
    row, col, val, rows, cols = _skewed()
    w = ref.from_coo(row, col, val, rows, cols, dup)
    info = _check(row, col, val, rows, cols, dup, w)
    assert info["presorted"] == 0 and info["longest_run"] > 1500 and info["sort_passes"] == 4 and info["host_waits"] == 2
    _check(row, col, val, rows, cols, dup, w, device=False, pattern=dup in ("min", "first"))


def test_presorted():
    row, col, val, rows, cols = _skewed()
    p = ref.perm_of(row, col)
    srow, scol, sval = row[p], col[p], val[p]
    for dup in ("keep", "plus"):
        w = ref.from_coo(srow, scol, sval, rows, cols, dup)
        assert np.array_equal(w[3], np.arange(len(row)))
        assert _check(srow, scol, sval, rows, cols, dup, w)["presorted"] == 1
        u = ref.from_coo(row, col, val, rows, cols, dup)                 # the same outputs as from the unsorted list
        assert np.array_equal(u[0], w[0]) and np.array_equal(u[1], w[1]) and np.array_equal(u[2].view(np.int64), w[2].view(np.int64))
    assert _check(srow, scol, sval, rows, cols, "max", device=False)["presorted"] == 1
    n = len(row)
    assert (srow[n - 2], scol[n - 2]) != (srow[n - 1], scol[n - 1])
    for a in (srow, scol, sval):
        a[[n - 2, n - 1]] = a[[n - 1, n - 2]]                              # one swapped pair at the very end
    assert _check(srow, scol, sval, rows, cols, "plus")["presorted"] == 0


# ------------------------------------------------------------------------------------------------ 9. round trip and row indices
def _row_indices(rp, nnz, device=True, stream=None):
    from g4s_amd import capi
    rp = np.ascontiguousarray(rp, np.int32)
    sp_ = C.c_void_p(stream.cuda_stream) if stream is not None else None
    if device:
        t = torch.from_numpy(rp).cuda()
        out = torch.full((nnz + 1,), GUARD_I, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        st = _lib().g4s_csr_row_indices(len(rp) - 1, nnz, _Q(t), _Q(out), capi.DEVICE_POINTERS, sp_)
        out = out.cpu().numpy()
    else:
        out = np.full(nnz + 1, GUARD_I, np.int32)
        st = _lib().g4s_csr_row_indices(len(rp) - 1, nnz, _P(rp), _P(out), capi.HOST_POINTERS, sp_)
    assert out[-1] == GUARD_I
    return st, out[:-1]


def test_round_trip():
    rows, cols = 2000, 1500
    rp, ci, va = helpers.random_csr(rows, cols, 30000 / (rows * cols), 9, empty_rows=(0, 17, 1999))
    nnz = len(ci)
    for device in (True, False):
        st, row = _row_indices(rp, nnz, device)
        assert st == 0 and np.array_equal(row, ref.row_indices(rp))
        mix = np.random.default_rng(10).permutation(nnz)
        w = (rp, ci, va, np.argsort(mix, kind="stable").astype(np.int32), 1)
        _check(row[mix], ci[mix], va[mix], rows, cols, "keep", w, device)


def test_row_indices_alone():
    rp = np.array([0, 0, 0, 70000, 70000, 70003, 70003], np.int32)       # a hub row of more than 65 536 entries between empty rows
    for device in (True, False):
        st, row = _row_indices(rp, 70003, device)
        assert st == 0 and np.array_equal(row, ref.row_indices(rp))
        assert _row_indices(np.zeros(4, np.int32), 0, device)[0] == 0 and _row_indices(np.zeros(1, np.int32), 0, device)[0] == 0
        for bad in ([1, 2, 3], [0, 2, 1, 3], [0, 1, 2], [0, 1, 4], [0, -1, 3]):
            st, row = _row_indices(np.array(bad, np.int32), 3, device)
            assert st == INVALID and "rowptr" in _lib().g4s_last_error().decode()
            assert np.all(row == GUARD_I)                                 # refused before anything was written
        st, row = _row_indices(np.array([0, 1, 3], np.int32), 3, device)
        assert st == 0 and row.tolist() == [0, 1, 1]


# ------------------------------------------------------------------------------------------------ 10. refused calls
def test_refused_symbolic_calls():
    row, col, val = _random(900, 20, 30, 11)
    want = ref.from_coo(row, col, val, 20, 30, "plus")
    for device in (True, False):
        for which, bad in [("row", 20), ("row", -1), ("col", 30), ("col", -1)] + [("row", INT32_MIN), ("col", INT32_MIN)]:
            for at in (0, 450, 899):
                r, c = row.copy(), col.copy()
                (r if which == "row" else c)[at] = bad
                st, _, _, _, _ = _symbolic(r, c, 20, 30, "plus", device)
                assert st == INVALID and "outside" in _lib().g4s_last_error().decode(), (which, bad, at)
                _check(row, col, val, 20, 30, "plus", want, device)      # an exact call behind every refused one, same thread and stream


def test_refused_numeric_calls():
    row, col, val = _random(900, 20, 30, 12)
    for dup in ("plus", "keep"):
        want = ref.from_coo(row, col, val, 20, 30, dup)
        crp, perm, cn = want[0], want[3], len(want[1])
        change = int(np.flatnonzero((row[perm][1:] != row[perm][:-1]) | (col[perm][1:] != col[perm][:-1]))[40])   # the keys at change and change + 1 differ
        for device in (True, False):
            cases = []
            for v in (900, -1, INT32_MIN):
                p = perm.copy()
                p[300] = v
                cases.append((p, crp, "perm element"))
            p = perm.copy()
            p[[change, change + 1]] = p[[change + 1, change]]
            cases.append((p, crp, "stable"))
            for d in (1, -1):
                c = crp.copy()
                c[20] += d
                cases.append((perm, c, "crpt[rows]"))
            for p, c, word in cases:
                size = max(cn, int(c[20]))
                st, cci, cva = _numeric(row, col, val, 20, 30, dup, c, p, size, device)
                assert st == INVALID and word in _lib().g4s_last_error().decode(), (dup, device, word)
                st, cci, cva = _numeric(row, col, val, 20, 30, dup, crp, perm, cn, device)        # exact behind every refusal
                assert st == 0
                _same((crp, cci, cva), want)
            r = row.copy()
            r[int(perm[5])] = 20                                          # an id that went bad after the symbolic call
            assert _numeric(r, col, val, 20, 30, dup, crp, perm, cn, device)[0] == INVALID
    q = ref.perm_of(row, col).copy()
    run = int(np.flatnonzero((row[q][1:] == row[q][:-1]) & (col[q][1:] == col[q][:-1]))[0])
    q[[run, run + 1]] = q[[run + 1, run]]                                 # equal keys, input indices descending: not the stable order
    w = ref.from_coo(row, col, val, 20, 30, "first")
    assert _numeric(row, col, val, 20, 30, "first", w[0], q, len(w[1]))[0] == INVALID


# ------------------------------------------------------------------------------------------------ 11. streams, capture, threads
def test_on_a_stream_of_its_own():
    row, col, val = _random(5000, 300, 200, 13)
    s = torch.cuda.Stream()
    for dup in ("keep", "times"):
        _check(row, col, val, 300, 200, dup, stream=s)
    rp = ref.from_coo(row, col, val, 300, 200, "keep")[0]
    st, out = _row_indices(rp, 5000, stream=s)
    assert st == 0 and np.array_equal(out, ref.row_indices(rp))


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi
    lib = _lib()
    row, col, val = _random(3000, 100, 100, 14)
    w = ref.from_coo(row, col, val, 100, 100, "plus")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    tr, tc, tv, tcrp, tperm = t(row, np.int32), t(col, np.int32), t(val, np.float64), t(w[0], np.int32), t(w[3], np.int32)
    crp = torch.full((101,), GUARD_I, dtype=torch.int32, device="cuda")
    perm = torch.full((3000,), GUARD_I, dtype=torch.int32, device="cuda")
    cci = torch.full((len(w[1]),), GUARD_I, dtype=torch.int32, device="cuda")
    cva = torch.full((len(w[1]),), GUARD_D, dtype=torch.float64, device="cuda")
    rix = torch.full((len(w[1]),), GUARD_I, dtype=torch.int32, device="cuda")
    cnnz, info = C.c_int64(-5), capi.CooInfo()
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        sp_ = C.c_void_p(stream.cuda_stream)
        st1 = lib.g4s_csr_from_coo_symbolic(0, 100, 100, 3000, _Q(tr), _Q(tc), _Q(crp), _Q(perm), C.byref(cnnz), capi.DEVICE_POINTERS, C.byref(info), sp_)
        e1 = lib.g4s_last_error().decode()
        st2 = lib.g4s_csr_from_coo_numeric(0, 100, 100, 3000, _Q(tr), _Q(tc), _Q(tv), _Q(tcrp), _Q(tperm), _Q(cci), _Q(cva), capi.DEVICE_POINTERS, sp_)
        st3 = lib.g4s_csr_row_indices(100, len(w[1]), _Q(tcrp), _Q(rix), capi.DEVICE_POINTERS, sp_)
        g.capture_end()
    assert st1 == st2 == st3 == capi.ERR_INVALID and "captur" in e1 and "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    for out in (crp, perm, cci, rix):
        assert torch.all(out == GUARD_I)                                  # the graph holds nothing of the three calls
    assert torch.all(cva == GUARD_D) and cnnz.value == -5
    _check(row, col, val, 100, 100, "plus", w)                             # and the library still works


def test_two_host_threads():
    jobs = []
    for k in range(2):
        row, col, val = _random(4000 + 700 * k, 150 + k, 90, 15 + k)
        dup = ("plus", "keep")[k]
        jobs.append((row, col, val, 150 + k, 90, dup, ref.from_coo(row, col, val, 150 + k, 90, dup)))
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            row, col, val, rows, cols, dup, want = jobs[k]
            for _ in range(20):
                _check(row, col, val, rows, cols, dup, want, stream=s)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ------------------------------------------------------------------------------------------------ 12. value refresh
def test_value_refresh_on_the_same_perm_and_crpt():
    row, col, val = _random(6000, 80, 70, 17)
    for device in (True, False):
        st, crp, perm, cnnz, _ = _symbolic(row, col, 80, 70, "plus", device)
        assert st == 0
        for seed in (1, 2):
            v = np.random.default_rng(seed).uniform(-3, 3, 6000)
            st, cci, cva = _numeric(row, col, v, 80, 70, "plus", crp, perm, cnnz, device)
            assert st == 0
            _same((crp, cci, cva), ref.from_coo(row, col, v, 80, 70, "plus"))


# ------------------------------------------------------------------------------------------------ 13. downstream
@functools.lru_cache(maxsize=None)
def _undirected():
    rng = np.random.default_rng(18)
    n, m = 3000, 40000
    u, v = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    flip = rng.random(m) < 0.5                                            # both orientations, with repeats (m draws on fewer distinct pairs) and loops
    u[:5000], v[:5000] = u[5000:10000], v[5000:10000]
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    return n, u, v


def test_downstream_ewise_and_triangles():
    from g4s_amd import capi, host
    n, u, v = _undirected()
    tu, tv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    ones = torch.ones(len(u), dtype=torch.float64, device="cuda")
    rp, ci, va, perm, info = host.csr_from_coo(tu, tv, ones, n, n, dup="max", symmetric=True, return_perm=True, return_info=True)
    off = u != v
    cu, cv = np.concatenate([u, v[off]]), np.concatenate([v, u[off]])
    w = ref.from_coo(cu, cv, np.ones(len(cu)), n, n, "max")
    _same((rp.cpu().numpy(), ci.cpu().numpy(), va.cpu().numpy()), w)
    assert np.array_equal(perm.cpu().numpy(), w[3]) and info["nnz_in"] == len(cu) and info["nnz_out"] == len(w[1])
    A = host.csr_select(host.CSR(rp, ci, va, n, n), "offdiag")
    crp = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    cnnz = C.c_int64(0)
    st = capi.load().g4s_csr_ewise_symbolic(capi.EWISE_UNION, n, n, _Q(A.rowptr), _Q(A.colids), _Q(A.rowptr), _Q(A.colids), _Q(crp), C.byref(cnnz),
                                            capi.DEVICE_POINTERS, None, None)
    assert st == 0 and cnnz.value == A.nnz                                # the library's own checker of strictly ascending rows
    S = sp.csr_matrix((np.ones(A.nnz), A.colids.cpu().numpy(), A.rowptr.cpu().numpy()), shape=(n, n))
    assert (S != S.T).nnz == 0 and S.diagonal().sum() == 0
    want = int(round((S @ S @ S).diagonal().sum())) // 6
    assert want > 0 and A.triangle_count() == want


def test_downstream_bfs():
    from g4s_amd import host
    n, u, v = _undirected()
    A = host.CSR.from_coo(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), None, n, n, dup="first", symmetric=True)
    off = u != v
    M = sp.coo_matrix((np.ones(len(u) + int(off.sum())), (np.concatenate([u, v[off]]), np.concatenate([v, u[off]]))), shape=(n, n)).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1.0
    assert np.array_equal(A.rowptr.cpu().numpy(), M.indptr) and np.array_equal(A.colids.cpu().numpy(), M.indices) and bool(torch.all(A.values == 1.0))
    levels, _ = A.bfs([0])
    assert np.array_equal(levels.cpu().numpy(), traverse_ref.bfs(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data, n, [0])[0])
    r, c, x = A.to_coo()
    assert np.array_equal(r.cpu().numpy(), ref.row_indices(M.indptr)) and c is A.colids and x is A.values


def test_canonical():
    from g4s_amd import host
    rng = np.random.default_rng(19)
    rows, cols, n = 400, 300, 9000
    row = np.sort(rng.integers(0, rows, n)).astype(np.int32)              # a CSR whose rows are shuffled inside and repeat columns
    col, val = rng.integers(0, cols, n).astype(np.int32), rng.uniform(-1, 1, n)
    rp = np.searchsorted(row, np.arange(rows + 1)).astype(np.int32)
    a = host.CSR.from_host(rp, col, val, rows, cols)
    for dup in ("plus", "keep", "second"):
        w = ref.from_coo(row, col, val, rows, cols, dup)
        for got in (host.csr_canonical(a, dup), a.canonical(dup)):
            assert (got.rows, got.cols, got.nnz) == (rows, cols, len(w[1]))
            _same(got.to_host(), w, dup)
