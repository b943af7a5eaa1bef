"""g4s_csr_ewise_* and g4s_csr_select_* on the device, and the symmetrise built from them. Every comparison is ==, values through .view(int64),
against the numpy oracle of tests/ewise_ref.py (pinned to scipy in test_ewise_cpu.py). Shapes that depend on the unit size read it from
info.unit_entries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ewise_ref as ref
from tests import helpers

pytestmark = pytest.mark.gpu

INVALID = -1


def _P(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _T(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _ewise(a, b, rows, cols, op, combine="plus", device=True, pattern=False, stream=None, same=False):
    """The two C calls: (status, (crp, cci, cva-or-None) as numpy, info dict). status != 0 comes from the symbolic call unless noted."""
    from g4s_amd import capi, host
    lib = capi.load()
    opv, cv = host.EWISE_OPS[op], host.COMBINERS[combine]
    info, cnnz = capi.EwiseInfo(), C.c_int64(-5)
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
    if device:
        ta = [_T(a[0], np.int32), _T(a[1], np.int32), _T(a[2], np.float64)]
        tb = ta if same else [_T(b[0], np.int32), _T(b[1], np.int32), _T(b[2], np.float64)]
        crp = torch.full((rows + 1,), -9, dtype=torch.int32, device="cuda")
        q = host._ptr_nn
        if stream is not None:
            torch.cuda.current_stream().synchronize()                 # the fills above ran on torch's stream
        st = lib.g4s_csr_ewise_symbolic(opv, rows, cols, q(ta[0]), q(ta[1]), q(tb[0]), q(tb[1]), q(crp), C.byref(cnnz), capi.DEVICE_POINTERS, C.byref(info), sp)
        inf = {k: getattr(info, k) for k, _ in capi.EwiseInfo._fields_}
        if st != 0:
            return st, None, inf
        assert cnnz.value == int(crp[rows].item()) == inf["nnz_c"]
        cci = torch.full((cnnz.value,), -9, dtype=torch.int32, device="cuda")
        cva = None if pattern else torch.full((cnnz.value,), -9.0, dtype=torch.float64, device="cuda")
        null = C.c_void_p(0)
        if stream is not None:
            torch.cuda.current_stream().synchronize()
        st = lib.g4s_csr_ewise_numeric(opv, cv, rows, cols, q(ta[0]), q(ta[1]), null if pattern else q(ta[2]), q(tb[0]), q(tb[1]), null if pattern else q(tb[2]),
                                       q(crp), q(cci), null if pattern else q(cva), capi.DEVICE_POINTERS, sp)
        return st, (crp.cpu().numpy(), cci.cpu().numpy(), None if pattern else cva.cpu().numpy()), inf
    ha = [np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.int32), np.ascontiguousarray(a[2], np.float64)]
    hb = ha if same else [np.ascontiguousarray(b[0], np.int32), np.ascontiguousarray(b[1], np.int32), np.ascontiguousarray(b[2], np.float64)]
    crp = np.full(rows + 1, -9, np.int32)
    st = lib.g4s_csr_ewise_symbolic(opv, rows, cols, _P(ha[0]), _P(ha[1]), _P(hb[0]), _P(hb[1]), _P(crp), C.byref(cnnz), capi.HOST_POINTERS, C.byref(info), sp)
    inf = {k: getattr(info, k) for k, _ in capi.EwiseInfo._fields_}
    if st != 0:
        return st, None, inf
    assert cnnz.value == crp[rows] == inf["nnz_c"]
    cci = np.full(cnnz.value + 1, -9, np.int32)
    cva = None if pattern else np.full(cnnz.value + 1, -9.0, np.float64)
    st = lib.g4s_csr_ewise_numeric(opv, cv, rows, cols, _P(ha[0]), _P(ha[1]), None if pattern else _P(ha[2]), _P(hb[0]), _P(hb[1]), None if pattern else _P(hb[2]),
                                   _P(crp), _P(cci), None if pattern else _P(cva), capi.HOST_POINTERS, sp)
    assert cci[-1] == -9 and (pattern or cva[-1] == -9.0)                 # nothing written behind cnnz
    return st, (crp, cci[:-1], None if pattern else cva[:-1]), inf


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    if got[2] is not None:
        assert np.array_equal(got[2].view(np.int64), np.asarray(want[2], np.float64).view(np.int64)), what


def _check(a, b, rows, cols, op, combine="plus", **kw):
    st, got, info = _ewise(a, b, rows, cols, op, combine, **kw)
    assert st == 0, (op, combine, kw)
    _same(got, ref.ewise(a, a if kw.get("same") else b, rows, cols, op, combine), (op, combine, kw))
    assert info["host_waits"] == 1 and info["nnz_a"] == len(a[1]) and info["nnz_c"] == len(got[1])
    return got, info


@functools.lru_cache(maxsize=None)
def _unit():
    z = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    _, _, info = _ewise(z, z, 1, 1, "union")
    assert info["unit_entries"] >= 2
    return info["unit_entries"]


def _csr(rows_cols, rows, seed=0):
    """rows_cols: {row: ascending column array}; values uniform in (−1, 1) by seed."""
    rp = np.zeros(rows + 1, np.int64)
    for r, c in rows_cols.items():
        rp[r + 1] = len(c)
    rp = np.cumsum(rp)
    ci = np.concatenate([np.asarray(rows_cols[r], np.int64) for r in sorted(rows_cols)] + [np.zeros(0, np.int64)])
    va = np.random.default_rng(seed).uniform(-1, 1, len(ci))
    return rp.astype(np.int32), ci.astype(np.int32), va


# ------------------------------------------------------------------------------------------------ 1. random matrices
@pytest.mark.parametrize("rows,cols", [(500, 500), (3000, 200), (200, 3000)])
def test_random_matrices(rows, cols):
    a = helpers.random_csr(rows, cols, 0.02, 11, empty_rows=(3, 7, 11, 150))
    b = helpers.random_csr(rows, cols, 0.02, 12, empty_rows=(5, 7, 11, 160))
    for op in ref.OPS:
        for device in (True, False):
            for combine in ref.COMBINERS:
                _check(a, b, rows, cols, op, combine, device=device)
            _check(a, b, rows, cols, op, device=device, pattern=True)


# ------------------------------------------------------------------------------------------------ 2. unit boundaries
def _boundary_rows(L, staggered):
    if staggered:
        lb = L // 2
        la = L - lb
        return np.arange(la), np.arange(1, lb + 1)
    la = (L + 1) // 2
    return np.arange(la), np.arange(L - la)


@pytest.mark.parametrize("mult,off", [(1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0)])
def test_unit_boundaries(mult, off):
    T = _unit()
    L = mult * T + off
    rng = np.random.default_rng(L)
    for staggered in (False, True):
        ra, rb = _boundary_rows(L, staggered)
        assert len(ra) + len(rb) == L
        for swap in (False, True):
            for place in (0, 2, 4):
                fa = {r: np.sort(rng.choice(3 * T, 5, replace=False)) for r in range(5)}
                fb = {r: np.sort(rng.choice(3 * T, 7, replace=False)) for r in range(5)}
                fa[place], fb[place] = (rb, ra) if swap else (ra, rb)
                a, b = _csr(fa, 5, 1), _csr(fb, 5, 2)
                for op in ref.OPS:
                    _, info = _check(a, b, 5, 3 * T, op, "plus")
                    assert info["rows_split"] == (1 if L > T else 0), (L, info)
                _check(a, b, 5, 3 * T, "union", "second", device=False)


# ------------------------------------------------------------------------------------------------ 3. hub rows, 8. determinism
@functools.lru_cache(maxsize=None)
def _hub_case():
    rows, cols = 301, 100000
    rng = np.random.default_rng(5)
    hub_a = np.sort(rng.choice(cols, 40000, replace=False))
    rest = np.setdiff1d(np.arange(cols), hub_a)
    hub_b = np.sort(np.concatenate([rng.choice(hub_a, 17500, replace=False), rng.choice(rest, 17500, replace=False)]))
    fa = {r: np.sort(rng.choice(cols, rng.integers(0, 12), replace=False)) for r in range(rows)}
    fb = {r: np.sort(rng.choice(cols, rng.integers(0, 12), replace=False)) for r in range(rows)}
    fa[150], fb[150] = hub_a, hub_b
    fa[10], fb[10] = hub_b, np.zeros(0, np.int64)                     # a hub against an empty row, both ways
    fa[20], fb[20] = np.zeros(0, np.int64), hub_a
    return _csr(fa, rows, 3), _csr(fb, rows, 4), rows, cols


def test_hub_rows_and_determinism():
    a, b, rows, cols = _hub_case()
    for op in ref.OPS:
        for kw in (dict(combine="plus"), dict(combine="min"), dict(pattern=True), dict(combine="times", device=False)):
            got, info = _check(a, b, rows, cols, op, **kw)
            assert info["rows_split"] >= 3 and info["units"] >= 75000 // info["unit_entries"], info
            again, info2 = _check(a, b, rows, cols, op, **kw)
            _same(again, got)
            assert info2 == info


# ------------------------------------------------------------------------------------------------ 4. degenerate cases
def test_degenerate_cases():
    rows, cols = 40, 300
    rng = np.random.default_rng(9)
    ev = _csr({r: np.sort(rng.choice(cols // 2, 20, replace=False)) * 2 for r in range(rows)}, rows, 1)
    od = _csr({r: np.sort(rng.choice(cols // 2, 20, replace=False)) * 2 + 1 for r in range(rows)}, rows, 2)
    none = (np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    for device in (True, False):
        for op in ref.OPS:
            got, _ = _check(ev, od, rows, cols, op, device=device)        # disjoint patterns
            assert len(got[1]) == {"union": 1600, "intersect": 0, "difference": 800}[op]
            got, _ = _check(ev, ev, rows, cols, op, "times", device=device, same=True)   # B = A through the same arrays
            assert len(got[1]) == (0 if op == "difference" else 800)
            _check(ev, none, rows, cols, op, device=device)               # an empty B
            _check(none, ev, rows, cols, op, device=device)
            _check(none, none, rows, cols, op, device=device)
            _check(none, none, rows, 0, op, device=device)                # cols == 0
            z = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
            _check(z, z, 0, cols, op, device=device)                      # rows == 0
            _check(z, z, 0, 0, op, device=device)


def test_widest_matrix():
    cols = 2 ** 31 - 1
    a = _csr({0: [0, 5, cols - 1], 1: [cols - 1], 2: [0], 3: [0, cols - 2, cols - 1]}, 4, 1)
    b = _csr({0: [0, cols - 1], 1: [0, cols - 1], 3: [1, cols - 2]}, 4, 2)
    for op in ref.OPS:
        for device in (True, False):
            _check(a, b, 4, cols, op, "max", device=device)


# ------------------------------------------------------------------------------------------------ 5. contract violations
def _violation_base():
    T = _unit()
    rows, cols = 6, 10 * T
    rng = np.random.default_rng(21)
    fa = {r: np.sort(rng.choice(cols, 9, replace=False)) for r in range(rows)}
    fb = {r: np.sort(rng.choice(cols, 6, replace=False)) for r in range(rows)}
    fa[2] = np.arange(3 * T) * 2                                       # the hub row: B's row 2 is empty, so merged position p is A's entry p
    fb[2] = np.zeros(0, np.int64)
    fa[5] = np.arange(10) * 3 + 1
    fb[5] = np.zeros(0, np.int64)
    return fa, fb, rows, cols, T


@pytest.mark.parametrize("kind", ["descending", "repeated", "id_equals_cols"])
@pytest.mark.parametrize("where", ["last_row", "hub_second_unit"])
@pytest.mark.parametrize("side", ["A", "B"])
def test_contract_violations_in_the_entries(kind, where, side):
    fa, fb, rows, cols, T = _violation_base()
    good_a, good_b = _csr(fa, rows, 1), _csr(fb, rows, 2)
    row = 5 if where == "last_row" else 2
    bad = {r: np.array(c, np.int64) for r, c in fa.items()}
    i = len(bad[row]) - 2 if where == "last_row" else T + 5
    if kind == "descending":
        bad[row][i], bad[row][i + 1] = bad[row][i + 1], bad[row][i]
    elif kind == "repeated":
        bad[row][i + 1] = bad[row][i]
    else:
        bad[row][i + 1] = cols
        if where == "last_row":
            assert np.all(np.diff(bad[row]) > 0)                          # only the range is wrong
    bad_a = _csr(bad, rows, 1)
    # the other operand stays valid; with side B the roles are exchanged (the same rows of B are empty in A)
    a, b = (bad_a, good_b) if side == "A" else (good_b, bad_a)
    for op in ref.OPS:
        for device in (True, False):
            st, _, _ = _ewise(a, b, rows, cols, op, device=device)
            assert st == INVALID, (op, device)
    st, _, _ = _ewise(good_a, good_b, rows, cols, "union")                # the call after a refusal is exact
    assert st == 0


@pytest.mark.parametrize("side", ["A", "B"])
def test_contract_violations_in_rowptr(side):
    fa, fb, rows, cols, _ = _violation_base()
    good_a, good_b = _csr(fa, rows, 1), _csr(fb, rows, 2)
    for kind in ("first", "decreasing"):
        rp = good_a[0].copy()
        if kind == "first":
            rp[0] = 1
        else:
            rp[4] = rp[3] - 2
        bad = (rp, good_a[1], good_a[2])
        a, b = (bad, good_b) if side == "A" else (good_b, bad)
        for op in ref.OPS:
            for device in (True, False):
                st, _, _ = _ewise(a, b, rows, cols, op, device=device)
                assert st == INVALID, (kind, op, device)


# ------------------------------------------------------------------------------------------------ 6. select
def _select(a, rows, cols, pred, k=0, thr=0.0, device=True, values=True):
    from g4s_amd import capi, host
    lib = capi.load()
    pv = host.SELECT_PREDICATES[pred]
    cnnz = C.c_int64(-5)
    if device:
        t = [_T(a[0], np.int32), _T(a[1], np.int32), _T(a[2], np.float64) if values else None]
        crp = torch.full((rows + 1,), -9, dtype=torch.int32, device="cuda")
        q = host._ptr_nn
        vptr = q(t[2]) if values else C.c_void_p(0)
        capi.check(lib.g4s_csr_select_symbolic(pv, k, thr, rows, cols, q(t[0]), q(t[1]), vptr, q(crp), C.byref(cnnz), capi.DEVICE_POINTERS, host._stream()))
        assert cnnz.value == int(crp[rows].item())
        cci = torch.full((cnnz.value,), -9, dtype=torch.int32, device="cuda")
        cva = torch.full((cnnz.value,), -9.0, dtype=torch.float64, device="cuda") if values else None
        capi.check(lib.g4s_csr_select_numeric(pv, k, thr, rows, cols, q(t[0]), q(t[1]), vptr, q(crp), q(cci), q(cva) if values else C.c_void_p(0),
                                              capi.DEVICE_POINTERS, host._stream()))
        return crp.cpu().numpy(), cci.cpu().numpy(), cva.cpu().numpy() if values else None
    h = [np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.int32), np.ascontiguousarray(a[2], np.float64) if values else None]
    crp = np.full(rows + 1, -9, np.int32)
    capi.check(lib.g4s_csr_select_symbolic(pv, k, thr, rows, cols, _P(h[0]), _P(h[1]), _P(h[2]), _P(crp), C.byref(cnnz), capi.HOST_POINTERS, None))
    assert cnnz.value == crp[rows]
    cci = np.full(cnnz.value + 1, -9, np.int32)
    cva = np.full(cnnz.value + 1, -9.0, np.float64) if values else None
    capi.check(lib.g4s_csr_select_numeric(pv, k, thr, rows, cols, _P(h[0]), _P(h[1]), _P(h[2]), _P(crp), _P(cci), _P(cva), capi.HOST_POINTERS, None))
    assert cci[-1] == -9
    return crp, cci[:-1], cva[:-1] if values else None


def _shuffled_with_repeats(rows, cols, seed, max_len):
    rp, ci, va = helpers.power_law_csr(rows, cols, seed, max_len)
    rng = np.random.default_rng(seed + 100)
    out = {}
    for r in range(rows):
        c = ci[rp[r]:rp[r + 1]].astype(np.int64)
        if len(c):
            c = np.concatenate([c, rng.choice(c, len(c) // 3 + 1)])      # repeated columns
            c[rng.integers(0, len(c))] = r if r < cols else 0            # and a diagonal entry now and then
            c = rng.permutation(c)
        out[r] = c
    return _csr(out, rows, seed)


@functools.lru_cache(maxsize=None)
def _select_case():
    return _shuffled_with_repeats(400, 500, 31, 300)


@pytest.mark.parametrize("pred", ref.PREDICATES)
def test_select_every_predicate(pred):
    a = _select_case()
    rows, cols = 400, 500
    special = a[2].copy()
    special[::7], special[1::7], special[2::7] = np.nan, 0.0, -0.0
    a = (a[0], a[1], special)
    positional = pred in ("tril", "triu", "offdiag", "diag")
    for k, thr in ([(k, 0.0) for k in (-cols, -1, 0, 1, cols)] if pred in ("tril", "triu") else [(0, 0.0), (0, 0.25), (0, -0.5)]):
        for device in (True, False):
            _same(_select(a, rows, cols, pred, k, thr, device=device), ref.select(a, rows, pred, k, thr), (pred, k, thr, device))
            if positional:
                got = _select(a, rows, cols, pred, k, thr, device=device, values=False)
                _same(got, ref.select((a[0], a[1], None), rows, pred, k, thr), (pred, k, thr, device))


def test_select_long_row():
    rng = np.random.default_rng(41)
    cols = 60000
    a = _csr({0: rng.permutation(50), 1: rng.permutation(cols)[:50000], 2: rng.permutation(30)}, 3, 6)
    for pred, k, thr in (("tril", 20000, 0.0), ("triu", 100, 0.0), ("gt", 0, 0.1), ("offdiag", 0, 0.0), ("diag", 0, 0.0)):
        _same(_select(a, 3, cols, pred, k, thr), ref.select(a, 3, pred, k, thr), pred)


# ------------------------------------------------------------------------------------------------ 7. symmetrise
def _directed_graph(n, seed, max_len):
    from g4s_amd import host
    rp, ci, va = helpers.power_law_csr(n, n, seed, max_len)
    loops = (np.arange(n + 1, dtype=np.int32).clip(0, n // 10), np.arange(n // 10, dtype=np.int32), np.full(n // 10, 0.5))
    a = ref.ewise((rp, ci, va), loops, n, n, "union", "first")          # some self-loops
    return a, host.CSR.from_host(a[0], a[1], a[2], n, n)


def _host(c):
    return tuple(x for x in c.to_host())


def test_symmetrise():
    n = 2000
    a, A = _directed_graph(n, 51, 400)
    at = ref.transpose(a, n, n)
    for combine in ("max", "plus"):
        S = A.symmetrise(combine)
        want = ref.ewise(a, at, n, n, "union", combine)
        _same(_host(S), want, combine)
        _same(_host(S.transpose()), want, combine)                      # its transpose equals it, all three arrays
    S = A.symmetrise()
    assert np.array_equal(S.connected_components(symmetric=True).cpu().numpy(), A.connected_components().cpu().numpy())
    want = ref.ewise(a, at, n, n, "union", "max")
    _same(_host(S.select("tril", -1)), ref.select(want, n, "tril", -1))
    D = A.symmetrise(drop_diagonal=True)
    _same(_host(D), ref.select(want, n, "offdiag"))
    assert np.any(ref.select_mask(*want, "diag")) and not np.any(ref.select_mask(*_host(D), "diag"))
    _same(_host(A.ewise(A, "difference")), ref.ewise(a, a, n, n, "difference"))
    got, info = A.ewise(S, "intersect", "second", return_info=True)
    _same(_host(got), ref.ewise(a, want, n, n, "intersect", "second"))
    assert info["nnz_c"] == A.nnz
    p = A.ewise(S, pattern_only=True)
    assert np.array_equal(p.colids.cpu().numpy(), want[1]) and bool(torch.all(p.values == 1.0))


def test_symmetrise_feeds_triangle_count():
    n = 300
    a, A = _directed_graph(n, 52, 60)
    S = A.symmetrise(drop_diagonal=True)
    rp, ci, _ = _host(S)
    adj = np.zeros((n, n), np.int64)
    adj[ref.row_of_entry(rp), ci] = 1
    assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
    want = int(np.trace(adj @ adj @ adj)) // 6
    assert want > 0 and S.triangle_count() == want


# ------------------------------------------------------------------------------------------------ 9. the two-call C form on a stream of its own
def test_two_call_form_on_a_stream():
    a, b, rows, cols = _hub_case()
    s = torch.cuda.Stream()
    for op in ref.OPS:
        st, got, info = _ewise(a, b, rows, cols, op, "max", stream=s)
        assert st == 0
        _same(got, ref.ewise(a, b, rows, cols, op, "max"))
        assert info["nnz_c"] == got[0][rows] == len(got[1])
