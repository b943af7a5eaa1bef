"""g4s_sptrsv_* on the device. Every comparison is exact: the levels, the info fields and every x are compared with == against tests/trsv_ref.py, x bit for
bit through view(int64) — the header fixes the arithmetic shape of a row, and the reference restates it. Each case runs with device and with host
pointers, and every output is pre-filled with a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import trsv_ref as ref

pytestmark = pytest.mark.gpu

FILL, XFILL = -7, -7.25


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(got, want, what=None):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.flatnonzero(_bits(got) != _bits(want))[:8], got[_bits(got) != _bits(want)][:4],
                                                     np.asarray(want)[_bits(got) != _bits(want)][:4])


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()                # a copy: the shared cases are read-only


class Plan:
    """The C entry points themselves: a handle, the level array the analysis wrote (pre-filled), its info, the status."""

    def __init__(self, mat, lower=True, unit=False, no_chains=False, device=True, stream=None, with_level=True, check=True):
        from g4s_amd import capi, host
        self.capi, self.host, self.lib = capi, host, capi.load()
        n, rp, ci, va = mat
        self.n, self.stream = n, stream
        flags = (0 if lower else capi.TRSV_UPPER) | (capi.TRSV_UNIT_DIAGONAL if unit else 0) | (capi.TRSV_NO_CHAINS if no_chains else 0)
        self.handle = C.c_void_p(0x5EED)                                    # a refusal leaves *out untouched
        info = capi.TRSVInfo()
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        if device:
            arrs = (_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64))
            lev = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
            self.status = self.lib.g4s_sptrsv_analyse(C.byref(self.handle), n, *(host._ptr_nn(a) for a in arrs), host._ptr_nn(lev) if with_level else None,
                                                      flags | capi.DEVICE_POINTERS, C.byref(info), s)
            for a in arrs:                                                  # the handle keeps its own copy: the caller's arrays need not outlive the analysis
                a.fill_(-1)
            torch.cuda.synchronize()
            lev = lev.cpu().numpy()
        else:
            arrs = (np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64))
            lev = np.full(max(n, 1), FILL, np.int32)
            spare = np.zeros(1, np.float64)
            P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
            self.status = self.lib.g4s_sptrsv_analyse(C.byref(self.handle), n, *(P(a) for a in arrs), P(lev) if with_level else None, flags | capi.HOST_POINTERS,
                                                      C.byref(info), s)
            for a in arrs:
                a.fill(-1)
        self.level_raw = lev
        self.level = lev[:n]
        self.info = {k: getattr(info, k) for k, _ in capi.TRSVInfo._fields_}
        if check:
            capi.check(self.status)

    def solve(self, b, alias=False, stream=None):
        stream = stream or self.stream
        bt = _dev(b, np.float64) if self.n else torch.zeros(1, dtype=torch.float64, device="cuda")
        xt = bt if alias else torch.full((max(self.n, 1),), XFILL, dtype=torch.float64, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else self.host._stream()
        self.capi.check(self.lib.g4s_sptrsv_solve(self.handle, self.host._ptr_nn(bt), self.host._ptr_nn(xt), s))
        if stream is not None:
            stream.synchronize()
        out = xt.cpu().numpy()
        if not alias:
            assert np.all(out[self.n:] == XFILL) and np.array_equal(_bits(bt.cpu().numpy()[:self.n]), _bits(np.asarray(b)[:self.n]))
        return out[:self.n]

    def close(self):
        if self.status == 0:
            self.capi.check(self.lib.g4s_sptrsv_destroy(self.handle))
            self.status = 1


def _check_info(got, want):
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["host_waits"] <= got["launches"] // 16 + 5, got


def _exact(mat, lower, unit, b, what):
    """both pointer kinds, chains and one launch per level: the reference's levels, counts and bits; (info with chains, info without)"""
    want_lev, want_x = ref.levels(*mat, lower, unit), ref.solve(*mat, b, lower, unit)
    infos = []
    for device in (True, False):
        for no_chains in (False, True):
            p = Plan(mat, lower, unit, no_chains, device)
            assert np.array_equal(p.level, want_lev), (what, device)
            _check_info(p.info, ref.info(*mat, lower, unit, no_chains))
            for alias in (False, True):
                _same_bits(p.solve(b, alias), want_x, (what, device, no_chains, alias))
            infos.append(p.info)
            p.close()
    return infos[0], infos[1]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_equals_reference(name):
    mat, lev, info, b, x = ref.case(name)
    for device in (True, False):
        p = Plan(mat, device=device)
        assert np.array_equal(p.level, lev) and np.all(p.level_raw[mat[0]:] == FILL)
        _check_info(p.info, info)
        _same_bits(p.solve(b), x, (name, device))
        _same_bits(p.solve(b), x, (name, device, "again"))                  # the handle is only read
        _same_bits(p.solve(b, alias=True), x, (name, device, "x is b"))
        if device:
            print(f"{name}: {p.info}")
        p.close()
    q = Plan(mat, no_chains=True, with_level=False)
    assert np.all(q.level_raw == FILL)                                      # a NULL level: nothing is written
    assert (q.info["launches_per_solve"], q.info["chains"]) == (info["levels"], 0)
    _same_bits(q.solve(b), x, (name, "one launch per level"))
    q.close()


@pytest.mark.parametrize("name", ["grid40", "messy", "n1", "diagonal_300"])
def test_upper_triangle(name):
    mat, _, _, b, _ = ref.case(name)
    with_chains, without = _exact(mat, False, False, b, name)
    assert without["launches_per_solve"] == without["levels"] and without["chains"] == 0


def test_the_other_triangle_is_not_read():
    """a full unsymmetric matrix solved as lower and as upper; the entries of the other triangle are NaN"""
    mat = ref.full(60)
    b = np.random.default_rng(3).uniform(-1, 1, 60)
    for lower in (True, False):
        clean = ref.solve(*mat, b, lower)
        assert np.all(np.isfinite(clean))
        poisoned = ref.poison_other_triangle(mat, lower)
        assert np.isnan(poisoned[3]).sum() == 60 * 59 // 2
        with_chains, _ = _exact(poisoned, lower, False, b, ("full", lower))
        assert with_chains["levels"] == 60 and with_chains["nnz_triangle"] == 60 * 61 // 2
        p = Plan(poisoned, lower)
        _same_bits(p.solve(b), clean)
        p.close()


def test_unit_diagonal_ignores_stored_diagonal_entries():
    mat = ref.unit_poisoned(90)
    b = np.random.default_rng(4).uniform(-1, 1, 90)
    assert np.isnan(mat[3]).sum() == 45 and np.all(np.isfinite(ref.solve(*mat, b, True, True)))
    info, _ = _exact(mat, True, True, b, "unit")
    assert info["nnz_triangle"] == int(np.isfinite(mat[3]).sum())
    p = Plan(mat, unit=False, check=False)                                  # without the flag the rows that store none are refused
    assert p.status == p.capi.ERR_INVALID and p.info["bad_row"] == 0 and p.handle.value == 0x5EED


SPECIAL_ROWS = [[(0, 0.0)], [(1, -0.0)], [(2, float("inf"))], [(3, 2.0)], [(4, float("nan"))], [(0, 2.0), (5, 1.0)], [(3, 1.0), (6, 1.0)],
                [(6, 1.0), (7, 1.0)], [(8, 2.0)], [(3, 5.0), (9, -4.0)], [(3, 0.0), (10, 1.0)]]
SPECIAL_B = [1.0, 1.0, 1.0, -0.0, 1.0, 1.0, float("nan"), 1.0, float("inf"), 0.0, -0.0]


def test_zero_inf_and_nan_by_bits():
    """±0.0, inf and NaN on the diagonal and in b: the division is IEEE and nothing is refused. A NaN x is stored in its canonical form (g4s.h), so
    every entry is compared by bits; row 7 is 1 − NaN, where the device's b + (−s) would otherwise flip the NaN's sign."""
    mat = ref.csr(SPECIAL_ROWS)
    b = np.array(SPECIAL_B)
    want = ref.solve(*mat, b)
    print("specials:", [hex(v & (2**64 - 1)) for v in _bits(want).tolist()])
    assert want[0] == np.inf and want[1] == -np.inf and want[2] == 0.0 and np.signbit(want[3]) and np.isnan(want[[4, 6, 7]]).all() and want[5] == -np.inf
    assert want[8] == np.inf and want[9] == 0.0 and np.signbit(want[9]) and want[10] == 0.0 and np.signbit(want[10])
    for device in (True, False):
        for no_chains in (False, True):
            p = Plan(mat, no_chains=no_chains, device=device)
            got = p.solve(b)
            print("specials got:", [hex(v & (2**64 - 1)) for v in _bits(got).tolist()])
            _same_bits(got, want, ("specials", device, no_chains))
            p.close()


def test_update_values_equals_a_fresh_analysis():
    from g4s_amd import host
    for name, lower in (("messy", True), ("messy", False), ("grid40", True), ("hub_row", True)):
        mat, _, _, b, _ = ref.case(name)
        n, rp, ci, va = mat
        new = np.random.default_rng(11).uniform(1.0, 2.0, va.size) * np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 8.0, 0.125)
        want = ref.solve(n, rp, ci, new, b, lower)
        assert not np.array_equal(want, ref.solve(*mat, b, lower))
        for device in (True, False):
            p = Plan(mat, lower, device=device)
            if device:
                p.capi.check(p.lib.g4s_sptrsv_update_values(p.handle, host._ptr_nn(_dev(new, np.float64)), p.capi.DEVICE_POINTERS, host._stream()))
            else:
                p.capi.check(p.lib.g4s_sptrsv_update_values(p.handle, C.c_void_p(new.ctypes.data), p.capi.HOST_POINTERS, host._stream()))
            _same_bits(p.solve(b), want, (name, lower, device))
            fresh = Plan((n, rp, ci, new), lower)
            _same_bits(fresh.solve(b), want)
            got, again = C.create_string_buffer(48), C.create_string_buffer(48)
            p.capi.check(p.lib.g4s_sptrsv_get_info(p.handle, C.cast(got, C.POINTER(p.capi.TRSVInfo))))
            p.capi.check(p.lib.g4s_sptrsv_get_info(fresh.handle, C.cast(again, C.POINTER(p.capi.TRSVInfo))))
            assert got.raw[:32] == again.raw[:32]                          # everything but the analysis's own launch counts
            p.close()
            fresh.close()


def _refused(mat, text, want_bad_row=-1, **kw):
    for device in (True, False):
        p = Plan(mat, device=device, check=False, **kw)
        assert p.status == p.capi.ERR_INVALID and text in p.lib.g4s_last_error().decode(), (p.status, p.lib.g4s_last_error())
        assert p.handle.value == 0x5EED and p.info["bad_row"] == want_bad_row
        good, _, _, b, x = ref.case("messy")                               # a correct call straight after the refusal
        q = Plan(good, device=device)
        _same_bits(q.solve(b), x)
        q.close()


def test_missing_diagonal_reports_the_smallest_row():
    n, rp, ci, va = ref.case("grid40")[0]
    rowid = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((ci == rowid) & np.isin(rowid, [1599, 777, 1234]))
    cut = ref.csr([[(int(c), float(v)) for c, v in zip(ci[(rowid == i) & keep], va[(rowid == i) & keep])] for i in range(n)])
    assert ref.bad_row(*cut) == 777
    _refused(cut, "row 777 stores no diagonal entry", 777)
    p = Plan(cut, device=True, check=False)
    assert np.all(p.level_raw == FILL)                                      # nothing is written
    q = Plan(cut, unit=True)                                                # the same pattern is fine with a unit diagonal
    assert q.info["bad_row"] == -1
    q.close()
    upper_only = ref.csr([[(0, 1.0), (1, 1.0)], [(1, 1.0)], [(0, 1.0)]])   # row 2 stores its diagonal in neither triangle
    _refused(upper_only, "row 2 stores no diagonal entry", 2)
    _refused(upper_only, "row 2 stores no diagonal entry", 2, lower=False)


def test_bad_patterns_are_refused():
    n, rp, ci, va = ref.case("messy")[0]
    for bad_id in (n, -1, 2**31 - 1):
        c2 = np.array(ci)
        c2[c2.size // 2] = bad_id
        _refused((n, rp, c2, va), "a column id is outside [0, n)")
    r2 = np.array(rp)
    r2[n // 2] = r2[n // 2 + 1] + 1                                         # decreases behind it
    _refused((n, r2, ci, va), "rowptr must start at 0 and never decrease")
    r3 = np.array(rp)
    r3[0] = 1
    _refused((n, r3, ci, va), "rowptr must start at 0 and never decrease")


def test_solve_on_a_side_stream():
    mat, lev, info, b, x = ref.case("blocks")
    side = torch.cuda.Stream()
    for device in (True, False):
        p = Plan(mat, device=device, stream=side)                           # the analysis on the side stream too
        assert np.array_equal(p.level, lev)
        _same_bits(p.solve(b), x)
        _same_bits(p.solve(b, alias=True), x)
        p.stream = None
        _same_bits(p.solve(b), x)                                           # and on the current stream, the same handle
        p.close()


def test_solve_in_a_captured_graph():
    """the capture itself proves that the solve waits for nothing on the host; two replays on changed b equal the eager solves"""
    from g4s_amd import host
    for name in ("blocks", "grid40", "hub_row"):
        mat, _, info, b0, x0 = ref.case(name)
        n, rp, ci, va = mat
        plan = host.sptrsv_analyse((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)))
        assert {k: plan.info[k] for k in info} == info
        b, x = _dev(b0, np.float64), torch.full((n,), XFILL, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                plan.solve(b, out=x)
        torch.cuda.current_stream().wait_stream(side)
        for k in range(2):
            bk = np.random.default_rng(20 + k).uniform(-1, 1, n)
            b.copy_(torch.from_numpy(bk))
            x.fill_(XFILL)
            g.replay()
            torch.cuda.synchronize()
            got = x.cpu().numpy()
            eager = plan.solve(b).cpu().numpy()
            _same_bits(got, eager, (name, k))
            _same_bits(got, ref.solve(*mat, bk), (name, k, "reference"))
        plan.close()


def test_analysis_is_refused_on_a_capturing_stream():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, va = ref.case("messy")[0]
    arrs = (_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64))
    lev = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    info, handle = capi.TRSVInfo(), C.c_void_p(0x5EED)
    info.levels = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_sptrsv_analyse(C.byref(handle), n, *(host._ptr(a) for a in arrs), host._ptr(lev), capi.DEVICE_POINTERS, C.byref(info),
                                    C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.levels == -3 and handle.value == 0x5EED
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda")) and torch.all(lev == FILL)   # nothing was enqueued
    plan, got = host.sptrsv_analyse(arrs, return_level=True)                # and the library still works
    assert np.array_equal(got.cpu().numpy(), ref.case("messy")[1])
    plan.close()


def test_analysis_bound_on_a_deep_and_a_wide_matrix():
    """host_waits <= launches / 16 + 5 where the peel makes many batches (a level per launch) and where it makes one"""
    for name in ("bidiagonal_cap_plus_1", "diagonal_300", "grid40"):
        p = Plan(ref.case(name)[0])
        assert p.info["host_waits"] <= p.info["launches"] // 16 + 5 and p.info["launches"] >= p.info["levels"], p.info
        print(name, p.info)
        p.close()


def test_host_layer_plan_and_one_shot():
    from scipy.sparse.linalg import spsolve_triangular
    from g4s_amd import host
    from tests.test_trsv_cpu import _scipy_triangle
    mat = ref.exact_case(48, 10, 4.0)
    n, rp, ci, va = mat
    b = np.random.default_rng(10).integers(-8, 9, n).astype(np.float64)
    A = host.CSR.from_host(rp, ci, va, n, n)
    for lower in (True, False):
        for unit in (False, True):
            want = spsolve_triangular(_scipy_triangle(mat, lower, unit), b, lower=lower, unit_diagonal=unit)
            for a in (A, (rp, ci, va), (A.rowptr, A.colids, A.values)):
                got = host.spsolve_triangular(a, b, lower, unit)
                assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), (lower, unit)
            plan, lev = A.triangular_plan(lower, unit, return_level=True)
            assert np.array_equal(lev.cpu().numpy(), ref.levels(*mat, lower, unit)) and plan.info["levels"] == int(lev.max()) + 1
            bt = torch.from_numpy(b).cuda()
            assert np.array_equal(plan.solve(bt).cpu().numpy(), want)
            assert plan.solve(bt, out=bt) is bt and np.array_equal(bt.cpu().numpy(), want)
            with pytest.raises(ValueError):
                plan.solve(bt[:-1])
            with pytest.raises(ValueError):
                plan.update_values(A.values[:-1])
            plan.update_values(A.values * 2.0)                              # a device tensor
            assert np.array_equal(plan.solve(torch.from_numpy(b).cuda()).cpu().numpy(), ref.solve(n, rp, ci, 2.0 * va, b, lower, unit))
            plan.update_values(2.0 * va)                                    # a numpy array: host pointers
            assert np.array_equal(plan.solve(torch.from_numpy(b).cuda()).cpu().numpy(), ref.solve(n, rp, ci, 2.0 * va, b, lower, unit))
            plan.close()
            plan.close()
    with pytest.raises(Exception, match="stores no diagonal entry"):
        host.sptrsv_analyse((np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0)))


def test_gauss_seidel_equals_its_restatement():
    from g4s_amd import host
    mat = ref.exact_case()
    n, rp, ci, va = mat
    b = np.random.default_rng(5).integers(-4, 5, n).astype(np.float64)
    A = host.CSR.from_host(rp, ci, va, n, n)
    for symmetric in (False, True):
        want = ref.gauss_seidel(*mat, b, np.zeros(n), 3, symmetric)
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        out = host.gauss_seidel(A, torch.from_numpy(b).cuda(), x, sweeps=3, symmetric=symmetric)
        assert out is x and np.array_equal(x.cpu().numpy(), want), symmetric
        plans = (A.triangular_plan(True), A.triangular_plan(False))         # the same with plans that are kept
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        for _ in range(3):
            host.gauss_seidel(A, torch.from_numpy(b).cuda(), y, 1, symmetric, plans=plans)
        assert np.array_equal(y.cpu().numpy(), want)
        for p in plans:
            p.close()
    assert not np.array_equal(ref.gauss_seidel(*mat, b, np.zeros(n), 3, True), ref.gauss_seidel(*mat, b, np.zeros(n), 3, False))
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    assert torch.equal(host.gauss_seidel(A, torch.from_numpy(b).cuda(), x, sweeps=0), torch.ones_like(x))
    with pytest.raises(ValueError):
        host.gauss_seidel(A, torch.from_numpy(b).cuda(), x, sweeps=-1)
    with pytest.raises(ValueError):
        host.gauss_seidel(A, torch.from_numpy(b).cuda()[:-1], x)
