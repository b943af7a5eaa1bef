"""g4s_ilu0_* on the device. Every comparison is exact: the info fields, the pivot word, every factor value and every z are compared with == against
tests/ilu_ref.py, the doubles bit for bit through view(int64) — the header fixes the arithmetic, and the reference restates it. Each case runs with
device and with host pointers, with chains and with one launch per level; every output is pre-filled with a sentinel and the caller's arrays are
overwritten behind the analysis."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ilu_ref as ref
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

FILL, WORD = -7.25, 0x5A5A


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(got, want, what=None):
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, np.flatnonzero(diff)[:8], np.asarray(got)[diff][:4], np.asarray(want)[diff][:4])


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()                # a copy: the shared cases are read-only


class Fact:
    """The C entry points themselves: a handle, its info, the status."""

    def __init__(self, mat, no_chains=False, device=True, stream=None, check=True):
        from g4s_amd import capi, host
        self.capi, self.host, self.lib = capi, host, capi.load()
        n, rp, ci, va = mat
        self.n, self.nnz, self.stream, self.device = n, int(np.asarray(va).size), stream, device
        flags = capi.ILU0_NO_CHAINS if no_chains else 0
        self.handle = C.c_void_p(0x5EED)                                    # a refusal leaves *out untouched
        info = capi.ILU0Info()
        if device:
            arrs = (_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64))
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
            self.status = self.lib.g4s_ilu0_analyse(C.byref(self.handle), n, *(host._ptr_nn(a) for a in arrs), flags | capi.DEVICE_POINTERS, C.byref(info),
                                                    self._s())
            for a in arrs:                                                  # the handle keeps its own copy
                a.fill_(-1)
            torch.cuda.synchronize()
        else:
            arrs = (np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64))
            spare = np.zeros(1, np.float64)
            P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
            self.status = self.lib.g4s_ilu0_analyse(C.byref(self.handle), n, *(P(a) for a in arrs), flags | capi.HOST_POINTERS, C.byref(info), self._s())
            for a in arrs:
                a.fill(-1)
        self.info = {k: getattr(info, k) for k, _ in capi.ILU0Info._fields_}
        if check:
            capi.check(self.status)

    def _s(self):
        return C.c_void_p(self.stream.cuda_stream) if self.stream is not None else self.host._stream()

    def _wait(self):
        (self.stream or torch.cuda.current_stream()).synchronize()

    def factors(self):
        """the factor array, read the way the handle was made: into a sentinel-filled device tensor or host array one entry longer"""
        if self.device:
            out = torch.full((self.nnz + 1,), FILL, dtype=torch.float64, device="cuda")
            if self.stream is not None:
                self.stream.wait_stream(torch.cuda.current_stream())
            self.capi.check(self.lib.g4s_ilu0_get_factors(self.handle, self.host._ptr_nn(out), self.capi.DEVICE_POINTERS, self._s()))
            self._wait()
            out = out.cpu().numpy()
        else:
            out = np.full(self.nnz + 1, FILL)
            self.capi.check(self.lib.g4s_ilu0_get_factors(self.handle, C.c_void_p(out.ctypes.data), self.capi.HOST_POINTERS, self._s()))
        assert out[self.nnz] == FILL
        return out[:self.nnz]

    def factor(self, values=None):
        """g4s_ilu0_factor the way the handle was made; returns the pivot word"""
        word = torch.full((2,), WORD, dtype=torch.int32, device="cuda")
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
        if values is None:
            st = self.lib.g4s_ilu0_factor(self.handle, None, self.capi.DEVICE_POINTERS if self.device else 0, self.host._ptr_nn(word), self._s())
        elif self.device:
            v = _dev(values, np.float64)
            if self.stream is not None:
                self.stream.wait_stream(torch.cuda.current_stream())
            st = self.lib.g4s_ilu0_factor(self.handle, self.host._ptr_nn(v), self.capi.DEVICE_POINTERS, self.host._ptr_nn(word), self._s())
            self._wait()
            v.fill_(-1)
        else:
            v = np.array(values, np.float64)
            st = self.lib.g4s_ilu0_factor(self.handle, C.c_void_p(v.ctypes.data), self.capi.HOST_POINTERS, self.host._ptr_nn(word), self._s())
            v.fill(-1)
        self.capi.check(st)
        self._wait()
        word = word.cpu().numpy()
        assert word[1] == WORD
        return int(word[0])

    def apply(self, r, alias=False, stream=None):
        stream = stream or self.stream
        rt = _dev(r, np.float64) if self.n else torch.zeros(1, dtype=torch.float64, device="cuda")
        zt = rt if alias else torch.full((max(self.n, 1),), FILL, dtype=torch.float64, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else self.host._stream()
        self.capi.check(self.lib.g4s_ilu0_apply(self.handle, self.host._ptr_nn(rt), self.host._ptr_nn(zt), s))
        (stream or torch.cuda.current_stream()).synchronize()
        out = zt.cpu().numpy()
        if not alias:
            assert np.all(out[self.n:] == FILL) and np.array_equal(_bits(rt.cpu().numpy()[:self.n]), _bits(np.asarray(r)[:self.n]))
        return out[:self.n]

    def close(self):
        if self.status == 0:
            self.capi.check(self.lib.g4s_ilu0_destroy(self.handle))
            self.status = 1


def _check_info(got, want):
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["host_waits"] <= got["launches"] // 16 + ref.HOST_WAITS_SLACK and got["launches"] >= got["launches_per_factor"], got


def check_case(name, mat, f, info, r, z):
    """both pointer kinds, chains and one launch per level: the reference's info, pivot word and bits — of the factors, and of z for r != z and r = z
    (tests/test_ilu_limits_gpu.py runs its cases through the same checks)"""
    for device in (True, False):
        for no_chains in (False, True):
            p = Fact(mat, no_chains, device)
            _check_info(p.info, ref.info(*mat, no_chains) if no_chains else info)
            if no_chains:
                assert (p.info["launches_per_factor"], p.info["chains"]) == (info["levels"], 0)
            _same_bits(p.factors(), f, (name, device, no_chains, "factors"))
            _same_bits(p.apply(r), z, (name, device, no_chains))
            _same_bits(p.apply(r, alias=True), z, (name, device, no_chains, "z is r"))
            assert p.factor() == info["bad_pivot"]                          # refactorise what is held: the same bits, the same word
            _same_bits(p.factors(), f, (name, device, no_chains, "again"))
            assert p.factor() == info["bad_pivot"]
            _same_bits(p.factors(), f, (name, device, no_chains, "a third time"))
            _same_bits(p.apply(r), z, (name, device, no_chains, "behind factor"))
            if device and not no_chains:
                print(f"{name}: {p.info}")
            p.close()


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_equals_reference(name):
    check_case(name, *ref.case(name))


def test_apply_is_the_two_solves_of_the_reference():
    for name in ("grid40", "messy", "dense_70"):
        (n, rp, ci, va), f, _, r, z = ref.case(name)
        y = tr.solve(n, rp, ci, f, r, True, True)
        _same_bits(tr.solve(n, rp, ci, f, y, False, False), z)
        p = Fact((n, rp, ci, va))
        _same_bits(p.apply(r), z, name)
        _same_bits(p.apply(r, alias=True), z, name)
        p.close()


def test_zero_pivot_is_reported_not_refused():
    mat, f, info, r, z = ref.case("zero_pivot")
    assert info["bad_pivot"] == 2 and np.isinf(f).any() and np.isnan(f).any()
    print("zero pivot factors:", [hex(v & (2**64 - 1)) for v in _bits(f).tolist()])
    for device in (True, False):
        for no_chains in (False, True):
            p = Fact(mat, no_chains, device)
            assert p.info["bad_pivot"] == 2 and p.info["bad_row"] == -1
            _same_bits(p.factors(), f)
            assert p.factor() == 2
            good = np.array(mat[3])
            good[mat[1][2] + 1] = 5.0                                       # a_22 = 5: no pivot is zero any more
            want, bad = ref.factor(mat[0], mat[1], mat[2], good)
            assert bad == -1 and np.all(np.isfinite(want))
            assert p.factor(good) == -1
            _same_bits(p.factors(), want)
            p.close()


def test_factor_with_new_values_equals_a_fresh_analysis():
    for name in ("messy", "grid40", "arrow_wave_plus_1", "row0_full"):
        (n, rp, ci, va), f, info, r, z = ref.case(name)
        rowid = np.repeat(np.arange(n), np.diff(rp))
        new = np.random.default_rng(11).uniform(1.0, 2.0, va.size) * np.where(ci == rowid, 16.0 + np.diff(rp)[rowid], 0.125)
        want, bad = ref.factor(n, rp, ci, new)
        want_z = ref.apply(n, rp, ci, want, r)
        assert bad == -1 and not np.array_equal(want, f)
        for device in (True, False):
            p = Fact((n, rp, ci, va), device=device)
            assert p.factor(new) == -1
            _same_bits(p.factors(), want, (name, device))
            _same_bits(p.apply(r), want_z, (name, device))
            assert p.factor() == -1                                         # what is held is the new values
            _same_bits(p.factors(), want, (name, device, "held"))
            fresh = Fact((n, rp, ci, new), device=device)
            _same_bits(fresh.factors(), want)
            _same_bits(fresh.apply(r), want_z)
            got, again = C.create_string_buffer(48), C.create_string_buffer(48)
            p.capi.check(p.lib.g4s_ilu0_get_info(p.handle, C.cast(got, C.POINTER(p.capi.ILU0Info))))
            p.capi.check(p.lib.g4s_ilu0_get_info(fresh.handle, C.cast(again, C.POINTER(p.capi.ILU0Info))))
            assert got.raw[:40] == again.raw[:40]                          # everything but the analysis's own launch counts
            p.close()
            fresh.close()


def _refused(mat, want_bad_row):
    kind, row = ref.refusal(*mat[:3])
    assert row == want_bad_row
    for device in (True, False):
        p = Fact(mat, device=device, check=False)
        assert p.status == p.capi.ERR_INVALID and ref.REFUSAL_TEXT[kind] in p.lib.g4s_last_error().decode(), (p.status, p.lib.g4s_last_error())
        if row >= 0:
            assert f"row {row} " in p.lib.g4s_last_error().decode()
        assert p.handle.value == 0x5EED and p.info["bad_row"] == want_bad_row and p.info["bad_pivot"] == -1
        good, f, _, r, z = ref.case("messy")                                # a correct call straight after the refusal
        q = Fact(good, device=device)
        _same_bits(q.factors(), f)
        _same_bits(q.apply(r), z)
        q.close()


def test_rows_that_are_not_canonical_are_refused():
    n, rp, ci, va = ref.case("grid40")[0]
    for rows in ([1234], [1599, 777, 1234]):                                # an unsorted row; the smallest of several
        c2 = np.array(ci)
        for i in rows:
            k = int(rp[i])
            c2[k], c2[k + 1] = ci[k + 1], ci[k]
        _refused((n, rp, c2, va), min(rows))
    c3 = np.array(ci)
    c3[int(rp[900]) + 1] = c3[int(rp[900])]                                 # a repeated column
    _refused((n, rp, c3, va), 900)
    rowid = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((ci == rowid) & np.isin(rowid, [1599, 777, 1234]))             # three rows without their diagonal entry
    r4 = np.concatenate([[0], np.cumsum(np.bincount(rowid[keep], minlength=n))]).astype(np.int32)
    _refused((n, r4, ci[keep], va[keep]), 777)
    mixed = np.array(c2)                                                    # rows 777, 1234 and 1599 unsorted, row 5 with an id out of range: the smallest
    mixed[int(rp[5])] = n
    _refused((n, rp, mixed, va), 5)
    _refused((2, np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32), np.ones(2)), 1)   # row 1 stores column 0 only


def test_bad_ids_and_a_bad_rowptr_are_refused():
    n, rp, ci, va = ref.case("messy")[0]
    row = int(np.searchsorted(rp, ci.size // 2, side="right") - 1)
    for bad_id in (n, -1, 2**31 - 1):
        c2 = np.array(ci)
        c2[c2.size // 2] = bad_id
        _refused((n, rp, c2, va), row)
    r2 = np.array(rp)
    r2[n // 2] = r2[n // 2 + 1] + 1                                         # decreases behind it
    _refused((n, r2, ci, va), -1)
    r3 = np.array(rp)
    r3[0] = 1
    _refused((n, r3, ci, va), -1)


def test_on_a_side_stream():
    mat, f, info, r, z = ref.case("blocks")
    side = torch.cuda.Stream()
    for device in (True, False):
        p = Fact(mat, device=device, stream=side)                           # the analysis on the side stream too
        _same_bits(p.factors(), f)
        _same_bits(p.apply(r), z)
        assert p.factor() == -1
        _same_bits(p.apply(r, alias=True), z)
        p.stream = None
        _same_bits(p.apply(r), z)                                           # and on the current stream, the same handle
        p.close()


def test_factor_and_apply_in_a_captured_graph():
    """the capture itself proves that factor with device pointers and apply wait for nothing on the host; replays on changed values equal the eager bits"""
    from g4s_amd import host
    for name in ("blocks", "grid40", "arrow_wave_plus_1"):
        (n, rp, ci, va), f, info, r0, z0 = ref.case(name)
        M = host.ilu0((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)))
        assert {k: M.info[k] for k in info} == info
        vals, r = _dev(va, np.float64), _dev(r0, np.float64)
        z = torch.full((n,), FILL, dtype=torch.float64, device="cuda")
        word = torch.full((1,), WORD, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                host.capi.check(host.capi.load().g4s_ilu0_factor(M._handle, host._ptr_nn(vals), host.capi.DEVICE_POINTERS, host._ptr_nn(word), host._stream()))
                M.apply(r, out=z)
        torch.cuda.current_stream().wait_stream(side)
        rowid = np.repeat(np.arange(n), np.diff(rp))
        for k in range(2):
            new = np.random.default_rng(30 + k).uniform(1.0, 2.0, va.size) * np.where(ci == rowid, 16.0 + np.diff(rp)[rowid], 0.125)
            vals.copy_(torch.from_numpy(new))
            z.fill_(FILL)
            word.fill_(WORD)
            g.replay()
            torch.cuda.synchronize()
            want, bad = ref.factor(n, rp, ci, new)
            assert int(word.item()) == bad == -1
            _same_bits(M.factors().cpu().numpy(), want, (name, k))
            _same_bits(z.cpu().numpy(), ref.apply(n, rp, ci, want, r0), (name, k, "reference"))
            _same_bits(z.cpu().numpy(), M.apply(r).cpu().numpy(), (name, k, "eager"))
        M.close()


def test_analysis_is_refused_on_a_capturing_stream():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, va = ref.case("messy")[0]
    arrs = (_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64))
    info, handle = capi.ILU0Info(), C.c_void_p(0x5EED)
    info.levels = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_ilu0_analyse(C.byref(handle), n, *(host._ptr(a) for a in arrs), capi.DEVICE_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.levels == -3 and handle.value == 0x5EED
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    M = host.ilu0(arrs)                                                     # and the library still works
    _same_bits(M.factors().cpu().numpy(), ref.case("messy")[1])
    M.close()


def test_host_layer():
    from g4s_amd import host
    (n, rp, ci, va), f, info, r, z = ref.case("messy")
    A = host.CSR.from_host(rp, ci, va, n, n)
    for a in (A, (rp, ci, va), (A.rowptr, A.colids, A.values)):
        for no_chains in (False, True):
            M = host.ilu0(a, no_chains=True) if no_chains else A.ilu0() if a is A else host.ilu0(a)
            want_info = ref.info(n, rp, ci, va, no_chains)
            assert {k: M.info[k] for k in want_info} == want_info
            assert M.factors().is_cuda and M.factors().numel() == va.size
            _same_bits(M.factors().cpu().numpy(), f)
            rt = torch.from_numpy(np.array(r)).cuda()
            _same_bits(M.apply(rt).cpu().numpy(), z)
            assert M.apply(rt, out=rt) is rt
            _same_bits(rt.cpu().numpy(), z)
            with pytest.raises(ValueError):
                M.apply(rt[:-1])
            with pytest.raises(ValueError):
                M.factor(A.values[:-1])
            want, _ = ref.factor(n, rp, ci, 2.0 * va)
            assert int(M.factor(A.values * 2.0).item()) == -1               # a device tensor
            _same_bits(M.factors().cpu().numpy(), want)
            assert int(M.factor(va).item()) == -1                           # a numpy array: host pointers
            _same_bits(M.factors().cpu().numpy(), f)
            assert int(M.factor().item()) == -1
            _same_bits(M.factors().cpu().numpy(), f)
            M.close()
            M.close()
    with pytest.raises(Exception, match="row 0 stores no diagonal entry"):
        host.ilu0((np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0)))


def test_preconditioned_cg_converges_in_fewer_than_half_the_iterations():
    """host.pcg on the grid Laplacian, tol 1e-10: the true relative residual, recomputed in numpy from the returned x, is at most 10 · tol with and
    without the preconditioner, and ILU(0) takes fewer than half the iterations of plain CG"""
    from g4s_amd import host
    (n, rp, ci, va), f, _, _, _ = ref.case("grid40")
    b = np.random.default_rng(40).uniform(-1.0, 1.0, n)
    a = tr.dense(n, rp, ci, va)
    A = host.CSR.from_host(rp, ci, va, n, n)
    M = A.ilu0()
    bt = torch.from_numpy(b).cuda()
    x0, it0, res0 = host.pcg(A, bt, None, tol=1e-10)
    x1, it1, res1 = host.pcg(A, bt, M, tol=1e-10)
    true0 = np.linalg.norm(b - a @ x0.cpu().numpy()) / np.linalg.norm(b)
    true1 = np.linalg.norm(b - a @ x1.cpu().numpy()) / np.linalg.norm(b)
    print(f"pcg: {it0} iterations without M (true residual {true0:.3e}), {it1} with ILU(0) ({true1:.3e})")
    assert true0 <= 1e-9 and true1 <= 1e-9 and res0 <= 1e-10 and res1 <= 1e-10
    assert it1 < it0 / 2
    x2, it2, _ = host.pcg(A, bt, M, x0=x1, tol=1e-10)                       # from the solution: next to nothing left to do
    assert it2 < it1 / 2 and torch.equal(bt, torch.from_numpy(b).cuda())
    with pytest.raises(ValueError):
        host.pcg(A, bt[:-1])
    with pytest.raises(ValueError):
        host.pcg(A, bt, tol=0.0)
    M.close()
