"""g4s_sptrsv_solve_multi on the device (include/g4s.h): T X = B for a block of k right-hand sides on the launches of one solve. Every
comparison is by bits, through view(int64): column j of X against tests/trsv_ref.py's solve of column j and against g4s_sptrsv_solve of column j on the
same plan. Both layouts, with and without padding behind the leading dimension — pre-filled with a sentinel bit pattern that must still be there —,
in place, with one launch per level, with a NaN and an inf column beside finite ones, behind update_values, in a captured graph, from two streams."""
import functools
import subprocess
import threading

import numpy as np
import pytest
import torch

from tests import trsv_ref as ref
from tests.test_cpp_host import _build_example

pytestmark = pytest.mark.gpu

SENT = 0x7FF4DEADBEEF0001                                                  # a NaN no solve produces: the padding's bit pattern
QNAN = 0x7FF8000000000000


def _kt():
    from g4s_amd import capi
    return capi.TRSV_RHS_TILE


def _ks():
    kt = _kt()
    return sorted({1, 2, kt - 1, kt, kt + 1, 2 * kt + 3})                  # one tile, a masked tail, two tiles, three tiles with a tail


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(got, want, what=None):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:8].tolist())


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def rhs(name, lower=True, unit=False):
    """(B, X) for a named case of trsv_ref: B of n × (2·KT + 3) random columns, shared by every k (the first k of them), and the reference's solves
    of the first KT columns — the Python reference would dominate the run time beyond them, and every column is compared with the device's own
    single solve as well. Built once, read-only."""
    mat = ref.case(name, lower, unit)[0]
    n, kt = mat[0], _kt()
    B = np.random.default_rng(7 + len(name)).uniform(-1.0, 1.0, (n, 2 * kt + 3))
    X = np.stack([ref.solve(*mat, B[:, j], lower, unit) for j in range(kt)], axis=1) if n else np.zeros((0, kt))
    B.setflags(write=False)
    X.setflags(write=False)
    return B, X


LAYOUTS = (("row", 0), ("row", 3), ("col", 0), ("col", 5))                  # row-major with ld = k and k + 3, column-major with ld = n and n + 5


def empty_block(shape, layout, pad):
    """(storage, view): a device block of n × k in the given layout whose leading dimension is the smallest one plus `pad`; the storage holds the
    sentinel everywhere, the window included"""
    n, k = shape
    ld = (k if layout == "row" else n) + pad
    size = max(1, (n if layout == "row" else k) * ld)
    st = torch.full((size,), SENT, dtype=torch.int64, device="cuda").view(torch.float64)
    return st, torch.as_strided(st, (n, k), (ld, 1) if layout == "row" else (1, ld))


def block(data, layout, pad):
    """the same with `data` (n × k, numpy) in the window"""
    st, view = empty_block(data.shape, layout, pad)
    view.copy_(torch.from_numpy(np.array(data, np.float64)).cuda())          # a copy: the shared cases are read-only
    return st, view


def check_block(st, shape, layout, pad, want, what):
    """the window of the storage holds `want` bit for bit, everything else still the sentinel"""
    n, k = shape
    ld = (k if layout == "row" else n) + pad
    got = st.cpu().numpy().view(np.int64)
    i, j = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    at = (i * ld + j) if layout == "row" else (i + j * ld)
    assert np.array_equal(got[at], _bits(want)), (what, np.argwhere(got[at] != _bits(want))[:8].tolist())
    rest = np.ones(got.size, bool)
    rest[at.reshape(-1)] = False
    assert np.all(got[rest] == SENT), (what, "padding", np.flatnonzero(rest & (got != SENT))[:8].tolist())


def solve_checked(solve, data, want, what, layouts=LAYOUTS, in_place=True):
    """`solve(b, out)` on `data` in every layout, out of place and in place; the result is `want` by bits, the padding and (out of place) B untouched"""
    for layout, pad in layouts:
        bst, b = block(data, layout, pad)
        xst, x = empty_block(data.shape, layout, pad)
        assert solve(b, x) is x
        torch.cuda.synchronize()
        check_block(xst, data.shape, layout, pad, want, (what, layout, pad))
        check_block(bst, data.shape, layout, pad, data, (what, layout, pad, "B"))
        if in_place:
            assert solve(b, b) is b
            torch.cuda.synchronize()
            check_block(bst, data.shape, layout, pad, want, (what, layout, pad, "in place"))


def singles(solve, B):
    """the device's own single solves of the columns of B (numpy n × k), as numpy n × k"""
    n, k = B.shape
    cols = [solve(torch.from_numpy(np.array(B[:, j])).cuda()).cpu().numpy() for j in range(k)]
    return np.stack(cols, axis=1) if k else np.zeros((n, 0))


def _plan(mat, lower=True, unit=False, no_chains=False):
    from g4s_amd import host
    n, rp, ci, va = mat
    return host.sptrsv_analyse((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)), lower, unit, no_chains=no_chains)


CASE_NAMES = ("n0", "n1", "bidiagonal_cap_plus_1", "blocks", "grid40", "wave_row_edges", "hub_row", "strided_tiles", "wave_tiles", "messy")
PARAMS = [(name, lower, False) for name in CASE_NAMES for lower in (True, False)] + [("messy", True, True), ("messy", False, True)]


@pytest.mark.parametrize("name,lower,unit", PARAMS)
def test_block_equals_reference_and_single_solves(name, lower, unit):
    kt = _kt()
    mat, _, info, _, _ = ref.case(name, lower, unit)
    n = mat[0]
    B, X = rhs(name, lower, unit)
    plan = _plan(mat, lower, unit)
    assert {k: plan.info[k] for k in info} == info
    if n == 0:
        with pytest.raises(ValueError):
            plan.solve(torch.zeros(1, 3, dtype=torch.float64, device="cuda"))
    one = singles(plan.solve, B) if n else np.zeros((0, B.shape[1]))
    _same_bits(one[:, :kt], X, (name, "single solves against the reference"))
    for k in ([kt + 1] if name == "hub_row" else _ks()):
        # the reference's columns as far as they go (all of them up to k = KT), the device's own single solves for every column
        solve_checked(lambda b, x: plan.solve(b, out=x), B[:, :k], one[:, :k], (name, lower, unit, k))
    fresh = plan.solve(torch.from_numpy(np.array(B[:, :kt + 1])).cuda())    # a new out: allocated in b's layout
    assert fresh.stride() == (kt + 1, 1) or n <= 1
    _same_bits(fresh.cpu().numpy(), one[:, :kt + 1])
    cm = torch.from_numpy(np.array(B[:, :kt + 1].T, order="C")).cuda().t()
    fresh = plan.solve(cm)
    assert fresh.stride() == (1, n) or n <= 1
    _same_bits(fresh.cpu().numpy(), one[:, :kt + 1])
    plan.close()


@pytest.mark.parametrize("name", ["bidiagonal_cap_plus_1", "blocks", "grid40", "messy"])
def test_one_launch_per_level_gives_the_same_bits(name):
    kt = _kt()
    for lower in (True, False):
        mat, _, info, _, _ = ref.case(name, lower)
        B, X = rhs(name, lower)
        k = kt + 1
        with_chains, without = _plan(mat, lower), _plan(mat, lower, no_chains=True)
        assert with_chains.info["chains"] == info["chains"] and (info["chains"] > 0 or not lower)   # every lower triangle here has a chain
        assert without.info["chains"] == 0 and without.info["launches_per_solve"] == without.info["levels"]
        want = singles(with_chains.solve, B[:, :k])
        _same_bits(want[:, :kt], X)
        solve_checked(lambda b, x: without.solve(b, out=x), B[:, :k], want, (name, lower, "no chains"), layouts=(("row", 3), ("col", 5)))
        with_chains.close()
        without.close()


@pytest.mark.parametrize("name", ["grid40", "messy", "blocks"])
def test_columns_never_meet(name):
    """one column of B all NaN, one with an inf, the rest finite: the finite columns are their single solves, the NaN column the canonical NaN
    wherever the reference says NaN — everywhere, with a NaN in every b[i]"""
    kt = _kt()
    k = kt + 1
    for lower in (True, False):
        mat = ref.case(name, lower)[0]
        n = mat[0]
        B0, X = rhs(name, lower)
        B = np.array(B0[:, :k])
        nan_col, inf_col = 1, kt                                            # the inf sits in the tail tile, the NaN column inside the first
        B[:, nan_col] = np.nan
        B[n // 3, inf_col] = np.inf
        plan = _plan(mat, lower)
        want = np.array(B)
        for j in range(k):
            want[:, j] = X[:, j] if j < kt and j != nan_col else ref.solve(*mat, B[:, j], lower)
        assert np.all(np.isnan(want[:, nan_col])) and np.all(_bits(want[:, nan_col]) == QNAN) and not np.all(np.isfinite(want[:, inf_col]))
        finite = [j for j in range(k) if j not in (nan_col, inf_col)]
        assert np.all(np.isfinite(want[:, finite]))
        solve_checked(lambda b, x: plan.solve(b, out=x), B, want, (name, lower, "NaN and inf columns"))
        one = singles(plan.solve, B)
        _same_bits(one, want)
        plan.close()


def test_update_values_then_a_block_solve():
    kt = _kt()
    k = kt + 1
    for lower in (True, False):
        mat = ref.case("messy", lower)[0]
        n, rp, ci, va = mat
        B, X = rhs("messy", lower)
        new = np.random.default_rng(11).uniform(1.0, 2.0, va.size) * np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 8.0, 0.125)
        want = np.stack([ref.solve(n, rp, ci, new, B[:, j], lower) for j in range(k)], axis=1)
        assert not np.array_equal(want[:, :kt], X)
        plan = _plan(mat, lower)
        plan.update_values(_dev(new, np.float64))
        solve_checked(lambda b, x: plan.solve(b, out=x), B[:, :k], want, ("update_values", lower), layouts=(("row", 0), ("col", 5)))
        plan.close()


def test_block_solve_in_a_captured_graph():
    """the capture proves that the block solve waits for nothing and allocates nothing; replays on new contents of B equal the eager bits. The graph
    is linear and on one stream: launches_per_solve kernels, one after another."""
    kt = _kt()
    k = kt + 1
    for name, layout in (("blocks", "row"), ("grid40", "col")):
        mat = ref.case(name)[0]
        n = mat[0]
        B0, X = rhs(name)
        plan = _plan(mat)
        bst, b = block(B0[:, :k], layout, 2)
        xst, x = block(np.zeros((n, k)), layout, 2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                plan.solve(b, out=x)
        torch.cuda.current_stream().wait_stream(side)
        for it in range(2):
            Bk = B0[:, :k] if it == 0 else np.random.default_rng(40 + it).uniform(-1.0, 1.0, (n, k))
            b.copy_(torch.from_numpy(np.array(Bk)).cuda())
            x.copy_(torch.zeros(n, k, dtype=torch.float64, device="cuda"))
            g.replay()
            torch.cuda.synchronize()
            eager = plan.solve(b).cpu().numpy()
            check_block(xst, (n, k), layout, 2, eager, (name, it, "eager"))
            if it == 0:
                _same_bits(eager[:, :kt], X)
            else:
                _same_bits(eager[:, 0], ref.solve(*mat, Bk[:, 0]))
        plan.close()


def test_two_streams_on_one_handle():
    """two host threads, each with a stream of its own, enqueue block solves on ONE plan into different X at the same time: the block solve only
    reads the handle"""
    kt = _kt()
    k = kt + 1
    mat = ref.case("grid40")[0]
    B0, X = rhs("grid40")
    plan = _plan(mat)
    want0 = singles(plan.solve, B0[:, :k])
    _same_bits(want0[:, :kt], X)
    want1 = singles(plan.solve, 2.0 * B0[:, :k])
    torch.cuda.synchronize()
    errors = []

    def job(t):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            layout, data, want = (("row", B0[:, :k], want0), ("col", 2.0 * B0[:, :k], want1))[t]
            with torch.cuda.stream(s):
                for it in range(6):
                    bst, b = block(data, layout, 1)
                    xst, x = block(np.zeros_like(data), layout, 1)
                    plan.solve(b, out=x)
                    s.synchronize()
                    check_block(xst, data.shape, layout, 1, want, ("thread", t, it))
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=job, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    plan.close()
    assert not errors, errors


def test_c_refusals_with_a_real_handle_and_a_correct_call_behind_them():
    import ctypes as C
    from g4s_amd import capi, host
    lib = capi.load()
    mat = ref.case("messy")[0]
    n = mat[0]
    B, X = rhs("messy")
    k = _kt()
    plan = _plan(mat)
    bst, b = block(B[:, :k], "row", 0)
    xst, x = block(np.zeros((n, k)), "row", 0)
    fn, h, s = lib.g4s_sptrsv_solve_multi, plan._handle, host._stream()
    P = host._ptr
    for args in ((h, -1, P(b), k, P(x), k, 0, s), (h, capi.TRSV_MAX_RHS + 1, P(b), k, P(x), k, 0, s), (h, k, P(b), k, P(x), k, capi.TRSV_UPPER, s),
                 (h, k, None, k, P(x), k, 0, s), (h, k, P(b), k, None, k, 0, s), (h, k, P(b), k - 1, P(x), k, 0, s), (h, k, P(b), k, P(x), k, capi.TRSV_COL_MAJOR, s),
                 (h, k, P(b), k, P(b), k + 1, 0, s)):
        assert fn(*args) == capi.ERR_INVALID and "g4s_sptrsv_solve_multi" in lib.g4s_last_error().decode()
    assert fn(h, 0, None, 0, None, 0, 0, s) == capi.OK
    torch.cuda.synchronize()
    check_block(xst, (n, k), "row", 0, np.zeros((n, k)), "nothing was enqueued")
    capi.check(fn(h, k, P(b), k, P(x), k, 0, s))
    torch.cuda.synchronize()
    check_block(xst, (n, k), "row", 0, X, "behind the refusals")
    plan.close()


def test_spsolve_triangular_with_a_matrix_right_hand_side():
    from g4s_amd import host
    kt = _kt()
    for lower in (True, False):
        mat = ref.case("messy", lower)[0]
        n, rp, ci, va = mat
        B, X = rhs("messy", lower)
        got = host.spsolve_triangular((rp, ci, va), B[:, :kt], lower)       # numpy in, a device tensor of n × k out
        assert got.is_cuda and tuple(got.shape) == (n, kt)
        _same_bits(got.cpu().numpy(), X)
        got = host.spsolve_triangular((rp, ci, va), torch.from_numpy(np.array(B[:, :kt])).cuda(), lower)
        _same_bits(got.cpu().numpy(), X)
        one = host.spsolve_triangular((rp, ci, va), B[:, 0], lower)         # the vector form is what it was
        assert tuple(one.shape) == (n,)
        _same_bits(one.cpu().numpy(), X[:, 0])


def test_gauss_seidel_on_a_block():
    """one symmetric sweep on trsv_ref.exact_case, whose every intermediate is exact under any summation order — which is why the residual may come
    from g4s_spmm: every column equals the restatement's sweep of that column with =="""
    from g4s_amd import host
    mat = ref.exact_case()
    n, rp, ci, va = mat
    k = _kt() + 1
    rng = np.random.default_rng(5)
    B = rng.integers(-4, 5, (n, k)).astype(np.float64)
    X0 = rng.integers(-2, 3, (n, k)).astype(np.float64)
    want = np.stack([ref.gauss_seidel(*mat, B[:, j], X0[:, j], 1, True) for j in range(k)], axis=1)
    assert not np.array_equal(want, X0)
    A = host.CSR.from_host(rp, ci, va, n, n)
    for layout in ("row", "col"):
        _, x = block(X0, layout, 0)
        _, b = block(B, "row", 0)
        out = host.gauss_seidel(A, b, x, sweeps=1, symmetric=True)
        assert out is x and np.array_equal(x.cpu().numpy(), want), layout
    x1 = torch.from_numpy(np.array(X0[:, 0])).cuda()                        # the vector form is what it was
    host.gauss_seidel(A, torch.from_numpy(np.array(B[:, 0])).cuda(), x1, sweeps=1, symmetric=True)
    assert np.array_equal(x1.cpu().numpy(), want[:, 0])


def test_trsm_example_prints_the_reference_solution(tmp_path):
    exe = str(tmp_path / "trsm")
    _build_example("trsm.cpp", exe)
    n, rp, ci, va = ref.grid5(8)
    k = 3
    rows = np.repeat(np.arange(n), np.diff(rp))
    f = tmp_path / "grid8.mtx"
    f.write_text(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {ci.size}\n" + "".join(f"{i + 1} {j + 1} {x!r}\n" for i, j, x in zip(rows.tolist(), ci.tolist(), va.tolist())))
    for lower in (True, False):
        out = subprocess.run([exe, str(f), "lower" if lower else "upper", str(k)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        lines = out.stdout.splitlines()
        info = ref.info(n, rp, ci, va, lower)
        assert lines[0] == (f"n {n}, nnz_triangle {info['nnz_triangle']}, {info['levels']} levels, widest {info['widest_level']}, "
                            f"{info['launches_per_solve']} launches per solve, {info['chains']} chains")
        got = [l.split() for l in lines[1:]]
        assert [(int(i), int(j)) for i, j, _ in got] == [(i, j) for i in range(n) for j in range(k)]
        # the reader keeps each row's entries in file order, so T·1 is the sum the example forms left to right; column j is (j + 1) times it
        t1 = np.zeros(n)
        for i, c, v in zip(rows.tolist(), ci.tolist(), va.tolist()):
            if (c <= i) if lower else (c >= i):
                t1[i] += v
        want = np.stack([ref.solve(n, rp, ci, va, np.float64(j + 1) * t1, lower) for j in range(k)], axis=1)
        _same_bits(np.array([float.fromhex(x) for _, _, x in got]).reshape(n, k), want)
