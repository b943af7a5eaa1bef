"""The kernels of the gather/apply graph interface (g4s_amd/csrc/graph.hip) at every instantiation and on both sides of every selection threshold, on
the cases of tests/graph_cases.py (whose claimed properties, and whose reference, tests/test_graph_cases_cpu.py proves).

Every case reads the line the library prints under G4S_DEBUG and requires it to name exactly the kernel, template arguments and launch geometry that the
restated selection rule predicts: a case cannot drift onto another kernel unnoticed. Results: integer data must equal the oracle's exactly (every sum
is exact in any order); real data within the project's 1e-10·Σ|terms| of the oracle (dense, element) or 1e-12·Σ|terms| of the longdouble restatement
(quadratic form: ≈ 1 030 additions per thread plus the tree at m = 513 is ≈ 1.2e-13, so a dropped term does not fit). Outputs the contract says are not
read start NaN-filled; every dense and element call is made twice and must give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import graph_cases as gc

pytestmark = pytest.mark.gpu
TOL = 1e-10
QUAD_TOL = 1e-12
NAN = float("nan")


@pytest.fixture
def tell_tale(monkeypatch, capfd):
    """The dense / element lines the library printed (G4S_DEBUG) since the last call."""
    monkeypatch.setenv("G4S_DEBUG", "1")
    capfd.readouterr()

    def read():
        return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith(("g4s dense ", "g4s element mat-vec:"))]
    return read


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def _dev(arr, misaligned=False):
    """A device copy of arr that starts on a 16-byte boundary, or 8 bytes past one."""
    buf = torch.empty(arr.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:arr.size + 1] if misaligned else buf[:arr.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(arr).ravel()))
    assert v.data_ptr() % 16 == (8 if misaligned else 0)
    return v


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _compare(got, want, scale, kind, what):
    if kind == "int":
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert bad.size == 0, f"{what}: {bad.size} entries differ, first {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"
    else:
        err = np.abs(got - want)
        assert np.all(err <= TOL * scale + 1e-300), f"{what}: max rel err {np.max(err / (scale + 1e-300))}"     # (a NaN fails the comparison)


# ================================================================================================ dense products
def _forward(oracle, tell_tale, c, kind):
    capi, lib = _lib()
    xx, w = gc.dense_operands(c, kind)
    xd, wd = _dev(xx, c.misaligned), _dev(w)
    if c.kernel is None:                                              # M == 0 or K == 0: nothing is launched, nothing is written
        rd = _nan(64)
        capi.check(lib.g4s_dense_rows_times_matrix(c.M, c.N, c.K, xd.data_ptr(), wd.data_ptr(), rd.data_ptr(), None))
        assert tell_tale() == [] and bool(torch.isnan(rd).all())
        return
    outs = []
    for _ in range(2):
        rd = _nan(c.M, c.K)
        capi.check(lib.g4s_dense_rows_times_matrix(c.M, c.N, c.K, xd.data_ptr(), wd.data_ptr(), rd.data_ptr(), None))
        assert tell_tale() == [gc.forward_line(c.dispatch())]
        outs.append(rd)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the second call gives other bits"
    got = outs[0].cpu().numpy()
    if c.claims.get("zero_result"):
        assert np.all(got == 0.0)
    _compare(got, gc.oracle_dense(oracle, xx, w), gc.dense_scale(xx, w), kind, f"{c.name} {kind}")


def _grad(oracle, tell_tale, c, kind):
    capi, lib = _lib()
    M, N, K = c.M, c.N, c.K
    xx, w, g = gc.dense_operands(c, kind)
    xd, wd, gd = _dev(xx), _dev(w), _dev(g, c.misaligned)
    dxx_line = [gc.forward_line(c.dispatch())] if c.dispatch() is not None else []
    dw_line = [gc.dw_line(c.dw())] if c.dw() is not None else []

    def call(want_dxx, want_dw):
        dxx, dw = _nan(M, N), _nan(N, K)
        capi.check(lib.g4s_dense_rows_times_matrix_grad(M, N, K, xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), dxx.data_ptr() if want_dxx else None,
                                                        dw.data_ptr() if want_dw else None, None))
        assert tell_tale() == (dxx_line if want_dxx else []) + (dw_line if want_dw else [])
        return dxx, dw

    dxx, dw = call(True, True)
    dxx2, dw2 = call(True, True)
    assert np.array_equal(_bits(dxx), _bits(dxx2)) and np.array_equal(_bits(dw), _bits(dw2)), "the second call gives other bits"
    dxx_alone, untouched = call(True, False)
    assert np.array_equal(_bits(dxx), _bits(dxx_alone)) and bool(torch.isnan(untouched).all()), "dxx alone (dw NULL) differs from the joint call"
    untouched, dw_alone = call(False, True)
    assert np.array_equal(_bits(dw), _bits(dw_alone)) and bool(torch.isnan(untouched).all()), "dw alone (dxx NULL) differs from the joint call"
    got_dxx, got_dw = dxx.cpu().numpy(), dw.cpu().numpy()
    if c.claims.get("zero_result"):
        assert np.all(got_dxx == 0.0)
    want_dxx, want_dw = oracle.dense_rows_times_matrix_grad(xx, w, g)
    s_dxx, s_dw = gc.dense_grad_scales(xx, w, g)
    _compare(got_dxx, want_dxx, s_dxx, kind, f"{c.name} {kind} dxx")
    _compare(got_dw, want_dw, s_dw, kind, f"{c.name} {kind} dw")


@pytest.mark.parametrize("name", [c.name for c in gc.dense_cases()])
def test_dense_case(oracle, tell_tale, name):
    c = gc.dense_case(name)
    for kind in gc.KINDS:
        (_forward if c.mode == "forward" else _grad)(oracle, tell_tale, c, kind)


# ================================================================================================ element-block mat-vec
def _rows(arr2d, base):
    rows = (C.POINTER(C.c_double) * (arr2d.shape[0] + base))()
    for e in range(arr2d.shape[0]):
        rows[e + base] = arr2d[e].ctypes.data_as(C.POINTER(C.c_double))
    return rows


def _elem_reference(oracle, m, K, u):
    want = oracle.element_matvec(m.ien, m.id, K, u, m.neq, npe=m.npe, dof=m.dof)
    scale = oracle.element_matvec(m.ien, m.id, np.abs(K), np.abs(u), m.neq, npe=m.npe, dof=m.dof)
    owned = np.zeros(m.neq, bool)
    owned[m.id.ravel()] = True
    return want, scale, owned


@pytest.mark.parametrize("name", [c.name for c in gc.elem_cases() if c.kernel != "refused"])
def test_element_case_device(oracle, tell_tale, name):
    capi, lib = _lib()
    m = gc.mesh(name)
    line = gc.elem_line(gc.elem_dispatch(m.ien, m.nno, m.npe, m.dof))
    assert gc.elem_case(name).kernel in line
    ien, idmap = np.ascontiguousarray(m.ien), np.ascontiguousarray(m.id)
    for kind in gc.KINDS:
        K, u = gc.elem_operands(name, kind)
        want, scale, owned = _elem_reference(oracle, m, K, u)
        Kd, ud = _dev(K), _dev(u)
        h = C.c_void_p()
        capi.check(lib.g4s_elem_op_create(C.byref(h), len(ien), m.npe, m.dof, ien.ctypes.data, idmap.ctypes.data, m.nno, m.neq, Kd.data_ptr()))
        try:
            outs = []
            for _ in range(2):
                Aud = _nan(m.neq)                                     # beta == 0: Au is not read; equations without an owner must read 0
                capi.check(lib.g4s_elem_op_apply(h, ud.data_ptr(), Aud.data_ptr(), None))
                assert tell_tale() == [line]
                outs.append(Aud)
        finally:
            lib.g4s_elem_op_destroy(h)
        assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the second call gives other bits"
        got = outs[0].cpu().numpy()
        assert np.all(got[~owned] == 0.0)
        _compare(got, want, scale, kind, f"{name} {kind}")


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", [c.name for c in gc.elem_cases() if c.kernel != "refused"])
def test_element_case_through_spmm_dense(oracle, tell_tale, name, base):
    """The drop-in call with a registered ELEMENT_BLOCK_MATVEC pattern of the case's shape: the result starts at a non-zero r0 and must end at
    r0 + K·u (the callbacks accumulate), equations without an owner keep r0, the element matrices arrive as row pointers from slot 0 or 1."""
    capi, lib = _lib()
    m = gc.mesh(name)
    line = gc.elem_line(gc.elem_dispatch(m.ien, m.nno, m.npe, m.dof))
    ien, idmap = np.ascontiguousarray(m.ien), np.ascontiguousarray(m.id)

    @capi.FUN_GATHER
    def gather(e, a, ew, st, res):                                    # the registration key: never called by the device path
        raise RuntimeError("host callback must not run")

    @capi.FUN_APPLY
    def apply(e, ew, st, res):
        raise RuntimeError("host callback must not run")

    desc = capi.PatternDesc(kind=capi.PATTERN_ELEMENT_BLOCK_MATVEC, num_elems=len(ien), nodes_per_elem=m.npe, dof=m.dof, ien=ien.ctypes.data,
                            id=idmap.ctypes.data, nno=m.nno, neq=m.neq, edge_weight_base=base, static_weights=0)
    capi.check(lib.g4s_register_pattern(gather, apply, C.byref(desc)))
    try:
        for kind in gc.KINDS:
            K, u = gc.elem_operands(name, kind)
            want, scale, owned = _elem_reference(oracle, m, K, u)
            rng = np.random.default_rng(base)
            r0 = rng.integers(1, 4, m.neq).astype(np.float64) if kind == "int" else rng.uniform(0.5, 1.5, m.neq)
            res = r0.copy()
            rows = _rows(K, base)
            capi.check(lib.g4s_spmm_dense(len(ien), m.npe, C.cast(rows, C.c_void_p), u.ctypes.data, None, res.ctypes.data, gather, apply, None, 1))
            assert tell_tale() == [line]
            assert np.array_equal(res[~owned], r0[~owned]), "an equation without an owner was written"
            _compare(res, r0 + want, scale + np.abs(r0), kind, f"{name} {kind} base {base}")
    finally:
        capi.check(lib.g4s_unregister_pattern(gather, apply))


def test_element_op_refuses_dof_above_4():
    capi, lib = _lib()
    m = gc.mesh("dof5_refused")
    assert m.dof == 5
    h = C.c_void_p()
    st = lib.g4s_elem_op_create(C.byref(h), len(m.ien), m.npe, m.dof, np.ascontiguousarray(m.ien).ctypes.data, np.ascontiguousarray(m.id).ctypes.data,
                                m.nno, m.neq, None)
    assert st == capi.ERR_INVALID and not h.value and b"dof <= 4" in lib.g4s_last_error()
    ok = m._replace(dof=4, id=np.ascontiguousarray(m.id[:, :4]))     # the same mesh at dof = 4 is taken
    capi.check(lib.g4s_elem_op_create(C.byref(h), len(ok.ien), ok.npe, 4, np.ascontiguousarray(ok.ien).ctypes.data, ok.id.ctypes.data, ok.nno, m.neq, None))
    lib.g4s_elem_op_destroy(h)


# ================================================================================================ symmetric quadratic form
@pytest.mark.parametrize("name", [c.name for c in gc.quad_cases()])
def test_quadratic_form_case(name):
    """Integer data: result == r0 + the exact sums (r0 = (0.5, 0.25): the call accumulates). Real data, from zero: within 1e-12·Σ|terms| of the
    longdouble restatement, Σ|terms| from the absolute values of the inputs."""
    capi, lib = _lib()
    c = {q.name: q for q in gc.quad_cases()}[name]
    for kind in gc.KINDS:
        a, x, b = gc.quad_operands(c, kind)
        want = gc.ld_sym_quadratic_form(c.m, c.numbers, a, x, b)
        r0 = np.array([0.5, 0.25]) if kind == "int" else np.zeros(2)
        out = r0.copy()
        capi.check(lib.g4s_sym_quadratic_form(c.m, c.numbers, a.ctypes.data, x.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data))
        if kind == "int":
            assert np.array_equal(out, r0 + want.astype(np.float64)), (name, out, want)
        else:
            mag = gc.ld_sym_quadratic_form(c.m, c.numbers, a, x, b, magnitudes=True)
            err = np.abs(out.astype(gc.LD) - want)
            print(f"{name}: err / Σ|terms| = {[float(e / max(s, 1e-300)) for e, s in zip(err, mag)]}")
            assert np.all(err <= QUAD_TOL * mag + 1e-300), (name, out, want, mag)
