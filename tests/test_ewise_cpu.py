"""g4s_csr_ewise_* / g4s_csr_select_* without a GPU: the numpy oracle of tests/ewise_ref.py against scipy (so that the yardstick of the GPU tests is
pinned to something this project did not write), the constants and the struct in every layer, the exported symbols, argument checking before any HIP
call (G4S_ERR_INVALID), the C++ forms of include/g4s/csr.hpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests import ewise_ref as ref
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_ewise_symbolic", "g4s_csr_ewise_numeric", "g4s_csr_select_symbolic", "g4s_csr_select_numeric")


def _pair(rows, cols, seed):
    a = helpers.random_csr(rows, cols, 0.05, seed, empty_rows=(1, 4))
    b = helpers.random_csr(rows, cols, 0.05, seed + 1, empty_rows=(2, 4))
    shift = lambda m: (m[0], m[1], 1.0 + (m[2] + 1.0) / 2.0 * 0.999)     # values in [1, 2): no sum, product, min or max is zero
    return shift(a), shift(b)


def _triple(m):
    m = m.tocsr()
    m.sort_indices()
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64)


def _equal(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(np.asarray(got[2]).view(np.int64), np.asarray(want[2]).view(np.int64))


@pytest.mark.parametrize("rows,cols", [(60, 60), (200, 31), (17, 400)])
def test_oracle_equals_scipy(rows, cols):
    a, b = _pair(rows, cols, rows)
    A, B = helpers.to_scipy(*a, rows, cols), helpers.to_scipy(*b, rows, cols)
    _equal(ref.ewise(a, b, rows, cols, "union", "plus"), _triple(A + B))
    _equal(ref.ewise(a, b, rows, cols, "intersect", "times"), _triple(A.multiply(B)))
    _equal(ref.ewise(a, b, rows, cols, "union", "max"), _triple(A.maximum(B)))
    _equal(ref.ewise(a, b, rows, cols, "intersect", "min"), _triple(A.minimum(B)))   # scipy's minimum with an implicit 0 is 0: only shared positions stay
    pat = sp.csr_matrix((np.ones(len(b[1])), b[1], b[0]), shape=(rows, cols))
    _equal(ref.ewise(a, b, rows, cols, "intersect", "first"), _triple(A.multiply(pat)))
    _equal(ref.ewise(a, b, rows, cols, "intersect", "second"), _triple(B.multiply(sp.csr_matrix((np.ones(len(a[1])), a[1], a[0]), shape=(rows, cols)))))
    _equal(ref.ewise(a, b, rows, cols, "difference"), _triple(A - A.multiply(pat)))
    # difference and intersection split A
    _equal(ref.ewise(ref.ewise(a, b, rows, cols, "difference"), ref.ewise(a, b, rows, cols, "intersect", "first"), rows, cols, "union"), a)
    for k in (-cols, -3, -1, 0, 1, 2, cols):
        _equal(ref.select(a, rows, "tril", k), _triple(sp.tril(A, k)))
        _equal(ref.select(a, rows, "triu", k), _triple(sp.triu(A, k)))
    _equal(ref.select(a, rows, "offdiag"), _triple(A - sp.diags(A.diagonal(), shape=(rows, cols))))
    _equal(ref.select(a, rows, "gt", thr=1.5), _triple(A.multiply(A > 1.5)))
    _equal(ref.transpose(a, rows, cols), _triple(A.T))


def test_oracle_keeps_an_explicit_zero_where_scipy_does_not():
    a = (np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.array([1.5, 0.0, 2.0]))
    b = (np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([-1.5, 4.0]))
    got = ref.ewise(a, b, 2, 3, "union", "plus")
    assert got[0].tolist() == [0, 2, 3] and got[1].tolist() == [0, 2, 1] and got[2].tolist() == [0.0, 0.0, 6.0]
    S = helpers.to_scipy(*a, 2, 3) + helpers.to_scipy(*b, 2, 3)
    S.eliminate_zeros()
    assert S.nnz == 1                                                   # scipy: the cancelled sum and the stored zero are gone
    assert ref.ewise(a, b, 2, 3, "intersect", "times")[2].tolist() == [-2.25, 8.0]
    assert ref.ewise(a, b, 2, 3, "difference")[1].tolist() == [2]
    v = np.array([np.nan, 0.0, -0.0])
    m = (np.array([0, 3], np.int32), np.array([2, 2, 0], np.int32), v)
    assert ref.select_mask(*m, "nonzero").tolist() == [True, False, False]
    for p in ("gt", "ge", "lt", "le"):
        assert not ref.select_mask(*m, p, thr=0.0)[0]                    # NaN fails all four
    assert ref.select(m, 1, "tril", 1)[1].tolist() == [0] and ref.select(m, 1, "ge")[1].tolist() == [2, 0]


def test_constants_and_struct_agree_across_layers():
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_((?:EWISE|COMBINE|SELECT)_\w+)\s+(\d+)\s*$", text, re.M)}
    assert len(d) == 3 + 6 + 9
    for name, v in d.items():
        assert getattr(capi, name) == v, name
    assert {k: d["EWISE_" + k.upper()] for k in ref.OPS} == host.EWISE_OPS
    assert {k: d["COMBINE_" + k.upper()] for k in ref.COMBINERS} == host.COMBINERS
    assert {k: d["SELECT_" + k.upper()] for k in ref.PREDICATES} == host.SELECT_PREDICATES
    for group in ("EWISE", "COMBINE", "SELECT"):                          # dense from 0: the range checks of the library are lo <= x <= hi
        vals = sorted(v for k, v in d.items() if k.startswith(group))
        assert vals == list(range(len(vals)))
    assert C.sizeof(capi.EwiseInfo) == 48
    assert [n for n, _ in capi.EwiseInfo._fields_] == ["nnz_a", "nnz_b", "nnz_c", "units", "unit_entries", "rows_split", "host_waits", "reserved"]
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+%s\s*\(" % fn, text) and fn in capi.SIGNATURES and fn + "(" in hpp
    for name in ("EWiseAdd(", "EWiseMult(", "EWiseDifference(", "Select(", "Symmetrise("):
        assert hpp.count(name) >= 2, name                                # the function and the header comment's list
    assert "g4s_csr_ewise_" in text.split("Different host threads may call at the same time")[1].split("Different streams from one thread")[0]


def test_symbols_are_exported():
    from g4s_amd import capi
    lib = capi.load()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn)


def _arrays(rows=3):
    rp = np.array([0, 1, 2, 3][:rows + 1], np.int32)
    return rp, np.array([0, 1, 2], np.int32), np.array([1.0, 2.0, 3.0])


def test_ewise_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    sym, num = lib.g4s_csr_ewise_symbolic, lib.g4s_csr_ewise_numeric
    f = C.c_void_p(0x1000)                                              # never dereferenced: every check below comes first
    n = C.c_int64(0)
    info = capi.EwiseInfo()
    sym_ok = lambda op=0, rows=5, cols=5, arp=f, aci=f, brp=f, bci=f, crp=f, cn=C.byref(n), flags=1: sym(op, rows, cols, arp, aci, brp, bci, crp, cn, flags, C.byref(info), None)
    num_ok = lambda op=0, comb=0, rows=5, cols=5, arp=f, aci=f, ava=f, brp=f, bci=f, bva=f, crp=f, cci=f, cva=f, flags=1: num(op, comb, rows, cols, arp, aci, ava, brp, bci, bva, crp, cci, cva, flags, None)
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20]:
        for base in (0, 1):
            assert sym_ok(flags=base | b) == capi.ERR_INVALID and num_ok(flags=base | b) == capi.ERR_INVALID, b
    assert "flags" in lib.g4s_last_error().decode()
    for op in (-1, 3, 512, 1 << 20):
        assert sym_ok(op=op) == capi.ERR_INVALID and num_ok(op=op) == capi.ERR_INVALID
    assert "op" in lib.g4s_last_error().decode()
    for comb in (-1, 6, 1024):
        assert num_ok(comb=comb) == capi.ERR_INVALID
    assert "combine" in lib.g4s_last_error().decode()
    for kw in (dict(rows=-1), dict(cols=-1)):
        assert sym_ok(**kw) == capi.ERR_INVALID and num_ok(**kw) == capi.ERR_INVALID
    assert "negative" in lib.g4s_last_error().decode()
    for name in ("arp", "aci", "brp", "bci", "crp"):
        assert sym_ok(**{name: None}) == capi.ERR_INVALID, name
        assert num_ok(**{name: None}) == capi.ERR_INVALID, name
    assert sym_ok(cn=None) == capi.ERR_INVALID and num_ok(cci=None) == capi.ERR_INVALID
    assert sym_ok(rows=0, arp=None) == capi.ERR_INVALID                   # a rowptr is required even for rows == 0
    for mix in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):                   # NULL value arrays: all three or none
        kw = {("ava", "bva", "cva")[i]: None for i in mix}
        assert num_ok(**kw) == capi.ERR_INVALID, mix
    assert "pattern-only" in lib.g4s_last_error().decode()
    # overlap, host pointers (every length is known on the host): an output on top of an input
    rp, ci, va = _arrays()
    P = lambda a: C.c_void_p(a.ctypes.data)
    big_i, big_d = np.zeros(16, np.int32), np.zeros(16, np.float64)
    assert sym(0, 3, 3, P(rp), P(ci), P(rp), P(ci), P(rp), C.byref(n), 0, None, None) == capi.ERR_INVALID
    assert "overlap" in lib.g4s_last_error().decode()
    assert sym(0, 3, 3, P(rp), P(ci), P(rp), P(ci), P(ci), C.byref(n), 0, None, None) == capi.ERR_INVALID
    assert sym(0, 3, 3, P(rp), P(big_i), P(rp), P(ci), C.c_void_p(big_i.ctypes.data + 8), C.byref(n), 0, None, None) == capi.ERR_INVALID
    assert sym(0, 3, 3, P(rp), P(ci), P(rp), P(ci), P(rp), C.byref(n), 1, None, None) == capi.ERR_INVALID   # device pointers: crpt on a rowptr is known at once
    crp = np.array([0, 1, 2, 3], np.int32)
    for out_c, out_v in ((ci, big_d), (big_i, va), (rp, big_d), (crp, big_d), (big_i, C.c_void_p(big_i.ctypes.data)), (big_d, big_d)):
        pv = out_v if isinstance(out_v, C.c_void_p) else P(out_v)
        assert num(0, 0, 3, 3, P(rp), P(ci), P(va), P(rp), P(ci), P(va), P(crp), P(out_c), pv, 0, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    bad = np.array([0, 1, 2, -3], np.int32)
    assert sym(0, 3, 3, P(bad), P(ci), P(rp), P(ci), P(big_i), C.byref(n), 0, None, None) == capi.ERR_INVALID
    assert "negative entry count" in lib.g4s_last_error().decode()


def test_select_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    sym, num = lib.g4s_csr_select_symbolic, lib.g4s_csr_select_numeric
    f = C.c_void_p(0x1000)
    n = C.c_int64(0)
    sym_ok = lambda pred=0, rows=5, cols=5, rp=f, ci=f, va=f, crp=f, cn=C.byref(n), flags=1: sym(pred, 0, 0.0, rows, cols, rp, ci, va, crp, cn, flags, None)
    num_ok = lambda pred=0, rows=5, cols=5, rp=f, ci=f, va=f, crp=f, cci=f, cva=f, flags=1: num(pred, 0, 0.0, rows, cols, rp, ci, va, crp, cci, cva, flags, None)
    for b in [1 << k for k in range(1, 32)]:
        assert sym_ok(flags=b) == capi.ERR_INVALID and num_ok(flags=b | 1) == capi.ERR_INVALID
    assert "flags" in lib.g4s_last_error().decode()
    for pred in (-1, 9, 4096):
        assert sym_ok(pred=pred) == capi.ERR_INVALID and num_ok(pred=pred) == capi.ERR_INVALID
    assert "pred" in lib.g4s_last_error().decode()
    for kw in (dict(rows=-1), dict(cols=-1), dict(rp=None), dict(ci=None), dict(crp=None)):
        assert sym_ok(**kw) == capi.ERR_INVALID and num_ok(**kw) == capi.ERR_INVALID, kw
    assert sym_ok(cn=None) == capi.ERR_INVALID and num_ok(cci=None) == capi.ERR_INVALID
    for pred in range(4, 9):                                            # value predicates need val
        assert sym_ok(pred=pred, va=None) == capi.ERR_INVALID and num_ok(pred=pred, va=None, cva=None) == capi.ERR_INVALID
    assert "val" in lib.g4s_last_error().decode()
    assert num_ok(va=None) == capi.ERR_INVALID                            # cval without val
    rp, ci, va = _arrays()
    P = lambda a: C.c_void_p(a.ctypes.data)
    assert sym(0, 0, 0.0, 3, 3, P(rp), P(ci), None, P(rp), C.byref(n), 0, None) == capi.ERR_INVALID
    assert "overlap" in lib.g4s_last_error().decode()
    assert num(0, 0, 0.0, 3, 3, P(rp), P(ci), P(va), P(rp), P(ci), P(np.zeros(8)), 0, None) == capi.ERR_INVALID
    assert "overlap" in lib.g4s_last_error().decode()


def test_cpp_forms_compile(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, b, c;\n    g4s_ewise_info info = {};\n"
           "    static_assert(sizeof(g4s_ewise_info) == 48, \"g4s_ewise_info\");\n"
           "    if (argc > 5) { g4s::EWiseAdd(a, b, c); g4s::EWiseAdd(a, b, c, G4S_COMBINE_MAX, &info); g4s::EWiseMult(a, b, c); g4s::EWiseMult(a, b, c, G4S_COMBINE_MIN);\n"
           "        g4s::EWiseDifference(a, b, c); g4s::Select(a, c, G4S_SELECT_TRIL, -1); g4s::Select(a, c, G4S_SELECT_GT, 0, 0.5); g4s::Symmetrise(a, c);\n"
           "        g4s::Symmetrise(a, c, G4S_COMBINE_PLUS, true);\n"
           "        int64_t n = 0; g4s_csr_ewise_symbolic(G4S_EWISE_UNION, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n, G4S_DEVICE_POINTERS, &info, nullptr);\n"
           "        g4s_csr_select_symbolic(G4S_SELECT_DIAG, 0, 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr, &n, G4S_HOST_POINTERS, nullptr); }\n"
           "    return (int)info.units * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    sq, wide, other = types.SimpleNamespace(rows=3, cols=3), types.SimpleNamespace(rows=3, cols=4), types.SimpleNamespace(rows=4, cols=3)
    for bad in ("sum", "", None, 0, "UNION"):
        with pytest.raises(ValueError, match="op"):
            host.csr_ewise(sq, sq, op=bad)
        with pytest.raises(ValueError, match="op"):
            host.CSR.ewise(sq, sq, bad)
    for bad in ("add", None, 1):
        with pytest.raises(ValueError, match="combine"):
            host.csr_ewise(sq, sq, combine=bad)
        with pytest.raises(ValueError, match="combine"):
            host.csr_symmetrise(sq, combine=bad)
    with pytest.raises(ValueError, match="shape"):
        host.csr_ewise(wide, other)
    with pytest.raises(ValueError, match="shape"):
        host.CSR.ewise(sq, wide)
    for bad in ("lower", None, 3):
        with pytest.raises(ValueError, match="pred"):
            host.csr_select(sq, bad)
        with pytest.raises(ValueError, match="pred"):
            host.CSR.select(sq, bad)
    with pytest.raises(ValueError, match="k must"):
        host.csr_select(sq, "tril", k=1.5)
    with pytest.raises(ValueError, match="thr must"):
        host.csr_select(sq, "gt", thr="1")
    with pytest.raises(ValueError, match="square"):
        host.csr_symmetrise(wide)
    with pytest.raises(ValueError, match="square"):
        host.CSR.symmetrise(wide)
    with pytest.raises(ValueError, match="drop_diagonal"):
        host.csr_symmetrise(sq, drop_diagonal=1)
