"""g4s_csr_from_coo_* / g4s_csr_row_indices without a GPU: the numpy reference of tests/coo_ref.py against scipy and against a dictionary built in plain
Python (so that the yardstick of the GPU tests is pinned to something this project did not write), the fold order, the constants and the struct in
every layer, argument checking before any HIP call, the C++ forms of include/g4s/csr.hpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import coo_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_from_coo_symbolic", "g4s_csr_from_coo_numeric", "g4s_csr_row_indices")


def _triples(n, rows, cols, seed, distinct=False):
    rng = np.random.default_rng(seed)
    row, col = rng.integers(0, rows, n).astype(np.int32), rng.integers(0, cols, n).astype(np.int32)
    val = rng.permutation(n).astype(np.float64) + 1.0 if distinct else rng.integers(-8, 9, n).astype(np.float64)   # integers: every order gives the same sum
    return row, col, val


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def test_reference_equals_scipy_on_plus_and_on_the_pattern():
    rows, cols = 300, 40
    row, col, val = _triples(5000, rows, cols, 0)
    m = sp.coo_matrix((val, (row, col)), shape=(rows, cols)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    rp, ci, va, perm, longest = ref.from_coo(row, col, val, rows, cols, "plus")
    assert len(ci) < 5000 and longest > 1                             # the list does repeat positions
    assert np.array_equal(rp, m.indptr) and np.array_equal(ci, m.indices) and np.array_equal(_bits(va), _bits(m.data))
    prp, pci, pva, _, _ = ref.from_coo(row, col, None, rows, cols, "max")
    assert pva is None and np.array_equal(prp, m.indptr) and np.array_equal(pci, m.indices)
    assert np.array_equal(perm, np.lexsort((np.arange(5000), col, row)))
    assert np.array_equal(ref.row_indices(rp), m.tocoo().row)


@pytest.mark.parametrize("dup", ["keep", "min", "max", "first", "second", "plus", "times"])
def test_reference_equals_a_dictionary(dup):
    rows, cols = 4, 5
    row, col, val = _triples(400, rows, cols, 3, distinct=dup != "times")
    if dup == "times":
        val = np.where(val == 0.0, 1.0, val) / 4.0
    d = {}
    for i in range(400):
        d.setdefault((int(row[i]), int(col[i])), []).append(float(val[i]))
    want_c, want_v, want_rp = [], [], [0] * (rows + 1)
    for (r, c) in sorted(d):
        vs = d[(r, c)]
        if dup == "keep":
            out = vs
        elif dup == "min":
            out = [min(vs)]
        elif dup == "max":
            out = [max(vs)]
        elif dup == "first":
            out = [vs[0]]
        elif dup == "second":
            out = [vs[-1]]
        else:
            acc = vs[0]
            for x in vs[1:]:
                acc = acc + x if dup == "plus" else acc * x
            out = [acc]
        want_c += [c] * len(out)
        want_v += out
        want_rp[r + 1] += len(out)
    rp, ci, va, _, longest = ref.from_coo(row, col, val, rows, cols, dup)
    assert rp.tolist() == np.cumsum(want_rp).tolist() and ci.tolist() == want_c
    assert np.array_equal(_bits(va), _bits(want_v))
    assert longest == max(len(v) for v in d.values())


def test_fold_is_left_to_right():
    v = [1e16, 1.0, -1e16, 1.0]
    assert ref.fold("plus", v) == 1.0
    assert sum(sorted(v)) == 0.0 and (v[0] + v[1]) + (v[2] + v[3]) == 0.0 and ref.fold("plus", v[::-1]) == 0.0   # ascending value, pairwise, reversed
    rp, ci, va, _, longest = ref.from_coo([2, 2, 2, 2], [1, 1, 1, 1], v, 3, 2, "plus")
    assert rp.tolist() == [0, 0, 0, 1] and ci.tolist() == [1] and va.tolist() == [1.0] and longest == 4
    t = [1e200, 1e200, 1e-200, 1e-200]                                # times: inf from the left, 1.0 in pairs from the middle
    assert ref.fold("times", t) == float("inf") and ref.fold("times", [t[0], t[2], t[1], t[3]]) == 1.0


def test_empty_and_gaps():
    rp, ci, va, perm, longest = ref.from_coo([], [], [], 5, 3, "plus")
    assert rp.tolist() == [0] * 6 and len(ci) == 0 and len(va) == 0 and len(perm) == 0 and longest == 0
    rp, ci, va, _, _ = ref.from_coo([4, 1, 4], [0, 2, 0], [1.0, 2.0, 3.0], 6, 3, "second")
    assert rp.tolist() == [0, 0, 1, 1, 1, 2, 2] and ci.tolist() == [2, 0] and va.tolist() == [2.0, 3.0]


def test_constants_and_struct_agree_across_layers():
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    assert re.search(r"#define\s+G4S_DUP_KEEP\s+\(-1\)", text) and capi.DUP_KEEP == -1
    assert host.DUPLICATES == {"keep": capi.DUP_KEEP, **host.COMBINERS} and tuple(host.DUPLICATES) == ref.DUPLICATES
    assert C.sizeof(capi.CooInfo) == 64
    assert [n for n, _ in capi.CooInfo._fields_] == ["nnz_in", "nnz_out", "longest_run", "row_bits", "col_bits", "digit_bits", "sort_passes", "tile_entries",
                                                     "presorted", "host_waits", "reserved"]
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+%s\s*\(" % fn, text) and fn in capi.SIGNATURES and fn + "(" in hpp
    for name in ("struct graph", "FromGraph(", "FromCOO(", "ToCOO(", "SortAndMerge("):
        assert name in hpp, name
    assert "g4s_csr_from_coo_" in text.split("Different host threads may call at the same time")[1].split("Different streams from one thread")[0]


def test_symbols_are_exported():
    from g4s_amd import capi
    lib = capi.load()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn)


def test_from_coo_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    sym, num, rix = lib.g4s_csr_from_coo_symbolic, lib.g4s_csr_from_coo_numeric, lib.g4s_csr_row_indices
    f = C.c_void_p(0x1000)                                              # never dereferenced: every check below comes first
    n = C.c_int64(0)
    info = capi.CooInfo()
    sym_ok = lambda dup=0, rows=5, cols=5, nnz=7, row=f, col=f, crp=f, perm=f, cn=C.byref(n), flags=1: sym(dup, rows, cols, nnz, row, col, crp, perm, cn, flags, C.byref(info), None)
    num_ok = lambda dup=0, rows=5, cols=5, nnz=7, row=f, col=f, val=f, crp=f, perm=f, cci=f, cva=f, flags=1: num(dup, rows, cols, nnz, row, col, val, crp, perm, cci, cva, flags, None)
    rix_ok = lambda rows=5, nnz=7, rp=f, out=f, flags=1: rix(rows, nnz, rp, out, flags, None)
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20]:
        for base in (0, 1):
            assert sym_ok(flags=base | b) == capi.ERR_INVALID and num_ok(flags=base | b) == capi.ERR_INVALID and rix_ok(flags=base | b) == capi.ERR_INVALID, b
    assert "flags" in lib.g4s_last_error().decode()
    for dup in (-2, 6, 512, 1 << 20):
        assert sym_ok(dup=dup) == capi.ERR_INVALID and num_ok(dup=dup) == capi.ERR_INVALID
    assert "dup" in lib.g4s_last_error().decode()
    for kw in (dict(rows=-1), dict(cols=-1), dict(nnz=-1)):
        assert sym_ok(**kw) == capi.ERR_INVALID and num_ok(**kw) == capi.ERR_INVALID, kw
    assert "negative" in lib.g4s_last_error().decode()
    assert rix_ok(rows=-1) == capi.ERR_INVALID and rix_ok(nnz=-1) == capi.ERR_INVALID
    for nnz in (1 << 31, 1 << 40):
        assert sym_ok(nnz=nnz) == capi.ERR_OVERFLOW and num_ok(nnz=nnz) == capi.ERR_OVERFLOW and rix_ok(nnz=nnz) == capi.ERR_OVERFLOW
    assert "exceed" in lib.g4s_last_error().decode()
    for name in ("row", "col", "crp", "perm"):
        assert sym_ok(**{name: None}) == capi.ERR_INVALID, name
        assert num_ok(**{name: None}) == capi.ERR_INVALID, name
    assert sym_ok(cn=None) == capi.ERR_INVALID and num_ok(cci=None) == capi.ERR_INVALID
    assert sym_ok(nnz=0, crp=None) == capi.ERR_INVALID and sym_ok(nnz=0, perm=None) == capi.ERR_INVALID   # required whatever nnz is
    assert rix_ok(rp=None) == capi.ERR_INVALID and rix_ok(out=None) == capi.ERR_INVALID
    for kw in (dict(val=None), dict(cva=None)):                           # NULL value arrays: both or neither
        assert num_ok(**kw) == capi.ERR_INVALID
    assert "pattern-only" in lib.g4s_last_error().decode()
    # overlap, host pointers: an output on top of an input or of another output
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    row, col, val = np.array([0, 1, 2], np.int32), np.array([2, 1, 0], np.int32), np.array([1.0, 2.0, 3.0])
    crp, perm, big_i, big_d = np.zeros(4, np.int32), np.zeros(3, np.int32), np.zeros(16, np.int32), np.zeros(16, np.float64)
    for c_, p_ in ((row, perm), (crp, col), (big_i, P(big_i, 8)), (crp, P(crp, 12))):
        p_ = p_ if isinstance(p_, C.c_void_p) else P(p_)
        assert sym(0, 3, 3, 3, P(row), P(col), P(c_), p_, C.byref(n), 0, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    crp[:] = [0, 1, 2, 3]
    for out_c, out_v in ((row, big_d), (col, big_d), (big_i, val), (crp, big_d), (perm, big_d), (big_i, big_i)):   # the last: ccol on cval
        assert num(0, 3, 3, 3, P(row), P(col), P(val), P(crp), P(perm), P(out_c), P(out_v), 0, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    crp[3] = -1
    assert num(0, 3, 3, 3, P(row), P(col), P(val), P(crp), P(perm), P(big_i), P(big_d), 0, None) == capi.ERR_INVALID
    crp[3] = 4                                                            # more entries than triples
    assert num(0, 3, 3, 3, P(row), P(col), P(val), P(crp), P(perm), P(big_i), P(big_d), 0, None) == capi.ERR_INVALID
    assert "crpt[rows]" in lib.g4s_last_error().decode()
    rp = np.array([0, 1, 2, 3], np.int32)
    assert rix(3, 3, P(rp), P(rp, 4), 0, None) == capi.ERR_INVALID
    assert "overlap" in lib.g4s_last_error().decode()


def test_cpp_forms_compile(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, c;\n    g4s_coo_info info = {};\n    g4s::graph g = {0, 0, nullptr, nullptr, nullptr};\n"
           "    static_assert(sizeof(g4s_coo_info) == 64, \"g4s_coo_info\");\n    static_assert(G4S_DUP_KEEP == -1, \"G4S_DUP_KEEP\");\n"
           "    if (argc > 5) { g4s::FromGraph(g, c); g4s::FromGraph(g, c, G4S_COMBINE_MAX, &info); g4s::FromCOO<int32_t, double>(0, 0, 0, nullptr, nullptr, nullptr, c);\n"
           "        g4s::FromCOO<int32_t, double>(0, 0, 0, nullptr, nullptr, nullptr, c, G4S_DUP_KEEP, &info); int32_t r[1]; g4s::ToCOO(a, r);\n"
           "        g4s::SortAndMerge(a, c); g4s::SortAndMerge(a, c, G4S_COMBINE_MIN, &info);\n"
           "        int64_t n = 0; g4s_csr_from_coo_symbolic(G4S_DUP_KEEP, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &n, G4S_DEVICE_POINTERS, &info, nullptr);\n"
           "        g4s_csr_from_coo_numeric(G4S_COMBINE_PLUS, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, G4S_HOST_POINTERS, nullptr);\n"
           "        g4s_csr_row_indices(0, 0, nullptr, nullptr, G4S_HOST_POINTERS, nullptr); }\n"
           "    return (int)info.nnz_out * 0 + (int)(g.m + g.n) * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_python_value_errors_before_any_gpu_call():
    import types
    from g4s_amd import host
    sq = types.SimpleNamespace(rows=3, cols=3)
    for bad in ("sum", "", None, 0, "KEEP"):
        with pytest.raises(ValueError, match="dup"):
            host.csr_from_coo(None, None, dup=bad)
        with pytest.raises(ValueError, match="dup"):
            host.csr_canonical(sq, dup=bad)
        with pytest.raises(ValueError, match="dup"):
            host.CSR.canonical(sq, bad)
    with pytest.raises(ValueError, match="symmetric"):
        host.csr_from_coo(None, None, symmetric=1)
    with pytest.raises(ValueError, match="return_perm"):
        host.csr_from_coo(None, None, return_perm="yes")
    for kw in (dict(rows=-1), dict(cols=2.5), dict(rows=True)):
        with pytest.raises(ValueError, match="non-negative integer"):
            host.csr_from_coo(None, None, **kw)
    with pytest.raises(ValueError, match="square"):
        host.csr_from_coo(None, None, rows=3, cols=4, symmetric=True)
    for bad in (-1, 2.0, None):
        with pytest.raises(ValueError, match="nnz"):
            host.csr_row_indices(None, bad)
