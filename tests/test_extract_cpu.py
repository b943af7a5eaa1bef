"""g4s_csr_extract_* without a GPU: the numpy reference of tests/extract_ref.py against scipy and against a dictionary built in plain Python (so that the
yardstick of the GPU tests is pinned to something this project did not write), the tie order on non-canonical rows, the constants and the struct in
every layer, argument checking before any HIP call, the C++ forms of include/g4s/csr.hpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests import extract_ref as ref
from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_extract_symbolic", "g4s_csr_extract_numeric")
INFO_FIELDS = ["nnz_a", "nnz_rows", "nnz_c", "units", "unit_entries", "j_kind", "rows_in_order", "rows_sorted_wave", "rows_sorted_lds", "rows_sorted_radix",
               "lds_sort_max", "host_waits", "reserved"]


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _canonical(rows, cols, density, seed):
    rng = np.random.default_rng(seed)
    m = sp.random(rows, cols, density=density, random_state=np.random.RandomState(seed), format="csr")
    m.sort_indices()
    m.data = rng.permutation(m.nnz).astype(np.float64) + 1.0           # distinct: a wrong gather shows
    return m


def test_reference_equals_scipy_on_unsorted_lists_with_repeats():
    m = _canonical(50, 40, 0.2, 0)
    rng = np.random.default_rng(1)
    for I, J in ((rng.integers(0, 50, 70), rng.integers(0, 40, 90)), (rng.permutation(50), rng.permutation(40)), (np.arange(50)[::-1], np.arange(0, 40, 3)),
                 (np.zeros(0, np.int64), np.arange(40)), (np.arange(50), np.zeros(0, np.int64))):
        want = m[I][:, J].tocsr()
        want.sort_indices()
        rp, ci, va, src = ref.extract(m.indptr, m.indices, m.data, 50, 40, I, J)
        assert np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices) and np.array_equal(_bits(va), _bits(want.data))
        assert np.array_equal(_bits(m.data[src]), _bits(va)) and np.array_equal(m.indices[src], np.asarray(J)[ci])
    rp, ci, va, _ = ref.extract(m.indptr, m.indices, m.data, 50, 40)    # None, None: the matrix itself
    assert np.array_equal(rp, m.indptr) and np.array_equal(ci, m.indices) and np.array_equal(_bits(va), _bits(m.data))
    rp, ci, va, _ = ref.extract(m.indptr, m.indices, None, 50, 40, [3, 3], None)
    assert va is None and np.array_equal(ci, np.tile(m.indices[m.indptr[3]:m.indptr[4]], 2))


def _dictionary(rowptr, colids, values, I, J):
    """C(p, q) from a dictionary (row, col) → [(stored position, value), …] of A: per output row the (q, stored position) order."""
    d = {}
    for r in range(len(rowptr) - 1):
        for e in range(rowptr[r], rowptr[r + 1]):
            d.setdefault((r, int(colids[e])), []).append((e, float(values[e])))
    crpt, ccol, cval = [0], [], []
    for r in I:
        for q, c in enumerate(J):
            for _, v in d.get((int(r), int(c)), []):                   # stored order inside one (row, column)
                ccol.append(q)
                cval.append(v)
        crpt.append(len(ccol))
    return crpt, ccol, cval


def test_reference_equals_a_dictionary():
    m = _canonical(50, 40, 0.25, 2)
    rng = np.random.default_rng(3)
    I, J = rng.integers(0, 50, 70), rng.integers(0, 40, 90)
    crpt, ccol, cval = _dictionary(m.indptr, m.indices, m.data, I, J)
    rp, ci, va, _ = ref.extract(m.indptr, m.indices, m.data, 50, 40, I, J)
    assert len(ci) > m.nnz                                             # the lists do repeat ids
    assert rp.tolist() == crpt and ci.tolist() == ccol and np.array_equal(_bits(va), _bits(cval))


def test_reference_tie_order_on_non_canonical_rows():
    rng = np.random.default_rng(4)
    rows, cols, per = 6, 5, 9                                           # 9 entries over 5 columns: every row repeats a column, in shuffled order
    rowptr = np.arange(rows + 1) * per
    colids = rng.integers(0, cols, rows * per)
    values = rng.permutation(rows * per).astype(np.float64) + 1.0
    assert any(np.any(np.diff(colids[r * per:(r + 1) * per]) < 0) for r in range(rows))
    I, J = [5, 0, 0, 3], [4, 1, 1, 0, 4]
    crpt, ccol, cval = _dictionary(rowptr, colids, values, I, J)
    rp, ci, va, src = ref.extract(rowptr, colids, values, rows, cols, I, J)
    assert rp.tolist() == crpt and ci.tolist() == ccol and np.array_equal(_bits(va), _bits(cval))
    for p in range(len(I)):                                             # equal q: ascending stored position
        q, e = ci[rp[p]:rp[p + 1]], src[rp[p]:rp[p + 1]]
        assert np.all((np.diff(q) > 0) | ((np.diff(q) == 0) & (np.diff(e) > 0)))


def test_symbols_are_exported():
    from g4s_amd import capi
    lib = capi.load()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn)


def test_constants_and_struct_agree_across_layers(tmp_path):
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert C.sizeof(capi.ExtractInfo) == 80 and [n for n, _ in capi.ExtractInfo._fields_] == INFO_FIELDS
    struct = text.split("typedef struct g4s_extract_info {")[1].split("} g4s_extract_info;")[0]
    assert re.findall(r"int(?:32|64)_t\s+(\w+)", struct) == INFO_FIELDS
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+%s\s*\(" % fn, text) and fn in capi.SIGNATURES and fn + "(" in hpp
    assert len(capi.SIGNATURES[FUNCTIONS[0]][1]) == 13 and len(capi.SIGNATURES[FUNCTIONS[1]][1]) == 16
    for name in ("Extract(", "SpRef(", "Permute(", "SubMatrix("):
        assert name in hpp, name
    for name in ("csr_extract", "csr_permute", "csr_induced_subgraph", "csr_submatrix"):
        assert hasattr(host, name) and hasattr(host.CSR, name[4:]), name
    assert "g4s_csr_extract_" in text.split("Different host threads may call at the same time")[1].split("Different streams from one thread")[0]
    src = ("#include <cstdio>\n#include \"g4s.h\"\nint main() { std::printf(\"%zu %d %d\\n\", sizeof(g4s_extract_info), (int)G4S_HOST_POINTERS, (int)G4S_DEVICE_POINTERS); return 0; }\n")
    f = tmp_path / "size.cpp"
    f.write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "size")])
    out = subprocess.run([str(tmp_path / "size")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(capi.ExtractInfo), capi.HOST_POINTERS, capi.DEVICE_POINTERS]


def test_extract_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    sym, num = lib.g4s_csr_extract_symbolic, lib.g4s_csr_extract_numeric
    f = C.c_void_p(0x1000)                                              # never dereferenced: every check below comes first
    n = C.c_int64(0)
    info = capi.ExtractInfo()
    sym_ok = lambda rows=5, cols=6, rpt=f, col=f, ni=3, I=f, nj=4, J=f, crp=f, cn=C.byref(n), flags=1: sym(rows, cols, rpt, col, ni, I, nj, J, crp, cn, flags, C.byref(info), None)
    num_ok = lambda rows=5, cols=6, rpt=f, col=f, val=f, ni=3, I=f, nj=4, J=f, crp=f, cci=f, cva=f, src=f, flags=1: num(rows, cols, rpt, col, val, ni, I, nj, J, crp, cci, cva, src, flags, C.byref(info), None)
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20]:
        for base in (0, 1):
            assert sym_ok(flags=base | b) == capi.ERR_INVALID and num_ok(flags=base | b) == capi.ERR_INVALID, b
    assert "flags" in lib.g4s_last_error().decode()
    for kw in (dict(rows=-1), dict(cols=-1), dict(ni=-1), dict(nj=-1)):
        assert sym_ok(**kw) == capi.ERR_INVALID and num_ok(**kw) == capi.ERR_INVALID, kw
        assert "negative" in lib.g4s_last_error().decode()
    for name in ("rpt", "col", "crp"):
        assert sym_ok(**{name: None}) == capi.ERR_INVALID and num_ok(**{name: None}) == capi.ERR_INVALID, name
        assert "NULL" in lib.g4s_last_error().decode()
    assert sym_ok(cn=None) == capi.ERR_INVALID and "cnnz" in lib.g4s_last_error().decode()
    assert num_ok(cci=None) == capi.ERR_INVALID and "ccol" in lib.g4s_last_error().decode()
    for call in (sym_ok, num_ok):                                        # NULL lists: every row / every column, and the count must say so
        assert call(I=None, ni=3) == capi.ERR_INVALID and "ni must equal rows" in lib.g4s_last_error().decode()
        assert call(J=None, nj=4) == capi.ERR_INVALID and "nj must equal cols" in lib.g4s_last_error().decode()
    for kw in (dict(val=None), dict(cva=None)):                           # NULL value arrays: both or neither
        assert num_ok(**kw) == capi.ERR_INVALID
        assert "pattern-only" in lib.g4s_last_error().decode()
    # overlap, host pointers: an output on top of an input or of another output
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    rpt, col, val = np.array([0, 1, 2, 3], np.int32), np.array([2, 1, 0], np.int32), np.array([1.0, 2.0, 3.0])
    I, J = np.array([2, 0, 1], np.int32), np.array([1, 2, 0], np.int32)
    crp, big_i, big_d, cn8 = np.zeros(4, np.int32), np.zeros(16, np.int32), np.zeros(16, np.float64), np.zeros(2, np.int64)
    for out_crp, out_cn in ((rpt, cn8), (col, cn8), (I, cn8), (J, cn8), (P(rpt, 12), cn8), (cn8.view(np.int32), cn8)):
        out_crp = out_crp if isinstance(out_crp, C.c_void_p) else P(out_crp)
        assert sym(3, 3, P(rpt), P(col), 3, P(I), 3, P(J), out_crp, C.cast(P(out_cn), capi.i64p), 0, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    crp[:] = [0, 1, 2, 3]
    for out_c, out_v, out_s in ((col, big_d, None), (I, big_d, None), (J, big_d, None), (crp, big_d, None), (rpt, big_d, None), (big_i, val, None),
                                (big_i, big_i, None), (big_i, big_d, big_i), (big_i, big_d, col), (big_i, big_d, P(big_d, 16))):   # ccol on cval, src on ccol, …
        out_s = out_s if isinstance(out_s, C.c_void_p) or out_s is None else P(out_s)
        assert num(3, 3, P(rpt), P(col), P(val), 3, P(I), 3, P(J), P(crp), P(out_c), P(out_v), out_s, 0, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    crp[3] = -1
    assert num(3, 3, P(rpt), P(col), P(val), 3, P(I), 3, P(J), P(crp), P(big_i), P(big_d), None, 0, None, None) == capi.ERR_INVALID
    assert "negative" in lib.g4s_last_error().decode()


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    sq, rect = types.SimpleNamespace(rows=3, cols=3), types.SimpleNamespace(rows=3, cols=4)
    for name in ("pattern_only", "return_src", "return_info"):
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match=name):
                host.csr_extract(sq, **{name: bad})
            with pytest.raises(ValueError, match=name):
                host.CSR.extract(sq, **{name: bad})
    import torch
    for bad in (np.arange(3, dtype=np.int32), [0, 1], torch.arange(3, dtype=torch.int32), torch.arange(3), torch.zeros((2, 2), dtype=torch.int32)):   # not a device tensor, not int32, not a vector
        with pytest.raises(ValueError, match="I must be"):
            host.csr_extract(sq, I=bad)
        with pytest.raises(ValueError, match="J must be"):
            host.CSR.extract(sq, None, bad)
    with pytest.raises(ValueError, match="square"):
        host.csr_permute(rect, np.arange(3))
    with pytest.raises(ValueError, match="square"):
        host.CSR.permute(rect, np.arange(3))
    for bad in (None, types.SimpleNamespace(numel=lambda: 2), types.SimpleNamespace(numel=lambda: 4)):
        with pytest.raises(ValueError, match="perm must hold 3 ids"):
            host.csr_permute(sq, bad)
    with pytest.raises(ValueError, match="square"):
        host.csr_induced_subgraph(rect, None)
    import torch
    with pytest.raises(ValueError, match="mask must hold 3 flags"):
        host.csr_induced_subgraph(sq, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask must hold 3 flags"):
        host.CSR.induced_subgraph(sq, torch.zeros(2, dtype=torch.bool))
    for kw in (dict(M=-1, N=1), dict(M=1, N=2.0), dict(M=True, N=1), dict(M=1, N=1, M_start=-1), dict(M=1, N=1, N_start="0")):
        with pytest.raises(ValueError, match="non-negative integer"):
            host.csr_submatrix(rect, **kw)
    for kw in (dict(M=4, N=1), dict(M=1, N=5), dict(M=2, N=2, M_start=2), dict(M=2, N=2, N_start=3)):
        with pytest.raises(ValueError, match="leaves the 3 x 4 matrix"):
            host.csr_submatrix(rect, **kw)
        with pytest.raises(ValueError, match="leaves the 3 x 4 matrix"):
            host.CSR.submatrix(rect, **kw)


CPP_FORMS = ("#include <vector>\n#include \"g4s/csr.hpp\"\n"
             "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, c;\n    g4s_extract_info info = {};\n    std::vector<int32_t> ri, ci, src;\n"
             "    static_assert(sizeof(g4s_extract_info) == 80, \"g4s_extract_info\");\n"
             "    if (argc > 5) { c = g4s::Extract(a, ri, ci); c = g4s::Extract(a, ri, ci, &src, &info); c = g4s::SpRef(a, ri, ci); c = g4s::Permute(a, ri);\n"
             "        c = g4s::SpRef2(a, ri.data(), (int32_t)ri.size(), ci.data(), (int32_t)ci.size()); c = g4s::SubMatrix(a, 0, 0, 0, 0); c = g4s::SubMatrix(a, 0, 0);\n"
             "        int64_t n = 0; g4s_csr_extract_symbolic(0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, &n, G4S_DEVICE_POINTERS, &info, nullptr);\n"
             "        g4s_csr_extract_numeric(0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, G4S_HOST_POINTERS, &info, nullptr); }\n"
             "    return (int)info.nnz_c * 0 + (int)c.nnz * 0;\n}\n")


def test_cpp_forms_compile(tmp_path):
    f = tmp_path / "prog.cpp"
    f.write_text(CPP_FORMS)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_examples_build(tmp_path):
    _build_example("induced_subgraph.cpp", str(tmp_path / "induced_subgraph"))
    f = tmp_path / "forms.cpp"                                           # the helper resolves its source under examples/: hand it the way from there
    f.write_text(CPP_FORMS)
    _build_example(os.path.relpath(str(f), os.path.join(ROOT, "examples")), str(tmp_path / "forms"))
