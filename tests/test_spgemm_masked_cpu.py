"""g4s_spgemm_masked / g4s_triangle_count without a GPU: the symbols in every layer, argument checking before any HIP call (G4S_ERR_INVALID), the
C++ forms of include/g4s/csr.hpp (compile only), the Python ValueErrors, and the numpy reference of tests/masked_ref.py against scipy and against
the oracle's SpGEMM restricted to the mask — so that the yardstick of the GPU tests is pinned to something this project did not write."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers, masked_ref, semiring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_spgemm_masked", "g4s_triangle_count")


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def test_declared_in_every_layer():
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+" + fn + r"\s*\(", text), fn
        assert fn in capi.SIGNATURES, fn
    assert len(capi.SIGNATURES["g4s_spgemm_masked"][1]) == 15 and len(capi.SIGNATURES["g4s_triangle_count"][1]) == 7
    assert "typedef struct g4s_masked_info" in text
    assert C.sizeof(capi.MaskedInfo) == 32
    assert [n for n, _ in capi.MaskedInfo._fields_] == ["mask_nnz", "products", "rows_wave", "rows_lds", "rows_global", "rows_split"]
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_spgemm_masked(" in hpp and "g4s_triangle_count(" in hpp
    assert callable(host.spgemm_masked) and callable(host.triangle_count) and callable(host.CSR.triangle_count)
    # no new flag bits: the header defines none between the traversal's and nothing named after the mask
    assert not re.search(r"#define\s+G4S_MASK(ED)?_", text)


def test_symbols_are_exported():
    _, lib = _lib()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn), fn
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "g4s_amd", "lib", "libg4s_hip.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(FUNCTIONS) <= exported


def test_masked_rejects_arguments_before_hip():
    capi, lib = _lib()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.MaskedInfo()
    fn = lib.g4s_spgemm_masked

    def call(M=4, K=4, N=4, arpt=fake, acol=fake, aval=fake, brpt=fake, bcol=fake, bval=fake, mrpt=fake, mcol=fake, cval=fake, flags=0, info_p=None):
        return fn(M, K, N, arpt, acol, aval, brpt, bcol, bval, mrpt, mcol, cval, flags, info_p, None)

    ok_flags = (0, capi.DEVICE_POINTERS, capi.SEMIRING_MIN_PLUS, capi.SEMIRING_MAX_PLUS | capi.DEVICE_POINTERS, capi.SEMIRING_OR_AND)
    for b in (2, 4, 8, 16, 32, 64, 128, 256, 2048, 4096, 8192, 16384, 32768, 1 << 20, 1 << 31):
        for base in ok_flags:
            assert call(flags=base | b, info_p=C.byref(info)) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in ok_flags:
        for name in ("arpt", "acol", "brpt", "bcol", "mrpt", "mcol", "cval"):
            assert call(flags=f, **{name: None}) == capi.ERR_INVALID, name
        assert call(flags=f, aval=None) == capi.ERR_INVALID           # one value array without the other
        assert "pattern-only" in lib.g4s_last_error().decode()
        assert call(flags=f, bval=None) == capi.ERR_INVALID
        for name in ("M", "K", "N"):
            assert call(flags=f, **{name: -1}) == capi.ERR_INVALID, name
        assert "negative" in lib.g4s_last_error().decode()


def test_triangle_count_rejects_arguments_before_hip():
    capi, lib = _lib()
    fake = C.c_void_p(0x1000)
    count = C.c_int64(-7)
    fn = lib.g4s_triangle_count
    for b in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1536, 2048, 4096, 8192, 16384, 1 << 20, 1 << 31):
        for base in (0, capi.DEVICE_POINTERS):
            assert fn(4, fake, fake, C.byref(count), base | b, None, None) == capi.ERR_INVALID, (base, b)
    for f in (0, capi.DEVICE_POINTERS):
        assert fn(4, None, fake, C.byref(count), f, None, None) == capi.ERR_INVALID
        assert fn(4, fake, None, C.byref(count), f, None, None) == capi.ERR_INVALID
        assert fn(4, fake, fake, None, f, None, None) == capi.ERR_INVALID
        assert fn(-1, fake, fake, C.byref(count), f, None, None) == capi.ERR_INVALID
    assert count.value == -7                                          # a refused call writes nothing


def test_cpp_forms_compile(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, b, m, c;\n    g4s_masked_info info;\n    info.rows_wave = 0;\n    long long t = 0;\n"
           "    if (argc > 5) {\n"
           "        g4s::MaskedSpGEMM(a, b, m, c);\n"
           "        g4s::MaskedSpGEMM(a, b, m, c, std::multiplies<double>(), std::plus<double>(), &info);\n"
           "        g4s::MaskedSpGEMM(a, b, m, c, std::plus<double>(), g4s::min_op<double>());\n"
           "        g4s::MaskedSpGEMM(a, b, m, c, std::plus<double>(), g4s::max_op<double>());\n"
           "        g4s::MaskedSpGEMM(a, b, m, c, std::logical_and<double>(), std::logical_or<double>());\n"
           "        t = g4s::TriangleCount(a) + g4s::TriangleCount(a, &info);\n"
           "        g4s_spgemm_masked(1, 1, 1, a.rowptr, a.colids, nullptr, b.rowptr, b.colids, nullptr, m.rowptr, m.colids, c.values,\n"
           "                          G4S_DEVICE_POINTERS | G4S_SEMIRING_OR_AND, &info, nullptr);\n"
           "    }\n"
           "    return (int)t + info.rows_wave;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bad = tmp_path / "bad.cpp"                                        # an unsupported functor pair is refused at compile time
    bad.write_text("#include \"g4s/csr.hpp\"\nint main()\n{\n    g4s::CSR<int32_t, double> a, c;\n"
                   "    g4s::MaskedSpGEMM(a, a, a, c, std::minus<double>(), std::plus<double>());\n    return 0;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-c", "-I" + INCLUDE, str(bad), "-o", str(tmp_path / "bad.o")], capture_output=True, text=True)
    assert r.returncode != 0 and "four (multop, addop) pairs" in r.stderr


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    for name in ("bogus", "PLUS_TIMES", "", None, 3):
        with pytest.raises(ValueError, match="semiring"):
            host.spgemm_masked(None, None, None, semiring=name)       # (no matrices, no device: the name is checked first)


def test_reference_equals_scipy_and_the_oracle(oracle):
    """mask = A on the power-law square of the GPU tests: both branches of the lookup are exercised, plus-times agrees with scipy's A @ A at the mask
    positions, and with the oracle's SpGEMM restricted to the mask"""
    n = 6000
    A = helpers.power_law_csr(n, n, 23, 1500)
    mask = (A[0], A[1])
    val, hit = masked_ref.spgemm_masked(A, A, n, n, mask, "plus_times")
    assert val.size == 207804 and int(hit.sum()) == 174195
    assert np.all(val[~hit] == 0.0)
    S = helpers.to_scipy(*A, n, n)
    rows = masked_ref.mask_rows(A[0])
    want = np.asarray((S @ S).tocsr()[rows, A[1]]).ravel()
    scale = masked_ref.abs_sums(A, A, n, n, mask)
    assert np.all(np.abs(val - want) <= 1e-10 * scale)
    assert np.abs(val - want).max() < 1e-13
    orpt, ocol, oval = oracle.spgemm(A, A, n, sort_output=True)
    okey = masked_ref.mask_rows(orpt) * n + ocol
    mkey = rows * n + A[1]
    pos = np.searchsorted(okey, mkey)
    ohit = (pos < okey.size) & (okey[np.minimum(pos, okey.size - 1)] == mkey)
    assert np.array_equal(ohit, hit)
    assert np.all(np.abs(val[hit] - oval[pos[hit]]) <= 1e-10 * scale[hit])
    # the three exact semirings and pattern-only: identity off the product's pattern, the full reference's value on it
    for name in ("min_plus", "max_plus", "or_and"):
        v, h = masked_ref.spgemm_masked(A, A, n, n, mask, name)
        assert np.array_equal(h, hit) and np.all(v[~h] == masked_ref.IDENTITY[name])
        full = semiring_ref.spgemm(A, A, n, name)[2]
        assert np.array_equal(v[h], full[pos[h]])
    cnt, h = masked_ref.spgemm_masked(A, A, n, n, mask, "plus_times", pattern_only=True)
    P = (abs(S).sign() @ abs(S).sign()).tocsr()
    assert np.array_equal(cnt, np.asarray(P[rows, A[1]]).ravel()) and np.array_equal(cnt > 0, hit)
    marks, _ = masked_ref.spgemm_masked(A, A, n, n, mask, "or_and", pattern_only=True)
    assert np.array_equal(marks, hit.astype(np.float64))


def test_triangle_references_agree():
    rp, ci, _ = helpers.power_law_csr(4000, 4000, 31, 800)
    G = masked_ref.symmetric_simple_graph(rp, ci, 4000)
    assert G.nnz == 2 * 100398 and np.diff(G.indptr).max() == 831
    assert masked_ref.triangles_trace(G) == masked_ref.triangles_lower(G) == 298117
    import scipy.sparse as sp
    K = sp.csr_matrix(np.ones((30, 30)) - np.eye(30))
    assert masked_ref.triangles_trace(K) == masked_ref.triangles_lower(K) == 30 * 29 * 28 // 6
