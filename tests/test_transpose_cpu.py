"""The transpose interface without a GPU: constants in every layer, argument checking before any HIP call (G4S_ERR_INVALID) for g4s_csr_transpose and
the transposed products, and the C++ form g4s::Transpose of include/g4s/csr.hpp (compile only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def test_flag_values_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u", text)}
    for name in ("HOST_POINTERS", "DEVICE_POINTERS", "SPMV_NO_NT", "SPMV_BLOCKED", "SPMV_STREAM", "SPMV_UPDATABLE", "SPMV_ACCUMULATE",
                 "SEMIRING_MIN_PLUS", "SEMIRING_MAX_PLUS", "SEMIRING_OR_AND", "SEMIRING_MASK"):
        assert getattr(capi, name) == d[name], name
    # the C++ header spells the pointer kind and the semirings through g4s.h's macros
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_csr_transpose(" in hpp and "G4S_HOST_POINTERS" in hpp
    for fn in ("g4s_csr_transpose", "g4s_csr_transpose_reserve", "g4s_csr_transpose_info", "g4s_spmv_transpose", "g4s_spmv_semiring_transpose"):
        assert re.search(r"g4s_status\s+" + fn + r"\(", text), fn
        assert fn in capi.SIGNATURES, fn


def test_symbols_are_exported():
    _, lib = _lib()
    for fn in ("g4s_csr_transpose", "g4s_csr_transpose_reserve", "g4s_csr_transpose_info", "g4s_spmv_transpose", "g4s_spmv_semiring_transpose"):
        assert hasattr(lib, fn), fn


def test_handle_products_reject_arguments_before_hip():
    capi, lib = _lib()
    x, y = (C.c_double * 4)(), (C.c_double * 4)()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: flags and aliasing are checked first
    bad_bits = [1, 2, 4, 8, 16, 32, 64, 128, 256, 4096, 1 << 20, 1 << 31]
    for b in bad_bits:
        for base in (capi.SEMIRING_MIN_PLUS, capi.SEMIRING_MAX_PLUS | capi.SPMV_ACCUMULATE, capi.SEMIRING_OR_AND):
            assert lib.g4s_spmv_semiring_transpose(fake, x, y, base | b, None) == capi.ERR_INVALID, (base, b)
    assert lib.g4s_spmv_semiring_transpose(None, x, y, capi.SEMIRING_MIN_PLUS, None) == capi.ERR_INVALID
    assert lib.g4s_spmv_transpose(None, x, y, 1.0, 0.0, None) == capi.ERR_INVALID
    assert lib.g4s_spmv_transpose(fake, x, x, 1.0, 0.0, None) == capi.ERR_INVALID                 # x aliases y
    assert "alias" in lib.g4s_last_error().decode()
    assert lib.g4s_spmv_semiring_transpose(fake, y, y, capi.SEMIRING_OR_AND, None) == capi.ERR_INVALID
    for xp, yp in ((None, y), (x, None), (None, None)):
        assert lib.g4s_spmv_transpose(None, xp, yp, 1.0, 0.0, None) == capi.ERR_INVALID
        assert lib.g4s_spmv_semiring_transpose(None, xp, yp, capi.SEMIRING_MIN_PLUS, None) == capi.ERR_INVALID
    assert lib.g4s_csr_transpose_reserve(None) == capi.ERR_INVALID
    assert lib.g4s_csr_transpose_info(None, C.byref(capi.CsrInfo())) == capi.ERR_INVALID
    assert lib.g4s_csr_transpose_info(fake, None) == capi.ERR_INVALID


def test_transpose_rejects_arguments_before_hip():
    capi, lib = _lib()
    rp = np.array([0, 1, 3], np.int32)
    ci = np.array([1, 0, 2], np.int32)
    va = np.array([1.0, 2.0, 3.0])
    trp, tci, tva, perm = np.zeros(4, np.int32), np.zeros(3, np.int32), np.zeros(3), np.zeros(3, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(rows=2, cols=3, nnz=3, rpp=P(rp), cip=P(ci), vap=P(va), trpp=P(trp), tcip=P(tci), tvap=P(tva), permp=P(perm), flags=capi.HOST_POINTERS):
        return lib.g4s_csr_transpose(rows, cols, nnz, rpp, cip, vap, trpp, tcip, tvap, permp, flags, None)

    for b in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1536, 2048, 4096, 1 << 20, 1 << 31):
        assert call(flags=b) == capi.ERR_INVALID, b
        assert call(flags=capi.DEVICE_POINTERS | b) == capi.ERR_INVALID, b
    assert call(rows=-1) == capi.ERR_INVALID
    assert call(cols=-1) == capi.ERR_INVALID
    assert call(nnz=-1) == capi.ERR_INVALID
    assert call(nnz=(1 << 31)) == capi.ERR_INVALID                                  # nnz > INT32_MAX
    assert "INT32_MAX" in lib.g4s_last_error().decode()
    assert call(rpp=None) == capi.ERR_INVALID
    assert call(trpp=None) == capi.ERR_INVALID
    assert call(cip=None) == capi.ERR_INVALID
    assert call(tcip=None) == capi.ERR_INVALID
    assert call(vap=None) == capi.ERR_INVALID                                        # tvalues without values
    assert "tvalues without values" in lib.g4s_last_error().decode()
    assert call(tvap=None) == capi.ERR_INVALID                                       # values without tvalues
    for f in (capi.HOST_POINTERS, capi.DEVICE_POINTERS):
        assert call(rpp=None, flags=f) == capi.ERR_INVALID


def _compile(tmp_path, src):
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)


def test_cpp_transpose_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "#include <type_traits>\n"
           "using Tr = void (*)(const g4s::CSR<int32_t, double> &, g4s::CSR<int32_t, double> &);\n"
           "static_assert(std::is_same<decltype(static_cast<Tr>(&g4s::Transpose<int32_t, double>)), Tr>::value, \"\");\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, at;\n"
           "    if (argc > 5) { g4s::Transpose(a, at); g4s::Transpose(at, a); }\n    return 0;\n}\n")
    r = _compile(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_python_value_errors_before_any_gpu_call():
    import pytest
    from g4s_amd import host
    for name in ("bogus", "min-plus", "", None):
        with pytest.raises(ValueError, match="semiring"):
            host.spmv_semiring_transpose(None, None, semiring=name)      # (no matrix, no device: the name is checked first)
        with pytest.raises(ValueError, match="semiring"):
            host.CSR.spmv_semiring_transpose(None, None, semiring=name)
    with pytest.raises(ValueError, match="accumulate"):
        host.spmv_semiring_transpose(None, None, y=None, semiring="min_plus", accumulate=True)
