"""The semiring SpMV interface without a GPU: the flag values in every layer, argument checking before any HIP call (G4S_ERR_INVALID), the Python
ValueErrors, and the C++ form of include/g4s/csr.hpp (compile only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header_flag_values():
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u", text)}


def test_accumulate_constant_matches_header_and_collides_with_nothing():
    from g4s_amd import capi
    d = _header_flag_values()
    assert d["SPMV_ACCUMULATE"] == capi.SPMV_ACCUMULATE == 2048
    acc = d["SPMV_ACCUMULATE"]
    assert acc & (acc - 1) == 0                                       # one bit
    others = {k: v for k, v in d.items() if k not in ("SPMV_ACCUMULATE",)}
    assert all(v & acc == 0 for v in others.values()), {k: v for k, v in others.items() if v & acc}
    for name in ("SEMIRING_PLUS_TIMES", "SEMIRING_MIN_PLUS", "SEMIRING_MAX_PLUS", "SEMIRING_OR_AND", "SEMIRING_MASK"):
        assert getattr(capi, name) == d[name]


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def _handle_less_cases(capi):
    bad_bits = [1, 2, 4, 8, 16, 32, 64, 128, 256, 4096, 1 << 31]
    return [capi.SEMIRING_MIN_PLUS | b for b in bad_bits] + [capi.SEMIRING_OR_AND | capi.SPMV_ACCUMULATE | capi.DEVICE_POINTERS]


def test_handle_form_rejects_flags_and_arguments_before_hip():
    capi, lib = _lib()
    x, y = (C.c_double * 4)(), (C.c_double * 4)()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: the flags are checked first
    for f in _handle_less_cases(capi):
        assert lib.g4s_spmv_semiring(fake, x, y, f, None) == capi.ERR_INVALID, f
    assert lib.g4s_spmv_semiring(None, x, y, capi.SEMIRING_MIN_PLUS, None) == capi.ERR_INVALID
    assert lib.g4s_spmv_semiring(None, x, y, capi.SEMIRING_MAX_PLUS | capi.SPMV_ACCUMULATE, None) == capi.ERR_INVALID
    assert "flags" in lib.g4s_last_error().decode() or "handle" in lib.g4s_last_error().decode()


def test_one_shot_rejects_flags_and_arguments_before_hip():
    capi, lib = _lib()
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    va = np.array([1.0, 2.0])
    x, y = np.zeros(2), np.zeros(2)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda f, rows=2, cols=2, rpp=P(rp), xp=P(x), yp=P(y): lib.g4s_spmv_semiring_csr_i32_f64(rows, cols, rpp, P(ci), P(va), xp, yp, f)
    for b in (2, 4, 32, 64, 128, 256, 4096, 1 << 20):
        assert call(capi.SEMIRING_MIN_PLUS | b) == capi.ERR_INVALID, b
    assert call(capi.SEMIRING_MIN_PLUS, rows=-1) == capi.ERR_INVALID
    assert call(capi.SEMIRING_MIN_PLUS, rpp=None) == capi.ERR_INVALID
    assert call(capi.SEMIRING_MIN_PLUS, yp=None) == capi.ERR_INVALID
    assert call(capi.SEMIRING_MIN_PLUS, xp=None) == capi.ERR_INVALID
    assert call(capi.SEMIRING_MIN_PLUS | capi.SPMV_ACCUMULATE, xp=P(y)) == capi.ERR_INVALID   # x aliases y
    assert call(capi.SEMIRING_OR_AND | capi.SPMV_ACCUMULATE | capi.SPMV_STREAM, rows=0) == capi.OK   # nothing to do: no HIP call either


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    for name in ("bogus", "min-plus", "", None, "MIN_PLUS"):
        with pytest.raises(ValueError, match="semiring"):
            host.spmv_semiring(None, None, semiring=name)             # (no matrix, no device: the name is checked first)
        with pytest.raises(ValueError, match="semiring"):
            host.CSR.spmv_semiring(None, None, semiring=name)
    with pytest.raises(ValueError, match="accumulate"):
        host.spmv_semiring(None, None, y=None, semiring="min_plus", accumulate=True)
    with pytest.raises(ValueError, match="accumulate"):
        host.CSR.spmv_semiring(None, None, semiring="or_and", accumulate=True)


PAIRS = {
    "plus_times": ("std::multiplies<double>()", "std::plus<double>()"),
    "min_plus": ("std::plus<double>()", "g4s::min_op<double>()"),
    "max_plus": ("std::plus<double>()", "g4s::max_op<double>()"),
    "or_and": ("std::logical_and<double>()", "std::logical_or<double>()"),
}


def _compile(tmp_path, src):
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)


def _program(body):
    return ("#include \"g4s/csr.hpp\"\n"
            "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    double x[4] = {0}, y[4] = {0};\n"
            f"    if (argc > 5) {{ {body} }}\n    return 0;\n}}\n")


@pytest.mark.parametrize("semiring", sorted(PAIRS))
def test_cpp_supported_pairs_compile(tmp_path, semiring):
    mul, add = PAIRS[semiring]
    r = _compile(tmp_path, _program(f"g4s::SpMVSemiring(a, x, y, {mul}, {add}); g4s::SpMVSemiring(a, x, y, {mul}, {add}, true);"))
    assert r.returncode == 0, r.stderr


def test_cpp_unsupported_pair_fails_with_the_list(tmp_path):
    r = _compile(tmp_path, _program("g4s::SpMVSemiring(a, x, y, std::minus<double>(), std::plus<double>());"))
    assert r.returncode != 0
    assert "device SpMV implements four (multop, addop) pairs only" in r.stderr, r.stderr[-2000:]
    assert "(std::plus, g4s::min_op)" in r.stderr and "(std::logical_and, std::logical_or)" in r.stderr


def test_cpp_alpha_beta_spmv_keeps_its_meaning(tmp_path):
    # SpMV(a, x, y, alpha, beta) is still the alpha/beta product: with integer literals too (as the NT arguments they convert to), and a functor pair
    # handed to SpMV does not turn it into the semiring form — that has its own name
    src = ("#include \"g4s/csr.hpp\"\n"
           "#include <type_traits>\n"
           "using Ab = void (*)(const g4s::CSR<int32_t, double> &, const double *, double *, double, double);\n"
           "static_assert(std::is_same<decltype(static_cast<Ab>(&g4s::SpMV<int32_t, double>)), Ab>::value, \"\");\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    double x[4] = {0}, y[4] = {0};\n"
           "    if (argc > 5) { g4s::SpMV<int32_t, double>(a, x, y, 1, 0); g4s::SpMV(a, x, y, 1.0, 0.0); g4s::SpMV(a, x, y); }\n    return 0;\n}\n")
    r = _compile(tmp_path, src)
    assert r.returncode == 0, r.stderr
    r = _compile(tmp_path, _program("g4s::SpMV(a, x, y, std::plus<double>(), g4s::min_op<double>());"))
    assert r.returncode != 0
