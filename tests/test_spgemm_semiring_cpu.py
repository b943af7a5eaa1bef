"""The SpGEMM semiring interface without a GPU: the flag values in every layer, argument checking before any GPU call, and the C++ functor
mapping of include/g4s/csr.hpp (compile only)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header_defines():
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(SEMIRING_\w+)\s+(\d+)u", text)}


def test_capi_constants_match_header():
    from g4s_amd import capi
    d = _header_defines()
    assert set(d) == {"SEMIRING_PLUS_TIMES", "SEMIRING_MIN_PLUS", "SEMIRING_MAX_PLUS", "SEMIRING_OR_AND", "SEMIRING_MASK"}
    for name, value in d.items():
        assert getattr(capi, name) == value, name
    flags = [v for k, v in d.items() if k != "SEMIRING_MASK"]
    assert len(set(flags)) == 4 and all(v & ~d["SEMIRING_MASK"] == 0 for v in flags)
    others = [capi.HOST_POINTERS, capi.DEVICE_POINTERS, capi.SORT_OUTPUT, capi.SPMV_NO_NT, capi.SPMV_BLOCKED, capi.SPMV_STREAM, capi.DIST_LOOPBACK,
              capi.DIST_ALLGATHER, capi.SPMV_UPDATABLE, capi.SPMM_COL_MAJOR]
    assert all(v & d["SEMIRING_MASK"] == 0 for v in others)


def test_host_names_map_onto_the_flags():
    from g4s_amd import capi, host
    assert host.SEMIRINGS == {"plus_times": capi.SEMIRING_PLUS_TIMES, "min_plus": capi.SEMIRING_MIN_PLUS, "max_plus": capi.SEMIRING_MAX_PLUS,
                              "or_and": capi.SEMIRING_OR_AND}


@pytest.mark.parametrize("name", ["bogus", "min-plus", "", None, "PLUS_TIMES"])
def test_unknown_semiring_raises_before_any_gpu_call(name):
    from g4s_amd import host
    with pytest.raises(ValueError, match="semiring"):
        host.HashSpGEMM(None, None, semiring=name)                 # (no matrices, no device: the name is checked first)


PAIRS = {
    "plus_times": ("std::multiplies<double>()", "std::plus<double>()"),
    "min_plus": ("std::plus<double>()", "g4s::min_op<double>()"),
    "max_plus": ("std::plus<double>()", "g4s::max_op<double>()"),
    "or_and": ("std::logical_and<double>()", "std::logical_or<double>()"),
}


def _program(mul, add):
    return ("#include \"g4s/csr.hpp\"\n"
            "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a, b, c;\n"
            f"    if (argc > 5) g4s::HashSpGEMM(a, b, c, {mul}, {add});\n    return 0;\n}}\n")


def _compile(tmp_path, src):
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)


@pytest.mark.parametrize("semiring", sorted(PAIRS))
def test_cpp_supported_pairs_compile(tmp_path, semiring):
    r = _compile(tmp_path, _program(*PAIRS[semiring]))
    assert r.returncode == 0, r.stderr


def test_cpp_semiring_flags_of_the_pairs(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "static_assert(g4s::semiring_flag<std::multiplies<double>, std::plus<double>, double>::value == G4S_SEMIRING_PLUS_TIMES, \"\");\n"
           "static_assert(g4s::semiring_flag<std::plus<double>, g4s::min_op<double>, double>::value == G4S_SEMIRING_MIN_PLUS, \"\");\n"
           "static_assert(g4s::semiring_flag<std::plus<double>, g4s::max_op<double>, double>::value == G4S_SEMIRING_MAX_PLUS, \"\");\n"
           "static_assert(g4s::semiring_flag<std::logical_and<double>, std::logical_or<double>, double>::value == G4S_SEMIRING_OR_AND, \"\");\n"
           "static_assert(!g4s::semiring_flag<std::minus<double>, std::plus<double>, double>::supported, \"\");\n"
           "int main() { return g4s::min_op<double>()(2.0, 1.0) == 1.0 && g4s::max_op<double>()(2.0, 1.0) == 2.0 ? 0 : 1; }\n")
    r = _compile(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_cpp_unsupported_pair_fails_with_the_list(tmp_path):
    r = _compile(tmp_path, _program("std::minus<double>()", "std::plus<double>()"))
    assert r.returncode != 0
    assert "device SpGEMM implements four (multop, addop) pairs only" in r.stderr, r.stderr[-2000:]
    assert "(std::plus, g4s::min_op)" in r.stderr and "(std::logical_and, std::logical_or)" in r.stderr
