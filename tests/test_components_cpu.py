"""g4s_connected_components without a GPU: the flag and struct in every layer, the exported symbol, argument checking before any HIP call
(G4S_ERR_INVALID), the C++ form of include/g4s/csr.hpp (compile only), the Python ValueErrors, and the numpy reference of tests/components_ref.py
against scipy.sparse.csgraph.connected_components — so that the yardstick of the GPU tests is pinned to something this project did not write."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import components_ref, helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# (density · n, seed) → (components, largest, rounds of the reference): from "no giant component" to "almost one component"
RANDOM_GRAPHS = {(0.5, 1): (25004, 1119, 58), (1, 2): (8164, 39780, 15), (2, 3): (956, 49007, 9), (4, 4): (17, 49984, 7)}


def test_flag_and_struct_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u\b", text)}
    assert d["CC_SYMMETRIC"] == 32768 == capi.CC_SYMMETRIC
    for k, v in d.items():                                            # the bit is nobody else's
        assert k == "CC_SYMMETRIC" or not (v & 32768), k
    assert re.search(r"g4s_status\s+g4s_connected_components\s*\(", text)
    assert "g4s_connected_components" in capi.SIGNATURES
    assert C.sizeof(capi.CCInfo) == 40
    assert [n for n, _ in capi.CCInfo._fields_] == ["components", "largest", "edges_linked", "largest_label", "sample_rounds", "skipped", "host_waits"]
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_connected_components(" in hpp and hpp.count("ConnectedComponents(") >= 2   # the function and the header comment's list


def test_symbol_is_exported():
    from g4s_amd import capi
    assert hasattr(capi.load(), "g4s_connected_components")


def test_call_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_connected_components
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.CCInfo()
    bits = [1 << k for k in range(32) if (1 << k) not in (1, 32768)]
    for b in bits + [1536, 3 << 20]:
        for base in (0, 1, 32768, 32769):
            assert fn(5, fake, fake, fake, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (0, 1, 32768, 32769):
        assert fn(5, None, fake, fake, f, None, None) == capi.ERR_INVALID
        assert fn(5, fake, fake, None, f, None, None) == capi.ERR_INVALID
        assert fn(5, fake, None, fake, f, None, None) == capi.ERR_INVALID
        assert "colids" in lib.g4s_last_error().decode()
        assert fn(-1, fake, fake, fake, f, None, None) == capi.ERR_INVALID
        assert "negative" in lib.g4s_last_error().decode()
        assert fn(0, None, None, fake, f, None, None) == capi.ERR_INVALID     # rowptr is required even for n == 0


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    int32_t l[4];\n    g4s_cc_info info = {};\n"
           "    static_assert(sizeof(g4s_cc_info) == 40, \"g4s_cc_info\");\n"
           "    if (argc > 5) { g4s::ConnectedComponents(a, l); g4s::ConnectedComponents(a, l, true); g4s::ConnectedComponents(a, l, false, &info);\n"
           "        g4s_connected_components(0, nullptr, nullptr, l, G4S_DEVICE_POINTERS | G4S_CC_SYMMETRIC, &info, nullptr); }\n"
           "    return (int)info.components * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    wide = types.SimpleNamespace(rows=3, cols=4)                      # no device arrays: the shape is checked first
    square = types.SimpleNamespace(rows=3, cols=3)
    with pytest.raises(ValueError, match="square"):
        host.connected_components(wide)
    with pytest.raises(ValueError, match="square"):
        host.CSR.connected_components(wide)
    for bad in ("yes", 1, 0, None, 2.0):
        with pytest.raises(ValueError, match="symmetric"):
            host.connected_components(square, symmetric=bad)
        with pytest.raises(ValueError, match="symmetric"):
            host.CSR.connected_components(square, symmetric=bad)
    with pytest.raises(ValueError, match="pair"):
        host.connected_components((np.zeros(1, np.int32),))
    with pytest.raises(ValueError, match="rowptr"):
        host.connected_components((np.zeros(0, np.int32), np.zeros(0, np.int32)))


@pytest.mark.parametrize("case", sorted(RANDOM_GRAPHS))
def test_reference_equals_scipy(case):
    d, seed = case
    n = 50000
    rp, ci, _ = helpers.random_csr(n, n, d / n, seed)
    lab, rounds = components_ref.labels(rp, ci, n)
    want, k = components_ref.scipy_labels(rp, ci, n)
    assert np.array_equal(lab, want)
    assert np.all(lab <= np.arange(n)) and np.array_equal(lab[lab], lab)
    comps, largest, label = components_ref.stats(lab)
    assert comps == k
    assert (comps, largest, rounds) == RANDOM_GRAPHS[case]
    assert np.count_nonzero(lab == label) == largest


def test_reference_small_cases():
    # a stored 0.0 is an edge for scipy too: one component
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    G = sp.csr_matrix((np.array([0.0, 1.0]), np.array([1, 2]), np.array([0, 1, 2, 2])), shape=(3, 3))
    assert connected_components(G, directed=True, connection="weak")[0] == 1
    lab, _ = components_ref.labels([0, 1, 2, 2], [1, 2], 3)
    assert lab.tolist() == [0, 0, 0]
    # self-loop, duplicate, empty rows, an edge stored from its larger end only
    lab, _ = components_ref.labels([0, 1, 1, 3, 3, 4], [0, 4, 4, 1], 5)
    assert lab.tolist() == [0, 1, 1, 3, 1]
    assert components_ref.canonical([2, 0, 2, 1], 4).tolist() == [0, 1, 0, 3]
    assert components_ref.stats(np.array([0, 1, 0, 3, 3])) == (3, 2, 0)
