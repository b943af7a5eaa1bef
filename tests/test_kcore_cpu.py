"""g4s_kcore without a GPU: the numpy reference of tests/kcore_ref.py against networkx.core_number on every graph the GPU tests use, (round, id) as a
degeneracy ordering, the property each graph is named for; then the struct and signature in every layer, the exported symbol, argument refusals
before any HIP call (G4S_ERR_INVALID), the C++ form of include/g4s/csr.hpp and examples/kcore.cpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import kcore_ref as ref
from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
INT32_MAX = 2**31 - 1

# name → (levels, rounds, degeneracy, size of the top core) of the reference
FACTS = {"tiny": (3, 3, 2, 3), "star": (1, 2, 1, 5001), "hub_leaves_clique": (3, 3, 19, 20), "path": (1, 2001, 1, 4001), "grid": (1, 63, 2, 4096),
         "doubling_tree": (2, 16, 39, 40), "rmat13": (62, 180, 90, 359)}


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_reference_equals_networkx_and_orders_by_degeneracy(name):
    n, rp, ci, core, rnd, levels, rounds = ref.case(name)
    assert np.array_equal(core, ref.networkx_core(rp, ci, n))
    assert (levels, rounds) + ref.top_core(core) == FACTS[name]
    assert rnd.min() == 0 and rnd.max() == rounds - 1 and np.unique(rnd).size == rounds          # every frontier is non-empty
    assert np.all(np.diff(core[ref.degeneracy_order(rnd)]) >= 0)                                  # k never decreases along the peel
    assert np.all(ref.later_neighbours(rp, ci, n, ref.degeneracy_order(rnd)) <= core)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.all(np.diff(ci.astype(np.int64))[np.diff(rows) == 0] > 0)                           # rows strictly ascending
    key = np.sort(rows * n + ci)
    assert np.array_equal(key, np.sort(ci.astype(np.int64) * n + rows))                          # symmetric


def test_each_case_has_the_property_it_is_named_for():
    n, rp, ci, core, rnd, _, _ = ref.case("tiny")
    assert core.tolist() == [0, 2, 2, 2, 0, 1, 1, 0] and rnd.tolist() == [0, 2, 2, 2, 0, 1, 1, 0]
    assert ci[rp[0]:rp[1]].tolist() == [0] and 3 in ci[rp[3]:rp[4]]                               # the stored diagonal entries
    n, rp, ci, core, rnd, _, _ = ref.case("star")
    assert rp[1] - rp[0] == 5000 > 4096 and core[0] == 1 and rnd[0] == 1 and np.all(rnd[1:] == 0)   # the hub leaves by the crossing, after its leaves
    n, rp, ci, core, rnd, _, _ = ref.case("hub_leaves_clique")
    assert rp[1] - rp[0] == 5000 > 4096 and core[0] == 10 and rnd[0] == 1                         # the hub is collected by a scan (a level jump 1 → 10)
    assert np.unique(core).tolist() == [1, 10, 19] and np.count_nonzero(core == 19) == 20
    n, rp, ci, core, rnd, _, rounds = ref.case("path")
    assert np.all(core == 1) and np.all(np.bincount(rnd)[:-1] == 2) and rounds == 2001
    n, rp, ci, core, rnd, _, _ = ref.case("grid")
    assert np.all(core == 2)
    n, rp, ci, core, rnd, _, _ = ref.case("doubling_tree")
    tree = (1 << 15) - 1
    assert np.all(core[:tree] == 2) and np.all(core[tree:] == 39) and n - tree == 40
    assert rnd[0] == 0 and np.all(rnd[(1 << 14) - 1:tree] == 14) and np.all(rnd[tree:] == 15)
    sizes = np.bincount(rnd)
    assert sizes[:15].tolist() == [1 << d for d in range(15)]                                     # the frontier doubles: 1 → 16384 vertices
    assert int(np.diff(rp)[(1 << 14) - 1:tree].sum()) == 49152
    n, rp, ci, core, rnd, levels, _ = ref.case("rmat13")
    assert levels >= 32 and np.any(ci == np.repeat(np.arange(n), np.diff(rp)))                    # many levels; self-loops are stored
    assert np.any(np.diff(np.unique(core)) > 1)                                                   # jumps between the sparse top levels


def test_reference_max_k():
    n, rp, ci, core, rnd, _, _ = ref.case("rmat13")
    for cap in (0, 1, 5, 90, 91):
        c, r, _, _, capped = ref.kcore(rp, ci, n, cap)
        assert np.array_equal(c, np.minimum(core, cap)) and np.array_equal(r < 0, core >= cap) and capped == int(np.any(core >= cap))
        assert np.array_equal(r[r >= 0], rnd[r >= 0])


def test_struct_and_signature_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    m = re.search(r"typedef struct g4s_kcore_info \{(.*?)\} g4s_kcore_info;", text, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(capi.KCoreInfo._fields_)
    assert C.sizeof(capi.KCoreInfo) == 48
    assert int(re.search(r"#define\s+G4S_KCORE_BATCH\s+(\d+)", text).group(1)) == capi.KCORE_BATCH == 16
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"g4s_status\s+g4s_kcore\s*\((.*?)\);", text, re.S).group(1), flags=re.S)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["int32_t n", "const int32_t *rowptr", "const int32_t *colids", "int32_t max_k", "int32_t *core", "int32_t *round", "unsigned flags",
                    "g4s_kcore_info *info", "void *stream"]
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_kcore"] == (C.c_int, [C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_uint, C.POINTER(capi.KCoreInfo), vp])
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_kcore(" in hpp and hpp.count("KCore(") >= 2                                      # the function and the header comment's list


def test_symbol_is_exported():
    from g4s_amd import capi
    assert hasattr(capi.load(), "g4s_kcore")


def test_call_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_kcore
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.KCoreInfo()
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20]:
        for base in (0, 1):
            assert fn(5, fake, fake, INT32_MAX, fake, fake, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (0, 1):
        for rnd in (fake, None):
            assert fn(5, None, fake, INT32_MAX, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert fn(5, fake, fake, INT32_MAX, None, rnd, f, None, None) == capi.ERR_INVALID
            assert fn(5, fake, None, INT32_MAX, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert "colids" in lib.g4s_last_error().decode()
            assert fn(-1, fake, fake, INT32_MAX, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert "negative" in lib.g4s_last_error().decode()
            assert fn(5, fake, fake, -1, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert "max_k" in lib.g4s_last_error().decode()
            assert fn(0, None, None, INT32_MAX, fake, rnd, f, None, None) == capi.ERR_INVALID    # rowptr is required even for n == 0
    # host pointers: outputs that overlap an input or each other (real arrays: the check reads rowptr[n])
    rp, ci = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32)
    buf = np.zeros(8, np.int32)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    for core, rnd in ((P(rp), P(buf)), (P(buf), P(ci)), (P(buf), P(buf, 2)), (P(rp, 3), None), (P(buf), P(buf))):
        assert fn(3, P(rp), P(ci), INT32_MAX, core, rnd, capi.HOST_POINTERS, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    assert rp.tolist() == [0, 1, 2, 2] and ci.tolist() == [1, 0] and not buf.any()


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    int32_t c[4], r[4];\n    g4s_kcore_info info = {};\n"
           "    static_assert(sizeof(g4s_kcore_info) == 48, \"g4s_kcore_info\");\n"
           "    static_assert(G4S_KCORE_BATCH == 16, \"G4S_KCORE_BATCH\");\n"
           "    if (argc > 5) { g4s::KCore(a, c); g4s::KCore(a, c, r); g4s::KCore(a, c, nullptr, 3); g4s::KCore(a, c, r, INT32_MAX, &info);\n"
           "        g4s_kcore(0, nullptr, nullptr, INT32_MAX, c, r, G4S_DEVICE_POINTERS, &info, nullptr); }\n"
           "    return (int)info.top_core_size * 0 + info.degeneracy * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_example_compiles(tmp_path):
    _build_example("kcore.cpp", str(tmp_path / "kcore"))


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    wide = types.SimpleNamespace(rows=3, cols=4)                      # no device arrays: the shape is checked first
    square = types.SimpleNamespace(rows=3, cols=3)
    for fn in (host.kcore, host.CSR.kcore, host.degeneracy_order):
        with pytest.raises(ValueError, match="square"):
            fn(wide)
    with pytest.raises(ValueError, match="square"):
        host.kcore_subgraph(wide, 2)
    for bad in (-1, 1.0, "3", True, 2**31):
        with pytest.raises(ValueError, match="max_k"):
            host.kcore(square, max_k=bad)
        with pytest.raises(ValueError, match="max_k"):
            host.CSR.kcore(square, max_k=bad)
    for bad in (-1, 1.0, "3", True, None, 2**31):
        with pytest.raises(ValueError, match="k must be"):
            host.kcore_subgraph(square, bad)
    for bad in ("yes", 1, 0, None):
        with pytest.raises(ValueError, match="return_round"):
            host.kcore(square, return_round=bad)
        with pytest.raises(ValueError, match="return_info"):
            host.kcore(square, return_info=bad)
    with pytest.raises(ValueError, match="pair"):
        host.kcore((np.zeros(1, np.int32),))
    with pytest.raises(ValueError, match="rowptr"):
        host.kcore((np.zeros(0, np.int32), np.zeros(0, np.int32)))
