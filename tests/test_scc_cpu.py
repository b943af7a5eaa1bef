"""g4s_strongly_connected_components without a GPU: the reference of tests/scc_ref.py against scipy and networkx on every graph the GPU tests use, the
property each graph is named for; then the struct and signature in every layer, the exported symbol, argument refusals before any HIP call
(G4S_ERR_INVALID), the C++ form of include/g4s/csr.hpp and examples/scc.cpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import scc_ref as ref
from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.mark.parametrize("name", sorted(ref.CASES) + ["doubling_out_tree"])
def test_reference_equals_scipy_and_networkx(name):
    n, rp, ci, trp, tci, r = ref.case(name)
    labels = r["labels"]
    assert np.array_equal(labels, ref.scipy_labels(rp, ci, n))
    assert np.array_equal(labels, ref.networkx_labels(rp, ci, n))
    assert np.all(labels <= np.arange(n)) and np.array_equal(labels[labels], labels)               # canonical
    assert r["trimmed"] + r["pivot_size"] <= n and (r["pivot"] == -1) == (r["trimmed"] == n)
    assert r["pivot"] == -1 or labels[r["pivot"]] == labels[labels == labels[r["pivot"]]].min() and np.count_nonzero(labels == labels[r["pivot"]]) == r["pivot_size"]
    assert len(r["roots"]) == r["color_rounds"] and all(k >= 1 for k in r["roots"])                # every round removes a component
    rows, trows = np.repeat(np.arange(n), np.diff(rp)), np.repeat(np.arange(n), np.diff(trp))
    assert np.array_equal(np.sort(rows * n + ci), np.sort(tci.astype(np.int64) * n + trows))       # the transpose the tests hand over is one


def test_each_case_has_the_property_it_is_named_for():
    n, rp, ci, trp, tci, r = ref.case("tiny")
    assert r["labels"].tolist() == ref.TINY_LABELS == [0, 1, 1, 3, 3, 3, 6, 7, 8, 9]
    assert ci[rp[0]:rp[1]].tolist() == [0] and ci[rp[1]:rp[2]].tolist() == [2, 2, 7] and ci[rp[5]:rp[6]].tolist() == [4, 3]   # a loop, a repeat, an unsorted row
    assert rp[6] == rp[7] and ci[rp[7]:rp[8]].tolist() == [7] and 3 in ci[rp[2]:rp[3]]             # an empty row, a lone self-loop, the bridge
    n, *_, r = ref.case("cycle")
    assert (n, r["pivot_size"], r["reach_steps"], r["trimmed"], r["color_rounds"]) == (2049, 2049, (2049, 2049), 0, 0)
    n, *_, r = ref.case("path")
    assert (n, r["trimmed"], r["pivot"], r["color_rounds"]) == (1500, 1500, -1, 0) and r["trim_frontiers"] == [2] * 750
    for name, hubs in (("hub_cycle", 1), ("two_hubs", 2)):
        n, rp, ci, trp, tci, r = ref.case(name)
        assert np.count_nonzero(np.diff(rp) > 4096) == hubs == np.count_nonzero(np.diff(trp) > 4096) and r["pivot"] == 0 and r["pivot_size"] == 5001
        assert (r["components"], r["color_rounds"], r["roots"]) == (hubs, hubs - 1, [1] * (hubs - 1))
    n, rp, ci, trp, tci, r = ref.case("hub_out")
    assert rp[1] - rp[0] == 5000 and r["trim_frontiers"] == [5001] and r["pivot"] == -1
    n, rp, ci, trp, tci, r = ref.case("funnel_closed")
    assert rp[1] - rp[0] == 5000 and trp[2] - trp[1] == 5000 and (r["components"], r["pivot_size"], r["trimmed"]) == (1, 5002, 0)
    n, rp, ci, trp, tci, r = ref.case("funnel_open")
    assert trp[2] - trp[1] == 5000 and r["trim_frontiers"] == [2, 5000] and r["trimmed"] == 5002    # 5000 decrements land on vertex 1's counter
    n, *_, r = ref.case("two_cycles")
    assert (r["pivot"], r["pivot_size"], r["color_rounds"], r["components"]) == (0, 1000, 1, 2) and r["labels"][:4].tolist() == [0, 1, 0, 1]
    n, *_, r = ref.case("chain40")
    assert (r["components"], r["pivot_size"], r["color_rounds"], r["roots"]) == (40, 3, 39, [1] * 39)
    n, *_, r = ref.case("chain40rev")
    assert (r["components"], r["pivot_size"], r["color_rounds"], r["roots"]) == (40, 3, 1, [39])
    n, *_, r = ref.case("cycles_dag")
    assert (r["components"], r["trimmed"], r["trim_frontiers"]) == (700, 400, [400]) and r["pivot_size"] <= 40
    assert 6 <= r["color_rounds"] <= 7 and r["roots"][0] >= 100
    n, rp, ci, trp, tci, r = ref.case("rmat13")
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.any(ci == rows) and np.unique(rows * n + ci).size < ci.size                          # self-loops and repeats are stored
    assert (r["largest"], r["pivot_size"], len(r["trim_frontiers"]), r["color_rounds"]) == (2969, 2969, 3, 0) and r["trimmed"] == n - 2969
    n, *_, r = ref.case("er")
    assert len(r["trim_frontiers"]) >= 10 and r["pivot_size"] > 1000 and min(r["reach_steps"]) >= 25
    n, *_, r = ref.case("doubling_out_tree")
    assert (n, r["pivot"], r["pivot_size"], r["reach_steps"][0]) == ((1 << 18) - 1, 0, n, 18)


def test_struct_and_signature_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    m = re.search(r"typedef struct g4s_scc_info \{(.*?)\} g4s_scc_info;", text, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(capi.SCCInfo._fields_)
    assert [name for _, name in fields if name != "reserved"] == ["components", "largest", "largest_label", "trimmed", "pivot", "pivot_size", "color_rounds",
                                                                 "edges_walked", "launches", "resumes", "host_waits", "built_transpose"]
    assert C.sizeof(capi.SCCInfo) == 64 and "} g4s_scc_info;              /* 64 bytes */" in text
    assert int(re.search(r"#define\s+G4S_SCC_BATCH\s+(\d+)", text).group(1)) == capi.SCC_BATCH == 16
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"g4s_status\s+g4s_strongly_connected_components\s*\((.*?)\);", text, re.S).group(1), flags=re.S)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["int32_t n", "const int32_t *rowptr", "const int32_t *colids", "const int32_t *trowptr", "const int32_t *tcolids", "int32_t *labels",
                    "unsigned flags", "g4s_scc_info *info", "void *stream"]
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_strongly_connected_components"] == (C.c_int, [C.c_int32, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(capi.SCCInfo), vp])
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_strongly_connected_components(" in hpp and hpp.count("StronglyConnectedComponents(") >= 2
    assert "info.host_waits <= info.launches / 16 + 5" in text                                    # the bound tests/test_scc_gpu.py holds the call to
    assert "g4s_strongly_connected_components, g4s_kcore" in text                                 # the list of calls that threads may make side by side


def test_symbol_is_exported():
    from g4s_amd import capi
    assert hasattr(capi.load(), "g4s_strongly_connected_components")


def test_call_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_strongly_connected_components
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.SCCInfo()
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20, capi.CC_SYMMETRIC]:
        for base in (0, 1):
            assert fn(5, fake, fake, fake, fake, fake, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (0, 1):
        for tr in ((fake, fake), (None, None)):
            assert fn(5, None, fake, *tr, fake, f, None, None) == capi.ERR_INVALID
            assert "rowptr" in lib.g4s_last_error().decode()
            assert fn(5, fake, fake, *tr, None, f, None, None) == capi.ERR_INVALID
            assert "labels" in lib.g4s_last_error().decode()
            assert fn(5, fake, None, *tr, fake, f, None, None) == capi.ERR_INVALID
            assert "colids" in lib.g4s_last_error().decode()
            assert fn(-1, fake, fake, *tr, fake, f, None, None) == capi.ERR_INVALID
            assert "negative" in lib.g4s_last_error().decode()
            assert fn(0, None, None, *tr, fake, f, None, None) == capi.ERR_INVALID               # rowptr is required even for n == 0
        for tr in ((fake, None), (None, fake)):                                                  # one NULL without the other
            assert fn(5, fake, fake, *tr, fake, f, None, None) == capi.ERR_INVALID
            assert "trowptr and tcolids" in lib.g4s_last_error().decode()
    # host pointers: labels that overlap an input (real arrays: the check reads rowptr[n] and trowptr[n])
    rp, ci = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32)
    trp, tci = rp.copy(), ci.copy()
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    for labels, tr in ((P(rp), (None, None)), (P(rp, 3), (None, None)), (P(ci), (None, None)), (P(trp, 1), (P(trp), P(tci))), (P(tci), (P(trp), P(tci)))):
        assert fn(3, P(rp), P(ci), *tr, labels, capi.HOST_POINTERS, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    assert rp.tolist() == trp.tolist() == [0, 1, 2, 2] and ci.tolist() == tci.tolist() == [1, 0]


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    int32_t l[4];\n    g4s_scc_info info = {};\n"
           "    static_assert(sizeof(g4s_scc_info) == 64, \"g4s_scc_info\");\n"
           "    static_assert(G4S_SCC_BATCH == 16, \"G4S_SCC_BATCH\");\n"
           "    if (argc > 5) { g4s::StronglyConnectedComponents(a, l); g4s::StronglyConnectedComponents(a, l, &info);\n"
           "        g4s_strongly_connected_components(0, nullptr, nullptr, nullptr, nullptr, l, G4S_DEVICE_POINTERS, &info, nullptr); }\n"
           "    return (int)info.components * 0 + info.pivot * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_example_compiles(tmp_path):
    _build_example("scc.cpp", str(tmp_path / "scc"))


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    wide = types.SimpleNamespace(rows=3, cols=4)                      # no device arrays: the shape is checked first
    for fn in (host.strongly_connected_components, host.CSR.strongly_connected_components, host.condensation):
        with pytest.raises(ValueError, match="square"):
            fn(wide)
    rp, ci = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32)
    for bad in ((rp[:-1], ci), (rp, ci[:-1]), (np.zeros(5, np.int32), ci)):
        with pytest.raises(ValueError, match="wrong length"):
            host.strongly_connected_components((rp, ci), transpose=bad)
    for bad in ((rp,), (rp, ci, ci), rp, 3):
        with pytest.raises(ValueError, match="pair"):
            host.strongly_connected_components((rp, ci), transpose=bad)
    import torch
    for bad in ((torch.from_numpy(rp), ci), (rp, torch.from_numpy(ci)), (torch.from_numpy(rp), torch.from_numpy(ci))):   # CPU tensors: nothing touches a GPU
        with pytest.raises(ValueError, match="same kind"):
            host.strongly_connected_components((rp, ci), transpose=bad)
    with pytest.raises(ValueError, match="same kind"):
        host.strongly_connected_components((torch.from_numpy(rp), torch.from_numpy(ci)), transpose=(rp, ci))
    for bad in ("yes", 1, 0, None):
        with pytest.raises(ValueError, match="return_info"):
            host.strongly_connected_components((rp, ci), return_info=bad)
    with pytest.raises(ValueError, match="pair"):
        host.strongly_connected_components((rp,))
    with pytest.raises(ValueError, match="rowptr"):
        host.strongly_connected_components((np.zeros(0, np.int32), np.zeros(0, np.int32)))
    with pytest.raises(ValueError, match="CSR"):
        host.condensation((rp, ci))
