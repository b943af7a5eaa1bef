"""g4s_ktruss without a GPU: the numpy reference of tests/ktruss_ref.py against networkx.k_truss for every k on the graphs the GPU tests use, the
property each graph is named for; then the struct and signature in every layer, the exported symbol, argument refusals before any HIP call
(G4S_ERR_INVALID), the C++ form of include/g4s/csr.hpp and examples/ktruss.cpp (compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import ktruss_ref as ref
from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
INT32_MAX = 2**31 - 1

# name → (undirected edges, triangles, max truss, levels, rounds) of the reference
FACTS = {"tiny": (4, 1, 3, 2, 2), "star": (5000, 0, 2, 1, 1), "path": (4000, 0, 2, 1, 1), "grid": (8064, 0, 2, 1, 1), "k4_ear": (8, 5, 4, 2, 2),
         "hub_leaves_clique": (5190, 1185, 20, 3, 3), "tri_grid": (12033, 7938, 3, 1, 64), "rmat10": (10588, 74294, 28, 25, 140),
         "rmat11": (22770, 191072, 37, 35, 194), "hub_bridge": (8270, 170, 9, 3, 4), "hub_pair": (8215, 4120, 6, 2, 2),
         "tri_tree": (458751, 327679, 4, 2, 17)}
# networkx needs 7 s for rmat10, 23 s for rmat11 and far longer for the 458 751 edges of tri_tree, whose decomposition is pinned in closed form below
NETWORKX = [name for name in ref.CASES if name not in ("rmat11", "tri_tree")]

# what the host loop sizes a peel grid with (step_batch.hpp)
EDGES_PER_WG, GRID_GROWTH, MIN_GRID, MAX_GRID = 2048, 8, 8, 2 * 256     # two workgroups per CU of an MI355X at the most
ENTRY_WEIGHT = 16                      # ktruss.hip: kEntryWeight


def _upper(rp, ci, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    return rows, np.asarray(ci) > rows


@pytest.mark.parametrize("name", NETWORKX)
def test_reference_equals_networkx_for_every_k(name):
    import networkx as nx
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case(name)
    G = ref.networkx_graph(rp, ci, n)
    top = ref.facts(rp, ci, n, support, truss)[2]
    for k in range(2, top + 2):
        want = {(min(a, b), max(a, b)) for a, b in nx.k_truss(G, k).edges()}
        assert ref.truss_edges(rp, ci, n, truss, k) == want, (name, k)
    assert not ref.truss_edges(rp, ci, n, truss, top + 1)
    tri = nx.triangles(G)
    assert sum(tri.values()) // 3 == FACTS[name][1]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_reference_counts_and_shape(name):
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case(name)
    assert ref.facts(rp, ci, n, support, truss)[:3] + (levels, rounds) == FACTS[name]
    rows, up = _upper(rp, ci, n)
    diag = np.asarray(ci) == rows
    assert np.all(truss[diag] == 0) and np.all(rnd[diag] == -1) and np.all(support[diag] == 0)
    assert np.all(truss[~diag] >= 2) and rnd[~diag].min() == 0 and np.unique(rnd[~diag]).size == rounds      # every frontier is non-empty
    assert np.unique(truss[~diag]).size == levels
    eid, eu, ev = ref.edge_ids(rp, ci, n)                              # both copies of an edge carry the same values
    for x in (support, truss, rnd):
        per_edge = np.zeros(eu.size, np.int64)
        per_edge[eid[up]] = x[up]
        assert np.array_equal(per_edge[eid[~diag]], x[~diag])
    order = np.argsort(rnd[up], kind="stable")
    assert np.all(np.diff(truss[up][order]) >= 0)                      # j never decreases along the peel
    assert np.all(np.diff(np.asarray(ci, np.int64))[np.diff(rows) == 0] > 0)                                   # rows strictly ascending
    key = np.sort(rows * n + ci)
    assert np.array_equal(key, np.sort(np.asarray(ci, np.int64) * n + rows))                                   # symmetric


def _edge(rp, ci, u, v):
    return int(rp[u] + np.searchsorted(ci[rp[u]:rp[u + 1]], v))


def test_each_case_has_the_property_it_is_named_for():
    for name in ("star", "path", "grid"):                             # triangle-free: one level, one round, everything truss 2
        n, rp, ci, support, truss, rnd, _, _ = ref.case(name)
        assert not support.any() and np.all(truss == 2) and not rnd.any()
    n, rp, ci, support, truss, rnd, _, _ = ref.case("tiny")
    rows, _ = _upper(rp, ci, n)
    assert np.count_nonzero(ci == rows) == 2 and sorted(truss.tolist()) == [0, 0, 2, 2, 3, 3, 3, 3, 3, 3]     # the stored diagonal entries
    # k4_ear: the triangle (0, 1, 4) has two frontier edges in round 0 and takes ONE off (0, 1): 3 → 2, which keeps it in the 4-truss
    n, rp, ci, support, truss, rnd, _, _ = ref.case("k4_ear")
    p01 = _edge(rp, ci, 0, 1)
    assert (support[p01], truss[p01], rnd[p01]) == (3, 4, 1)
    for u, v in ((0, 4), (1, 4), (4, 0), (4, 1)):
        assert (support[_edge(rp, ci, u, v)], truss[_edge(rp, ci, u, v)], rnd[_edge(rp, ci, u, v)]) == (1, 3, 0)
    rows, up = _upper(rp, ci, n)
    assert np.count_nonzero(truss[up] == 4) == 6 and np.count_nonzero(truss[up] == 3) == 2
    n, rp, ci, support, truss, rnd, _, _ = ref.case("hub_leaves_clique")
    assert np.unique(truss).tolist() == [2, 11, 20] and rp[1] - rp[0] == 5000 > ref.HUB_CUT
    n, rp, ci, support, truss, rnd, _, rounds = ref.case("tri_grid")
    rows, up = _upper(rp, ci, n)
    assert np.all(truss == 3) and rounds == 64 and np.all(np.bincount(rnd[up]) > 0)                            # a long run of dependent frontiers
    for name in ("rmat10", "rmat11"):
        n, rp, ci, support, truss, rnd, _, _ = ref.case(name)
        rows, up = _upper(rp, ci, n)
        assert np.any(ci == rows)                                     # stored diagonal entries
        eid, eu, ev = ref.edge_ids(rp, ci, n)
        T = ref.triangles(eu, ev, n)
        r = np.zeros(eu.size, np.int64)
        r[eid[up]] = rnd[up]
        rt = np.sort(r[T], axis=1)
        assert np.any((rt[:, 0] == rt[:, 1]) & (rt[:, 1] < rt[:, 2]))                                          # triangles with two frontier edges
    # hub_bridge: (0, 1) is peeled alone in round 1 along a 4 109-entry row and takes one off each of the six alive edges (0, a), (1, a)
    n, rp, ci, support, truss, rnd, _, _ = ref.case("hub_bridge")
    rows, up = _upper(rp, ci, n)
    p01 = _edge(rp, ci, 0, 1)
    assert rp[1] - rp[0] == rp[2] - rp[1] == 4109 > ref.HUB_CUT
    assert (support[p01], truss[p01], rnd[p01]) == (3, 5, 1) and np.count_nonzero(rnd[up] == 1) == 1
    assert np.count_nonzero(rnd[up] == 0) == 8200                     # the first frontier: the leaf edges
    for a in (2, 3, 4):
        for u in (0, 1):
            p = _edge(rp, ci, u, a)
            assert (support[p], truss[p]) == (8, 9) and rnd[p] > 1    # 8 → 7 = j + 2 − 2 at truss 9: alive when (0, 1) goes, and it stays
    n, rp, ci, support, truss, rnd, _, _ = ref.case("hub_pair")
    p01 = _edge(rp, ci, 0, 1)
    assert support[p01] == 4104 and min(rp[1] - rp[0], rp[2] - rp[1]) == 4105 > ref.HUB_CUT and truss[p01] == 6


def test_the_resume_case_outgrows_the_grid_of_its_batch():
    """tri_tree: generation g is round g at level j = 1, the frontier doubles. The host sizes a peel grid from the frontier it reads between batches
    (StepGrid of step_batch.hpp, a walk entry weighing ENTRY_WEIGHT plain ones) and stops a batch whose frontier passes that grid's cap. The first
    batch is 16 launches with two peels in four, so the second begins by round 8 and holds at least 14 peels: whichever round b <= 9 a batch begins
    at, a frontier BUILT BY A PEEL within its next 14 rounds has more walk entries than the cap of the grid sized at b."""
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case("tri_tree")
    rows, up = _upper(rp, ci, n)
    eid, eu, ev = ref.edge_ids(rp, ci, n)
    r = rnd[up]
    sizes = np.bincount(r, minlength=rounds)
    walk = np.bincount(r, weights=ref.walk_len(rp, eu, ev), minlength=rounds).astype(np.int64)
    assert sizes[:16].tolist() == [1 << g for g in range(16)] and sizes[16] == 6 << 16
    assert np.all(truss[up][r < 16] == 3) and np.all(truss[up][r == 16] == 4)
    for b in range(10):
        grid = max(MIN_GRID, min(MAX_GRID, ENTRY_WEIGHT * int(walk[b] + sizes[b]) // EDGES_PER_WG))
        assert grid < MAX_GRID                                        # the largest grid takes whatever comes
        cap = grid * EDGES_PER_WG * GRID_GROWTH // ENTRY_WEIGHT
        assert np.any(walk[b + 1:min(b + 15, 16)] > cap), b          # rounds 1 … 15 are built by peels, round 16 by a scan
    assert ci.size < 1 << 20


def test_reference_max_k():
    n, rp, ci, support, truss, rnd, _, _ = ref.case("rmat10")
    rows, up = _upper(rp, ci, n)
    off = np.asarray(ci) != rows
    for cap in (2, 3, 5, 28, 29):
        s, t, r, lv, _, capped = ref.ktruss(rp, ci, n, cap)
        assert np.array_equal(s, support) and np.array_equal(t, np.minimum(truss, cap))
        assert np.array_equal(r[off] < 0, truss[off] >= cap) and capped == int(np.any(truss >= cap))
        assert np.array_equal(r[r >= 0], rnd[r >= 0]) and lv == np.unique(truss[off & (truss < cap)]).size


def test_struct_and_signature_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    m = re.search(r"typedef struct g4s_ktruss_info \{(.*?)\} g4s_ktruss_info;", text, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(capi.KTrussInfo._fields_)
    assert [name for _, name in fields] == ["triangles", "edges_walked", "support_walked", "top_truss_edges", "max_truss", "levels", "rounds", "scans",
                                            "launches", "resumes", "host_waits", "capped"]
    assert C.sizeof(capi.KTrussInfo) == 64
    assert int(re.search(r"#define\s+G4S_KTRUSS_BATCH\s+(\d+)", text).group(1)) == capi.KTRUSS_BATCH == 16 and capi.KTRUSS_FULL == INT32_MAX
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"g4s_status\s+g4s_ktruss\s*\((.*?)\);", text, re.S).group(1), flags=re.S)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["int32_t n", "const int32_t *rowptr", "const int32_t *colids", "int32_t max_k", "int32_t *truss", "int32_t *round", "int32_t *support",
                    "unsigned flags", "g4s_ktruss_info *info", "void *stream"]
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_ktruss"] == (C.c_int, [C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_uint, C.POINTER(capi.KTrussInfo), vp])
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_ktruss(" in hpp and hpp.count("KTruss(") >= 2                                     # the function and the header comment's list
    assert "g4s_ktruss" in text.split("Different host threads may call at the same time")[1].split("Different streams from one thread")[0]


def test_symbol_is_exported():
    from g4s_amd import capi
    assert hasattr(capi.load(), "g4s_ktruss")


def test_call_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_ktruss
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.KTrussInfo()
    for b in [1 << k for k in range(1, 32)] + [1536, 3 << 20]:
        for base in (0, 1):
            assert fn(5, fake, fake, INT32_MAX, fake, fake, fake, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (0, 1):
        for rnd in (fake, None):
            for sup in (fake, None):
                assert fn(5, None, fake, INT32_MAX, fake, rnd, sup, f, None, None) == capi.ERR_INVALID
                assert fn(5, fake, fake, INT32_MAX, None, rnd, sup, f, None, None) == capi.ERR_INVALID
                assert fn(5, fake, None, INT32_MAX, fake, rnd, sup, f, None, None) == capi.ERR_INVALID
                assert "colids" in lib.g4s_last_error().decode()
                assert fn(-1, fake, fake, INT32_MAX, fake, rnd, sup, f, None, None) == capi.ERR_INVALID
                assert "negative" in lib.g4s_last_error().decode()
                for bad in (1, 0, -1, -2**31):
                    assert fn(5, fake, fake, bad, fake, rnd, sup, f, None, None) == capi.ERR_INVALID
                    assert "max_k" in lib.g4s_last_error().decode()
                assert fn(0, None, None, INT32_MAX, fake, rnd, sup, f, None, None) == capi.ERR_INVALID   # rowptr is required even for n == 0
    # host pointers: outputs that overlap an input or each other (real arrays: the check reads rowptr[n])
    rp, ci = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32)
    buf = np.zeros(8, np.int32)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    for truss, rnd, sup in ((P(rp), P(buf), None), (P(buf), P(ci), None), (P(buf), None, P(ci, 1)), (P(buf), P(buf, 1), None), (P(buf), None, P(buf, 1)),
                            (P(buf), P(buf, 4), P(buf, 5)), (P(rp, 3), None, None), (P(buf), P(buf), None)):
        assert fn(3, P(rp), P(ci), INT32_MAX, truss, rnd, sup, capi.HOST_POINTERS, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    assert rp.tolist() == [0, 1, 2, 2] and ci.tolist() == [1, 0] and not buf.any()


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    int32_t t[4], r[4], s[4];\n    g4s_ktruss_info info = {};\n"
           "    static_assert(sizeof(g4s_ktruss_info) == 64, \"g4s_ktruss_info\");\n"
           "    static_assert(G4S_KTRUSS_BATCH == 16, \"G4S_KTRUSS_BATCH\");\n"
           "    if (argc > 5) { g4s::KTruss(a, t); g4s::KTruss(a, t, r); g4s::KTruss(a, t, nullptr, s); g4s::KTruss(a, t, r, s, 4);\n"
           "        g4s::KTruss(a, t, r, s, INT32_MAX, &info);\n"
           "        g4s_ktruss(0, nullptr, nullptr, INT32_MAX, t, r, s, G4S_DEVICE_POINTERS, &info, nullptr); }\n"
           "    return (int)info.triangles * 0 + (int)info.top_truss_edges * 0 + info.max_truss * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_example_compiles(tmp_path):
    _build_example("ktruss.cpp", str(tmp_path / "ktruss"))


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    wide = types.SimpleNamespace(rows=3, cols=4)                      # no device arrays: the shape is checked first
    square = types.SimpleNamespace(rows=3, cols=3)
    for fn in (host.ktruss, host.CSR.ktruss):
        with pytest.raises(ValueError, match="square"):
            fn(wide)
    with pytest.raises(ValueError, match="square"):
        host.ktruss_subgraph(wide, 3)
    for bad in (-1, 0, 1, 2.0, "3", True, 2**31):
        with pytest.raises(ValueError, match="max_k"):
            host.ktruss(square, max_k=bad)
        with pytest.raises(ValueError, match="max_k"):
            host.CSR.ktruss(square, max_k=bad)
    for bad in (-1, 0, 1, 2.0, "3", True, None, 2**31):
        with pytest.raises(ValueError, match="k must be"):
            host.ktruss_subgraph(square, bad)
    for bad in ("yes", 1, 0, None):
        with pytest.raises(ValueError, match="return_round"):
            host.ktruss(square, return_round=bad)
        with pytest.raises(ValueError, match="return_support"):
            host.ktruss(square, return_support=bad)
        with pytest.raises(ValueError, match="return_info"):
            host.ktruss(square, return_info=bad)
    with pytest.raises(ValueError, match="pair"):
        host.ktruss((np.zeros(1, np.int32),))
    with pytest.raises(ValueError, match="rowptr"):
        host.ktruss((np.zeros(0, np.int32), np.zeros(0, np.int32)))
