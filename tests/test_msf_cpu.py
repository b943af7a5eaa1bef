"""tests/msf_ref.py, the reference of the GPU tests of g4s_minimum_spanning_forest, held against scipy's minimum_spanning_tree and networkx's
minimum_spanning_edges / maximum_spanning_edges on every named graph: edge count, component count and total weight (the weights are integer-valued, so
every sum is exact and compared with ==), the labels against tests/components_ref.py, and the edge set itself where all weights are distinct; then the struct and signature in every layer, the argument refusals before any HIP call
(G4S_ERR_INVALID) and the Python ValueErrors. No GPU."""
import numpy as np
import pytest

from tests import components_ref
from tests import msf_ref as ref


def _pair_weights(n, rp, ci, w, maximum):
    """{(lo, hi): the weight Kruskal would meet first} of the off-diagonal entries; all 1.0 without values"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    best = {}
    for i, j, x in zip(rows.tolist(), ci.tolist(), (np.ones(ci.size) if w is None else w).tolist()):
        if i != j:
            key = (min(i, j), max(i, j))
            best[key] = x if key not in best else (max(best[key], x) if maximum else min(best[key], x))
    return best


def _scipy_total(n, best, maximum):
    """(edges, total weight) of scipy's minimum spanning tree of the pairs, every weight shifted to >= 1 first: scipy takes a stored 0 for no edge"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    if not best:
        return 0, 0.0
    keys = np.array(list(best.keys()))
    w = np.array(list(best.values()))
    w = -w if maximum else w
    shift = 1.0 - w.min()
    T = minimum_spanning_tree(sp.csr_matrix((w + shift, (keys[:, 0], keys[:, 1])), shape=(n, n)))
    total = T.sum() - shift * T.nnz
    return int(T.nnz), float(-total if maximum else total)


def _networkx(n, best, maximum):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from((a, b, x) for (a, b), x in best.items())
    edges = list((nx.maximum_spanning_edges if maximum else nx.minimum_spanning_edges)(G, data=True))
    return {(min(a, b), max(a, b)) for a, b, _ in edges}, float(sum(d["weight"] for _, _, d in edges)), nx.number_connected_components(G)


@pytest.mark.parametrize("maximum", [False, True])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_reference_agrees_with_scipy_and_networkx(name, maximum):
    n, rp, ci, w, r = ref.case(name, maximum)
    best = _pair_weights(n, rp, ci, w, maximum)
    unit = 0.0 if w is None else 1.0                                    # without values the call reports weight 0.0
    s_edges, s_total = _scipy_total(n, best, maximum)
    x_pairs, x_total, x_comps = _networkx(n, best, maximum)
    assert r["edges"] == s_edges == len(x_pairs)
    assert r["components"] == x_comps == n - r["edges"]
    assert r["weight"] == s_total * unit == x_total * unit
    assert np.array_equal(r["labels"], components_ref.labels(rp, ci, n)[0])
    assert np.array_equal(r["positions"], np.unique(r["positions"]))   # ascending, no repeats
    got = ref.pairs(rp, ci, r["positions"], n)
    assert len(got) == r["edges"] and got <= set(best)
    if name in ref.DISTINCT:
        assert got == x_pairs


@pytest.mark.parametrize("deg,kind", ref.RANDOM)
def test_random_graphs_agree_with_scipy(deg, kind):
    n, rp, ci, w, r = ref.random_case(deg, kind)
    s_edges, s_total = _scipy_total(n, _pair_weights(n, rp, ci, w, False), False)
    assert (r["edges"], r["weight"]) == (s_edges, s_total)
    lab, k = components_ref.scipy_labels(rp, ci, n)
    assert np.array_equal(r["labels"], lab) and r["components"] == k


def test_the_order_by_hand():
    # the tie-break: all weights equal → (lo, hi) decides, then the position
    n, rp, ci, w, r = ref.case("repeats_equal")
    assert r["positions"].tolist() == [0, 3, 4]
    n, rp, ci, w, r = ref.case("repeats_differ")
    assert r["positions"].tolist() == [2, 3, 4] and r["weight"] == 10.0
    n, rp, ci, w, r = ref.case("two_k6")
    light, heavy = (5, 11), (0, 6)
    got = ref.pairs(rp, ci, r["positions"], n)
    assert light in got and heavy not in got
    got = ref.pairs(rp, ci, ref.case("two_k6", True)[4]["positions"], n)
    assert heavy in got and light not in got
    n, rp, ci, w, r = ref.case("self_loops")
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert (rows[r["positions"]] != ci[r["positions"]]).all() and r["weight"] == 6.0 and r["components"] == 2
    # −0.0 ties with +0.0: the position decides
    z = ref.forest(2, [0, 2, 2], [1, 1], [0.0, -0.0])
    assert z["positions"].tolist() == [0]
    z = ref.forest(2, [0, 2, 2], [1, 1], [-0.0, 0.0], maximum=True)
    assert z["positions"].tolist() == [0]
    with pytest.raises(ValueError):
        ref.forest(2, [0, 1, 1], [1], [float("nan")])
    up, low, full = (ref.case(f"tri_{p}") for p in ("upper", "lower", "full"))
    assert ref.pairs(up[1], up[2], up[4]["positions"], up[0]) == ref.pairs(low[1], low[2], low[4]["positions"], low[0]) == ref.pairs(full[1], full[2], full[4]["positions"], full[0])


def test_struct_and_signature_agree_across_layers():
    import ctypes as C
    import os
    import re
    from g4s_amd import capi
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = open(os.path.join(include, "g4s.h")).read()
    m = re.search(r"typedef struct g4s_msf_info \{(.*?)\} g4s_msf_info;", text, re.S)
    fields = re.findall(r"(int64_t|int32_t|double)\s+(\w+);", m.group(1))
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    assert [(name, ctype[t]) for t, name in fields] == list(capi.MSFInfo._fields_)
    assert [name for _, name in fields] == ["components", "edges", "weight", "entries_walked", "rounds", "launches", "resumes", "host_waits"]
    assert C.sizeof(capi.MSFInfo) == 48 and "} g4s_msf_info;              /* 48 bytes */" in text
    assert int(re.search(r"#define\s+G4S_MSF_BATCH\s+(\d+)", text).group(1)) == capi.MSF_BATCH == 16
    assert int(re.search(r"#define\s+G4S_MSF_MAXIMUM\s+(\d+)u", text).group(1)) == capi.MSF_MAXIMUM == 1 << 20
    others = {int(v) for v in re.findall(r"#define\s+G4S_(?!MSF_MAXIMUM)[A-Z0-9_]+\s+(\d+)u\b", text)}
    assert not any(v & capi.MSF_MAXIMUM for v in others)               # no other flag shares the bit
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"g4s_status\s+g4s_minimum_spanning_forest\s*\((.*?)\);", text, re.S).group(1), flags=re.S)
    assert [" ".join(a.split()) for a in proto.split(",")] == ["int32_t n", "const int32_t *rowptr", "const int32_t *colids", "const double *values", "int32_t *edges",
                                                              "int32_t *labels", "unsigned flags", "g4s_msf_info *info", "void *stream"]
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_minimum_spanning_forest"] == (C.c_int, [C.c_int32, vp, vp, vp, vp, vp, C.c_uint, C.POINTER(capi.MSFInfo), vp])
    hpp = open(os.path.join(include, "g4s", "csr.hpp")).read()
    assert "g4s_minimum_spanning_forest(" in hpp and "MinimumSpanningForest(" in hpp and "MaximumSpanningForest(" in hpp
    assert "info.host_waits <= info.launches / 16 + 3" in text         # the bound tests/test_msf_gpu.py holds the call to
    assert "rounds <= ceil(log2 n) + 1" in text
    assert "g4s_minimum_spanning_forest, g4s_connected_components" in text   # the list of calls that threads may make side by side


def test_call_rejects_arguments_before_hip():
    import ctypes as C
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_minimum_spanning_forest
    fake = C.c_void_p(0x1000)                                          # never dereferenced: every check below comes first
    other = C.c_void_p(0x100000)
    info = capi.MSFInfo()
    D = capi.DEVICE_POINTERS
    for b in [1 << k for k in range(1, 32) if 1 << k != capi.MSF_MAXIMUM] + [1536, capi.CC_SYMMETRIC]:
        for base in (0, 1, capi.MSF_MAXIMUM):
            assert fn(5, fake, fake, None, other, None, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (D, D | capi.MSF_MAXIMUM):
        assert fn(5, None, fake, None, other, None, f, None, None) == capi.ERR_INVALID and "rowptr" in lib.g4s_last_error().decode()
        assert fn(5, fake, fake, None, None, None, f, None, None) == capi.ERR_INVALID and "edges" in lib.g4s_last_error().decode()
        assert fn(5, fake, None, None, other, None, f, None, None) == capi.ERR_INVALID and "colids" in lib.g4s_last_error().decode()
        assert fn(-1, fake, fake, None, other, None, f, None, None) == capi.ERR_INVALID and "negative" in lib.g4s_last_error().decode()
        assert fn(5, fake, fake, None, fake, None, f, None, None) == capi.ERR_INVALID and "overlap" in lib.g4s_last_error().decode()
        assert fn(5, fake, C.c_void_p(0x2000), None, other, other, f, None, None) == capi.ERR_INVALID and "overlap" in lib.g4s_last_error().decode()
    # host pointers: outputs that overlap an input or each other (real arrays: the check reads rowptr[n])
    rp, ci, w = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0])
    out, lab = np.full(4, -7, np.int32), np.full(4, -7, np.int32)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    for edges, labels in ((P(rp), None), (P(rp, 3), None), (P(ci, 1), None), (P(w, 2), None), (P(out), P(rp, 2)), (P(out), P(out, 1)), (P(out), P(w))):
        assert fn(3, P(rp), P(ci), P(w), edges, labels, capi.HOST_POINTERS, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    assert rp.tolist() == [0, 1, 2, 2] and ci.tolist() == [1, 0] and w.tolist() == [1.0, 2.0] and (out == -7).all() and (lab == -7).all()


def test_python_value_errors_come_before_the_gpu():
    from g4s_amd import host
    rp, ci = np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32)
    for bad in (lambda: host.minimum_spanning_forest((rp, ci), maximum=1), lambda: host.minimum_spanning_forest((rp, ci), return_labels="yes"),
                lambda: host.minimum_spanning_forest((rp,)), lambda: host.minimum_spanning_forest((rp, ci, np.ones(3))),
                lambda: host.minimum_spanning_forest((np.zeros(0, np.int32), ci)), lambda: host.spanning_forest_csr((rp, ci), None),
                lambda: host.spanning_forest_csr(None, None, symmetric=0)):
        with pytest.raises(ValueError):
            bad()
