"""g4s_betweenness without a GPU: constants in every layer, exported symbols, argument checking before any HIP call (G4S_ERR_INVALID with a message
that names the argument), the C++ form of include/g4s/csr.hpp (compile only), the Python ValueErrors, and the numpy reference of
tests/betweenness_ref.py against networkx — so that the yardstick of the GPU tests is pinned to something this project did not write.

The bar of the networkx comparison is the project's fp64 parity bar, |ref − nx| <= 1e-10 · ref: every term of every sum is non-negative, so Σ|terms|
is the value itself and no cancellation can amplify a rounding error; networkx computes in float64 with a handful of roundings per edge."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import betweenness_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_betweenness_reserve", "g4s_betweenness")


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def test_constants_agree_across_layers():
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u?\b", text)}
    assert (d["BC_ACCUMULATE"], d["BC_BATCH"]) == (262144, 16)
    assert (capi.BC_ACCUMULATE, capi.BC_BATCH) == (262144, 16)
    others = [v for k, v in d.items() if not k.startswith("BC_") and re.search(r"#define\s+G4S_" + k + r"\s+\d+u", text)]
    assert len(others) > 10 and all(not (v & 262144) for v in others)     # the new bit is nobody else's
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+" + fn + r"\s*\(", text), fn
        assert fn in capi.SIGNATURES, fn
    assert C.sizeof(capi.BcInfo) == 48
    assert [n for n, _ in capi.BcInfo._fields_] == ["sources", "max_depth", "host_waits", "sigma_exact", "levels", "reached", "edges_walked", "sigma_max"]
    assert "g4s_betweenness(" in open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    src, flags = host._betweenness_args([3, 1, 3], 1.0, None, False)
    assert src.dtype == np.int32 and src.tolist() == [3, 1, 3] and flags == 0
    assert host._betweenness_args(7, 0.5, None, False)[0].tolist() == [7]
    assert callable(host.betweenness) and callable(host.CSR.betweenness) and callable(host.CSR.betweenness_reserve)


def test_symbols_are_exported():
    _, lib = _lib()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn), fn


def test_calls_reject_arguments_before_hip():
    capi, lib = _lib()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    out = (C.c_double * 4)()
    src = (C.c_int32 * 2)(0, 1)
    info = capi.BcInfo()
    fn = lib.g4s_betweenness
    err = lambda: lib.g4s_last_error().decode()
    for b in [1 << i for i in range(32) if i != 18]:
        for base in (0, capi.BC_ACCUMULATE):
            assert fn(fake, src, 2, 1.0, out, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
            assert "flags" in err()
    for b in [1 << i for i in range(32)]:                             # the reserve accepts no bit
        assert lib.g4s_csr_betweenness_reserve(fake, b) == capi.ERR_INVALID, b
        assert "flags" in err()
    assert lib.g4s_csr_betweenness_reserve(None, 0) == capi.ERR_INVALID and "handle" in err()
    for f in (0, capi.BC_ACCUMULATE):
        assert fn(None, src, 2, 1.0, out, f, None, None) == capi.ERR_INVALID and "handle" in err()
        assert fn(fake, None, 2, 1.0, out, f, None, None) == capi.ERR_INVALID and "sources" in err()
        assert fn(fake, src, 2, 1.0, None, f, None, None) == capi.ERR_INVALID and "bc_dev" in err()
        for n_src in (0, -1, -(1 << 31)):
            assert fn(fake, src, n_src, 1.0, out, f, None, None) == capi.ERR_INVALID and "sources" in err(), n_src
        for scale in (math.nan, math.inf, -math.inf):
            assert fn(fake, src, 2, scale, out, f, None, None) == capi.ERR_INVALID and "scale" in err(), scale
    # no other entry point takes the bit
    tinfo, pinfo = capi.TraverseInfo(), capi.PagerankInfo()
    assert lib.g4s_bfs(fake, src, 2, out, 0, capi.BC_ACCUMULATE, C.byref(tinfo), None) == capi.ERR_INVALID
    assert lib.g4s_sssp(fake, src, 2, out, 0, capi.BC_ACCUMULATE, C.byref(tinfo), None) == capi.ERR_INVALID
    assert lib.g4s_pagerank(fake, 0.85, 1e-10, 0, None, out, capi.BC_ACCUMULATE, C.byref(pinfo), None) == capi.ERR_INVALID
    assert lib.g4s_csr_traverse_reserve(fake, capi.BC_ACCUMULATE) == capi.ERR_INVALID
    assert lib.g4s_csr_pagerank_reserve(fake, capi.BC_ACCUMULATE) == capi.ERR_INVALID
    assert lib.g4s_spmv_semiring(fake, out, out, capi.BC_ACCUMULATE, None) == capi.ERR_INVALID


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    double bc[4];\n    int32_t s[2] = {0, 1};\n"
           "    g4s_bc_info info;\n    info.sources = 0;\n"
           "    if (argc > 5) { g4s::BetweennessCentrality(a, bc, s, 2); g4s::BetweennessCentrality(a, bc, s, 2, 0.5); g4s::BetweennessCentrality(a, bc, s, 1, 1.0, &info);\n"
           "        g4s_betweenness(nullptr, s, 2, 1.0, bc, G4S_BC_ACCUMULATE, &info, nullptr);\n"
           "        g4s_csr_betweenness_reserve(nullptr, 0u); }\n"
           "    static_assert(G4S_BC_BATCH >= 16, \"\");\n    static_assert(sizeof(g4s_bc_info) == 48, \"\");\n"
           "    return info.sources * 0 + (int)(sizeof(info.sigma_max) - 8 + sizeof(info.levels) - 8);\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_value_errors_before_any_gpu_call():
    import torch
    from g4s_amd import host
    for fn in (host.betweenness, host.CSR.betweenness):               # (no matrix, no device: the arguments are checked first)
        for sources in ([], None, "3", [1.5], [[1, 2], [3, 4]], [-1], [True], 1 << 31):
            with pytest.raises(ValueError, match="sources"):
                fn(None, sources)
        for scale in (math.nan, math.inf, "1", None, True):
            with pytest.raises(ValueError, match="scale"):
                fn(None, [0], scale=scale)
        with pytest.raises(ValueError, match="accumulate"):
            fn(None, [0], accumulate=1)
        with pytest.raises(ValueError, match="out"):
            fn(None, [0], accumulate=True)
        for bad in ([0.5, 0.5], np.ones(3), torch.ones(3, dtype=torch.float32), torch.ones(2, 2, dtype=torch.float64), torch.ones(3, dtype=torch.float64)):
            with pytest.raises(ValueError, match="out"):              # the last one: a host tensor
                fn(None, [0], out=bad)


def _networkx(arrays, sources):
    """Σ_s betweenness_centrality_subset(G, [s], all nodes, normalized=False) on the DiGraph of the nonzero entries."""
    import networkx as nx
    rp, ci, va = arrays
    n = len(rp) - 1
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    src = np.repeat(np.arange(n), np.diff(rp))
    keep = np.asarray(va) != 0
    G.add_edges_from(zip(src[keep].tolist(), np.asarray(ci)[keep].tolist()))
    assert G.number_of_edges() == int(keep.sum())                     # no parallel edges: a DiGraph would merge them
    total = np.zeros(n)
    nodes = list(range(n))
    for s in sources:
        b = nx.betweenness_centrality_subset(G, [s], nodes, normalized=False)
        total += np.array([b[v] for v in nodes])
    return total


CASES = {
    "rmat10": (lambda: bref.rmat_directed(10, 8, 77), [0, 1, 5, 700, 700]),
    "grid33x17": (lambda: bref.grid(33, 17), [0, 280, 560]),
    "rmat9s": (lambda: bref.rmat_symmetric(9, 4, 78), list(range(0, 512, 37))),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_networkx(name):
    build, sources = CASES[name]
    arrays = build()
    n = len(arrays[0]) - 1
    ref = bref.betweenness(*arrays, n, sources)
    want = _networkx(arrays, sources)
    got = ref.bc.astype(np.float64)
    diff = np.abs(ref.bc - want.astype(np.longdouble))
    print(f"{name}: n {n}, nnz {arrays[1].size}, depth {ref.max_depth}, sigma max {float(ref.sigma_max):.4g}, bc max {got.max():.6g}, "
          f"max |ref - nx| {float(diff.max()):.3e}, max relative {float((diff[ref.bc > 0] / ref.bc[ref.bc > 0]).max()):.3e}")
    assert got.max() > 10 and ref.max_depth >= 3
    assert np.all(diff <= bref.PARITY * ref.bc)
    assert np.all(want[ref.bc == 0] == 0)
    if name == "rmat10":
        assert (np.diff(arrays[0]) == 0).sum() > 50                   # empty rows, and vertices no source reaches
        assert ref.reached < len(sources) * n
    # a missed edge is far outside the bar: the comparison can fail
    rp, ci, va = arrays
    u = int(np.argmax(ref.bc))
    k = int(rp[u])
    va2 = va.copy()
    va2[k] = 0.0
    worse = bref.betweenness(rp, ci, va2, n, sources)
    assert np.any(np.abs(worse.bc - ref.bc) > 1e6 * bref.PARITY * ref.bc)


def test_reference_edge_rule_and_closed_forms():
    """A stored zero is no edge, NaN is one, a repeated column is a parallel edge; the closed forms the exact GPU cases rely on."""
    # 0 → 1 → 3, 0 → 2 → 3, 3 → 4, plus a second 0 → 1: σ[3] = 3 with two of the three paths through 1
    arrays = bref.csr_of_edges(5, [0, 0, 0, 1, 2, 3], [1, 1, 2, 3, 3, 4], np.ones(6))
    r = bref.betweenness(*arrays, 5, [0])
    assert float(r.sigma_max) == 3.0 and r.max_depth == 3 and r.levels == 4 and r.reached == 5
    assert np.array_equal(r.bc.astype(np.float64), np.array([0.0, 4.0 / 3.0, 2.0 / 3.0, 1.0, 0.0]))
    rp, ci, va = arrays
    va_nan, va_zero = va.copy(), va.copy()
    va_nan[0] = math.nan
    va_zero[0] = 0.0
    assert np.array_equal(bref.betweenness(rp, ci, va_nan, 5, [0]).bc, r.bc)
    single = bref.csr_of_edges(5, [0, 0, 1, 2, 3], [1, 2, 3, 3, 4], np.ones(5))
    assert np.array_equal(bref.betweenness(rp, ci, va_zero, 5, [0]).bc, bref.betweenness(*single, 5, [0]).bc)
    assert np.array_equal(bref.betweenness(*single, 5, [0]).bc.astype(np.float64), np.array([0.0, 1.0, 1.0, 1.0, 0.0]))
    # a repeated source counts twice; scale multiplies
    assert np.array_equal(bref.betweenness(*single, 5, [0, 0], scale=0.5).bc, bref.betweenness(*single, 5, [0]).bc)
    p = bref.betweenness(*bref.path(300), 300, [0])
    assert np.array_equal(p.bc.astype(np.float64), np.concatenate([[0.0], 299.0 - np.arange(1, 300)])) and p.max_depth == 299
    k = 40
    dm = bref.betweenness(*bref.diamonds(k), 3 * k + 1, [0])
    assert float(dm.sigma_max) == 2.0 ** k and dm.max_depth == 2 * k
    a = 3 * np.arange(1, k)
    assert np.array_equal(dm.bc[a].astype(np.float64), 3.0 * (k - np.arange(1, k)))          # every path to a later vertex passes a_i
    assert np.array_equal(dm.bc[a + 1].astype(np.float64), (1.0 + 3.0 * (k - np.arange(1, k) - 1)) / 2.0)
    s = bref.betweenness(*bref.star(5000), 5001, [0, 1])
    assert float(s.bc[0]) == 4999.0 and not s.bc[1:].any() and s.max_depth == 2 and s.reached == 2 * 5001
