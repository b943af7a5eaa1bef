"""g4s_pagerank without a GPU: constants in every layer, exported symbols, argument checking before any HIP call (G4S_ERR_INVALID), the C++ form of
include/g4s/csr.hpp (compile only), the Python ValueErrors, and the numpy reference of tests/pagerank_ref.py against networkx.pagerank — so that the
yardstick of the GPU tests is pinned to something this project did not write.

The bound of the networkx comparison: the iteration contracts in L1 by d = damping, so an iterate whose last step moved it by `residual` is within
residual · d / (1 − d) of the fixed point r*. networkx stops at residual < n · tol_nx, the reference at its own last residual; a float64 run carries
γ / (1 − d) of rounding (tests/test_pagerank_gpu.py derives γ). Hence ‖ref − nx‖₁ <= (n · tol_nx + residual_ref) · d / (1 − d) + γ / (1 − d)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pagerank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_pagerank_reserve", "g4s_pagerank")


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def test_flag_values_agree_across_layers():
    from g4s_amd import capi, host
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u?\b", text)}
    assert (d["PAGERANK_SYMMETRIC"], d["PAGERANK_WARM_START"], d["PAGERANK_BATCH"]) == (65536, 131072, 8)
    for name in ("PAGERANK_SYMMETRIC", "PAGERANK_WARM_START", "PAGERANK_BATCH"):
        assert getattr(capi, name) == d[name], name
    others = [v for k, v in d.items() if not k.startswith("PAGERANK_") and re.search(r"#define\s+G4S_" + k + r"\s+\d+u", text)]
    for bit in (65536, 131072):                                       # the new bits are nobody else's
        assert all(not (v & bit) for v in others), bit
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+" + fn + r"\s*\(", text), fn
        assert fn in capi.SIGNATURES, fn
    assert C.sizeof(capi.PagerankInfo) == 32
    assert [n for n, _ in capi.PagerankInfo._fields_] == ["iterations", "converged", "host_waits", "products", "dangling", "residual"]
    assert "g4s_pagerank(" in open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert host._pagerank_args(0.85, 1e-10, 0, None, None, False) == 0
    assert host._pagerank_args(0.0, 0.0, 7, None, None, True) == capi.PAGERANK_SYMMETRIC
    assert callable(host.pagerank) and callable(host.CSR.pagerank) and callable(host.CSR.pagerank_reserve)


def test_symbols_are_exported():
    _, lib = _lib()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn), fn


def test_calls_reject_arguments_before_hip():
    capi, lib = _lib()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    out = (C.c_double * 4)()
    info = capi.PagerankInfo()
    ok_flags = (0, capi.PAGERANK_SYMMETRIC, capi.PAGERANK_WARM_START, capi.PAGERANK_SYMMETRIC | capi.PAGERANK_WARM_START)
    fn = lib.g4s_pagerank
    for b in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 1 << 18, 1 << 20, 1 << 31):
        for base in ok_flags:
            assert fn(fake, 0.85, 1e-10, 0, None, out, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
            assert lib.g4s_csr_pagerank_reserve(fake, base | b) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in ok_flags:
        assert fn(None, 0.85, 1e-10, 0, None, out, f, None, None) == capi.ERR_INVALID
        assert fn(fake, 0.85, 1e-10, 0, None, None, f, None, None) == capi.ERR_INVALID
        for damping in (1.0, 1.5, -0.1, -1e-300, math.nan, math.inf, -math.inf):
            assert fn(fake, damping, 1e-10, 0, None, out, f, None, None) == capi.ERR_INVALID, damping
        assert "damping" in lib.g4s_last_error().decode()
        for tol in (-1e-300, -1.0, math.nan, -math.inf):
            assert fn(fake, 0.85, tol, 0, None, out, f, None, None) == capi.ERR_INVALID, tol
        assert "tol" in lib.g4s_last_error().decode()
        assert fn(fake, 0.85, 1e-10, -1, None, out, f, None, None) == capi.ERR_INVALID
        assert "cap" in lib.g4s_last_error().decode()
        assert lib.g4s_csr_pagerank_reserve(None, f) == capi.ERR_INVALID


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    double r[4], p[4] = {1, 0, 2, 1};\n"
           "    g4s_pagerank_info info;\n    info.iterations = 0;\n"
           "    if (argc > 5) { g4s::PageRank(a, r); g4s::PageRank(a, r, 0.9, 1e-8, 50); g4s::PageRank(a, r, 0.85, 0.0, 30, p, &info);\n"
           "        g4s_pagerank(nullptr, 0.85, 1e-10, 0, nullptr, r, G4S_PAGERANK_SYMMETRIC | G4S_PAGERANK_WARM_START, &info, nullptr);\n"
           "        g4s_csr_pagerank_reserve(nullptr, G4S_PAGERANK_SYMMETRIC); }\n"
           "    static_assert(G4S_PAGERANK_BATCH >= 8, \"\");\n"
           "    return info.iterations * 0 + (int)(sizeof(info.residual) - 8 + sizeof(info.dangling) - 8);\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_value_errors_before_any_gpu_call():
    import torch
    from g4s_amd import host
    for fn in (host.pagerank, host.CSR.pagerank):                     # (no matrix, no device: the arguments are checked first)
        for damping in (1.0, -0.5, math.nan, "0.85", None, True):
            with pytest.raises(ValueError, match="damping"):
                fn(None, damping=damping)
        for tol in (-1e-12, math.nan, "x", None):
            with pytest.raises(ValueError, match="tol"):
                fn(None, tol=tol)
        for cap in (-1, 2.5, None, 1 << 31):
            with pytest.raises(ValueError, match="max_iterations"):
                fn(None, max_iterations=cap)
        with pytest.raises(ValueError, match="symmetric"):
            fn(None, symmetric=1)
        for name in ("personalization", "start"):
            for bad in ([0.5, 0.5], np.ones(3), torch.ones(3, dtype=torch.float32), torch.ones(2, 2, dtype=torch.float64), torch.ones(3, dtype=torch.float64)):
                with pytest.raises(ValueError, match=name):       # the last one: a host tensor
                    fn(None, **{name: bad})
    with pytest.raises(ValueError, match="symmetric"):
        host.CSR.pagerank_reserve(None, symmetric="yes")


def _networkx(rp, ci, va, n, damping, tol_nx, personalization=None):
    import networkx as nx
    G = nx.MultiDiGraph()
    G.add_nodes_from(range(n))
    src = np.repeat(np.arange(n), np.diff(rp))
    G.add_weighted_edges_from(zip(src.tolist(), np.asarray(ci).tolist(), np.asarray(va).tolist()))
    pers = None if personalization is None else {v: float(personalization[v]) for v in range(n)}
    pr = nx.pagerank(G, alpha=damping, personalization=pers, max_iter=1000, tol=tol_nx, weight="weight")
    return np.array([pr[v] for v in range(n)])


def _fixed_point_bound(n, ref, damping, tol_nx):
    g = pagerank_ref.gamma(n, ref.max_in_degree, ref.max_out_degree)
    return (n * tol_nx + float(ref.residuals[-1])) * damping / (1.0 - damping) + g / (1.0 - damping)


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_reference_equals_networkx_rmat(dtype):
    scale, damping, tol_nx = 10, 0.85, 1e-13
    n = 1 << scale
    rp, ci, va = pagerank_ref.rmat_csr(scale, 8, 77)
    key = np.repeat(np.arange(n), np.diff(rp)).astype(np.int64) * n + ci
    assert np.unique(key).size < key.size                             # duplicate edges: repeated columns add
    pers = np.random.default_rng(3).uniform(0.0, 1.0, n)
    pers[::5] = 0.0
    for p in (None, pers):
        ref = pagerank_ref.pagerank(rp, ci, va, n, damping=damping, tol=1e-14, max_iterations=200, personalization=p, dtype=dtype)
        assert ref.dangling > 50 and ref.dangling == int(np.sum(np.add.reduceat(np.append(va, 0.0), np.minimum(rp[:-1], va.size)) * (np.diff(rp) > 0) == 0))
        assert len(ref.residuals) < 200 and ref.residuals[-1] < 1e-14
        want = _networkx(rp, ci, va, n, damping, tol_nx, p)
        dist = float(np.abs(ref.rank.astype(np.float64) - want).sum())
        bound = _fixed_point_bound(n, ref, damping, tol_nx)
        print(f"{dtype.__name__} personalised={p is not None}: iterations {len(ref.residuals)}, L1 distance {dist:.3e}, bound {bound:.3e}")
        assert dist <= bound
        assert abs(float(ref.rank.sum()) - 1.0) <= pagerank_ref.gamma(n, ref.max_in_degree, ref.max_out_degree) / (1.0 - damping)
    # one missed edge is far outside the bound: the comparison can fail
    k = int(rp[np.argmax(np.diff(rp))])                               # the first entry of the longest row
    keep = np.arange(ci.size) != k
    rp_less = (rp - (rp > k)).astype(np.int32)
    worse = pagerank_ref.pagerank(rp_less, ci[keep], va[keep], n, damping=damping, tol=1e-14, max_iterations=200, dtype=dtype)
    full = pagerank_ref.pagerank(rp, ci, va, n, damping=damping, tol=1e-14, max_iterations=200, dtype=dtype)
    assert float(np.abs(worse.rank - full.rank).sum()) > 1e3 * _fixed_point_bound(n, full, damping, tol_nx)


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_reference_three_cycle_and_isolated_vertices(dtype):
    rp, ci, va = pagerank_ref.csr_of_edges(3, [0, 1, 2], [1, 2, 0], [1.0, 2.5, 0.5])
    ref = pagerank_ref.pagerank(rp, ci, va, 3, damping=0.85, tol=0.0, max_iterations=40, dtype=dtype)
    g = pagerank_ref.gamma(3, 1, 1) / (1.0 - 0.85)
    assert ref.dangling == 0 and (ref.max_in_degree, ref.max_out_degree) == (1, 1)
    assert np.all(np.abs(ref.rank.astype(np.float64) - 1.0 / 3.0) <= g)          # exactly 1/3 each, up to the rounding the bound allows
    assert max(float(r) for r in ref.residuals) <= g
    assert np.abs(_networkx(rp, ci, va, 3, 0.85, 1e-13) - 1.0 / 3.0).max() <= 3 * 1e-13 * 0.85 / 0.15 + g
    for n in (64, 100):                                               # no edges: every vertex dangles, r = p
        rp0 = np.zeros(n + 1, np.int32)
        pers = np.random.default_rng(n).integers(0, 8, n).astype(np.float64) if n == 64 else None
        ref = pagerank_ref.pagerank(rp0, np.zeros(0, np.int32), np.zeros(0), n, damping=0.85, tol=0.0, max_iterations=25, personalization=pers, dtype=dtype)
        p = np.full(n, 1.0 / n) if pers is None else pers / pers.sum()
        assert ref.dangling == n and ref.max_in_degree == 0 and ref.max_out_degree == 0
        assert np.abs(ref.rank.astype(np.float64) - p).sum() <= pagerank_ref.gamma(n, 0, 0) / 0.15
        want = _networkx(rp0, [], [], n, 0.85, 1e-13, pers)
        assert np.abs(want - p).sum() <= n * 1e-13 * 0.85 / 0.15 + pagerank_ref.gamma(n, 0, 0) / 0.15
    ref = pagerank_ref.pagerank(np.zeros(65, np.int32), np.zeros(0, np.int32), np.zeros(0), 64, damping=0.5, tol=0.0, max_iterations=10, dtype=dtype)
    assert np.array_equal(ref.rank, np.full(64, dtype(1) / dtype(64)))   # powers of two: every operation is exact, r == p bit for bit
