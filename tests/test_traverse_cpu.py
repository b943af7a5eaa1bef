"""g4s_sssp / g4s_bfs without a GPU: constants in every layer, exported symbols, argument checking before any HIP call (G4S_ERR_INVALID), the C++
forms of include/g4s/csr.hpp (compile only), the Python ValueErrors, and the numpy reference of tests/traverse_ref.py against scipy.sparse.csgraph —
so that the yardstick of the GPU tests is pinned to something this project did not write."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers, traverse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = ("g4s_csr_traverse_reserve", "g4s_sssp", "g4s_bfs")


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def test_flag_values_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+G4S_(\w+)\s+(\d+)u?\b", text)}
    assert (d["TRAVERSE_PUSH"], d["TRAVERSE_PULL"], d["TRAVERSE_SYMMETRIC"]) == (4096, 8192, 16384)
    for name in ("TRAVERSE_PUSH", "TRAVERSE_PULL", "TRAVERSE_SYMMETRIC", "TRAVERSE_BATCH"):
        assert getattr(capi, name) == d[name], name
    assert capi.TRAVERSE_BATCH >= 8
    others = [v for k, v in d.items() if not k.startswith("TRAVERSE_") and re.search(r"#define\s+G4S_" + k + r"\s+\d+u", text)]
    for bit in (4096, 8192, 16384):                                   # the new bits are nobody else's
        assert all(not (v & bit) for v in others), bit
    for fn in FUNCTIONS:
        assert re.search(r"g4s_status\s+" + fn + r"\s*\(", text), fn
        assert fn in capi.SIGNATURES, fn
    assert C.sizeof(capi.TraverseInfo) == 40
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_sssp(" in hpp and "g4s_bfs(" in hpp


def test_symbols_are_exported():
    _, lib = _lib()
    for fn in FUNCTIONS:
        assert hasattr(lib, fn), fn


def test_calls_reject_arguments_before_hip():
    capi, lib = _lib()
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    src = (C.c_int32 * 2)(0, 1)
    out = (C.c_double * 4)()
    info = capi.TraverseInfo()
    ok_flags = (0, capi.TRAVERSE_PUSH, capi.TRAVERSE_PULL, capi.TRAVERSE_SYMMETRIC, capi.TRAVERSE_PUSH | capi.TRAVERSE_SYMMETRIC)
    for fn in (lib.g4s_sssp, lib.g4s_bfs):
        for b in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1536, 2048, 32768, 1 << 20, 1 << 31):
            for base in ok_flags:
                assert fn(fake, src, 2, out, 0, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
        assert fn(fake, src, 2, out, 0, capi.TRAVERSE_PUSH | capi.TRAVERSE_PULL, None, None) == capi.ERR_INVALID
        assert "together" in lib.g4s_last_error().decode()
        for f in ok_flags:
            assert fn(None, src, 2, out, 0, f, None, None) == capi.ERR_INVALID
            assert fn(fake, None, 2, out, 0, f, None, None) == capi.ERR_INVALID
            assert fn(fake, src, 2, None, 0, f, None, None) == capi.ERR_INVALID
            assert fn(fake, src, 0, out, 0, f, None, None) == capi.ERR_INVALID
            assert fn(fake, src, -3, out, 0, f, None, None) == capi.ERR_INVALID
            assert fn(fake, src, 2, out, -1, f, None, None) == capi.ERR_INVALID
        assert "cap" in lib.g4s_last_error().decode()
    for b in (1, 8, 16, 128, 512, 2048, 32768, 1 << 31, capi.TRAVERSE_PUSH | capi.TRAVERSE_PULL):
        assert lib.g4s_csr_traverse_reserve(fake, b) == capi.ERR_INVALID, b
    for f in ok_flags:
        assert lib.g4s_csr_traverse_reserve(None, f) == capi.ERR_INVALID


def test_cpp_forms_compile(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    double d[4]; int32_t l[4]; int32_t s[2] = {0, 1};\n"
           "    g4s_traverse_info info;\n"
           "    if (argc > 5) { g4s::SSSP(a, s, 2, d); g4s::SSSP(a, s, 2, d, &info); g4s::SSSP(a, 0, d); g4s::BFS(a, s, 2, l); g4s::BFS(a, s, 2, l, &info); g4s::BFS(a, 1, l);\n"
           "        g4s_sssp(nullptr, s, 2, d, 0, G4S_TRAVERSE_PUSH | G4S_TRAVERSE_SYMMETRIC, &info, nullptr); g4s_csr_traverse_reserve(nullptr, G4S_TRAVERSE_PULL); }\n"
           "    return info.iterations * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_value_errors_before_any_gpu_call():
    from g4s_amd import host
    for name in ("bogus", "PUSH", "", None, 3):
        for fn in (host.sssp, host.bfs):
            with pytest.raises(ValueError, match="direction"):
                fn(None, [0], direction=name)                         # (no matrix, no device: the name is checked first)
        for fn in (host.CSR.sssp, host.CSR.bfs):
            with pytest.raises(ValueError, match="direction"):
                fn(None, [0], direction=name)
        with pytest.raises(ValueError, match="direction"):
            host.CSR.traverse_reserve(None, direction=name)


@pytest.mark.parametrize("seed", [3, 11])
def test_reference_equals_scipy(seed):
    """The fixed point of the synchronous min-plus iteration is Dijkstra's answer bit for bit (both sum a path left to right and take the minimum),
    and the or-and loop gives scipy's hop counts."""
    from scipy.sparse.csgraph import dijkstra, shortest_path
    n = 5000
    rp, ci, va = helpers.random_csr(n, n, 0.002, seed)
    va = np.random.default_rng(seed).uniform(0.05, 1.0, va.size)
    G = helpers.to_scipy(rp, ci, va, n, n)
    d, rounds, converged, after = traverse_ref.sssp(rp, ci, va, n, [7], keep=(2,))
    assert converged and rounds < 40
    assert np.isfinite(d).sum() > n // 2
    assert np.array_equal(d, dijkstra(G, directed=True, indices=7))
    assert np.all(d <= after[2]) and not np.array_equal(d, after[2])
    level, depth = traverse_ref.bfs(rp, ci, va, n, [7])
    hops = shortest_path(G, directed=True, unweighted=True, indices=7)
    assert np.array_equal(level, np.where(np.isfinite(hops), hops, -1).astype(np.int32))
    assert depth == level.max()
    # several sources: the distance to the nearest
    d2, _, _, _ = traverse_ref.sssp(rp, ci, va, n, [7, 99, 7])
    assert np.array_equal(d2, dijkstra(G, directed=True, indices=[7, 99]).min(axis=0))
