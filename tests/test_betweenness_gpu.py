"""g4s_betweenness on the GPU, through the C-ABI via g4s_amd.host, against the longdouble reference of tests/betweenness_ref.py.

The bar is the project's fp64 parity bar: |bc − ref| <= 1e-10 · ref, and bc == 0 exactly where ref is 0. Every term of σ, δ and the sum
over sources is non-negative, so Σ|terms| is the value itself and the bar is relative to it; a float64 run carries a few roundings per edge of the
shortest-path DAG, some 1e4 times below the bar at these sizes. Where σ is 1 or a power of two every δ is dyadic and the comparison is `==`.
Largest err / ref observed on one MI355X: see DESIGN §4.10."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import betweenness_ref as bref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO53 = 2.0 ** 53


def _host():
    from g4s_amd import capi, host
    return capi, host


def _from_arrays(arrays, **kw):
    _, host = _host()
    rp, ci, va = arrays
    n = len(rp) - 1
    return host.CSR.from_host(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64), n, n, **kw)


def _check_info(label, info, ref, n_sources):
    capi, _ = _host()
    print(f"betweenness {label}: {info}")
    assert info["sources"] == n_sources
    assert (info["levels"], info["reached"], info["max_depth"]) == (ref.levels, ref.reached, ref.max_depth), (label, info, ref[1:])
    assert info["host_waits"] <= math.ceil(info["levels"] / capi.BC_BATCH) + 2 * n_sources, (label, info)
    assert info["sigma_exact"] == (1 if float(ref.sigma_max) <= TWO53 else 0)
    if info["sigma_exact"]:
        assert info["sigma_max"] == float(ref.sigma_max)
    assert info["edges_walked"] >= info["reached"] - n_sources


def _run(label, arrays, sources, exact=False, A=None, ref=None, **kw):
    n = len(arrays[0]) - 1
    if ref is None:
        ref = bref.betweenness(*arrays, n, sources, scale=kw.get("scale", 1.0))
    A = A or _from_arrays(arrays)
    bc, info = A.betweenness(sources, **kw)
    _check_info(label, info, ref, len(np.atleast_1d(sources)))
    got = bc.cpu().numpy()
    worst = bref.check_parity(label, got, ref.bc)
    if exact:
        assert np.array_equal(got, ref.bc.astype(np.float64)), label
        assert worst == 0.0 and info["sigma_exact"] == 1
    return bc, info, ref


@pytest.fixture(scope="module")
def grid():
    arrays, sources = bref.grid(33, 17), [0, 280, 560]
    return arrays, sources, bref.betweenness(*arrays, 33 * 17, sources)


@pytest.fixture(scope="module")
def rmat13hub():
    arrays = bref.with_hub(bref.rmat_symmetric(13, 8, 20261017), 0, 5000, 5)
    sources = [0, 1, 77, 4001]
    rp = arrays[0]
    assert rp[1] - rp[0] > 4096                                       # vertex 0 is a hub: the chunked forward walk and the workgroup sum
    assert (np.diff(rp) > 4096).sum() == 1 and np.diff(rp)[1:].max() > 64
    ref = bref.betweenness(*arrays, 1 << 13, sources)
    assert float(ref.sigma_max) > 100 and ref.bc[0] > 1e4             # a hub with non-trivial σ that many paths cross
    return arrays, sources, ref


@pytest.fixture(scope="module")
def tree():
    return bref.binary_tree(8191)


# ---------------------------------------------------------------------------------------------- 1. exact cases
def test_exact_path_spans_several_batches():
    capi, _ = _host()
    bc, info, _ = _run("path 300", bref.path(300), [0], exact=True)
    assert np.array_equal(bc.cpu().numpy(), np.concatenate([[0.0], 299.0 - np.arange(1, 300)]))
    assert info["max_depth"] == 299 and info["levels"] == 300 > 4 * capi.BC_BATCH and info["host_waits"] < 300 // capi.BC_BATCH


def test_exact_star_with_a_hub():
    arrays = bref.star(5000)
    assert arrays[0][1] - arrays[0][0] == 5000                        # the centre is above the hub cut of 4096 edges
    bc, info, _ = _run("star 5000", arrays, [0, 1], exact=True)
    assert bc[0].item() == 4999.0 and info["max_depth"] == 2


def test_exact_binary_tree_many_tiles(tree):
    bc, info, ref = _run("tree 8191", tree, [0, 8190], exact=True)    # its last level: 4096 vertices, 16 workgroup tiles
    assert info["max_depth"] == 24 and info["reached"] == 2 * 8191
    assert np.array_equal(bc.cpu().numpy(), np.round(bc.cpu().numpy()))


def test_exact_diamond_chain_sigma_2_to_40():
    k = 40
    bc, info, _ = _run("40 diamonds", bref.diamonds(k), [0], exact=True)
    assert info["sigma_max"] == 2.0 ** k and info["max_depth"] == 2 * k
    a = 3 * np.arange(1, k)
    assert np.array_equal(bc.cpu().numpy()[a + 1], (1.0 + 3.0 * (k - np.arange(1, k) - 1)) / 2.0)


# ---------------------------------------------------------------------------------------------- 2. tolerance cases
def test_rmat_directed_with_empty_rows_and_a_repeated_source():
    arrays, sources = bref.rmat_directed(10, 8, 77), [0, 1, 5, 700, 700]
    _, info, ref = _run("rmat10 directed", arrays, sources)
    assert (np.diff(arrays[0]) == 0).sum() > 50 and ref.reached < 5 * 1024
    once = bref.betweenness(*arrays, 1024, [0, 1, 5, 700])
    assert np.any(ref.bc != once.bc)                                  # the repeated source counts twice


def test_grid(grid):
    arrays, sources, ref = grid
    _run("grid 33x17", arrays, sources, ref=ref)


def test_rmat_symmetric():
    _run("rmat9 symmetrised", bref.rmat_symmetric(9, 4, 78), list(range(0, 512, 37)))


def test_rmat13_with_a_hub(rmat13hub):
    arrays, sources, ref = rmat13hub
    _run("rmat13 + hub", arrays, sources, ref=ref)


# ---------------------------------------------------------------------------------------------- 3. the edge rule
def test_edge_rule_zeros_nan_parallel_edges_and_update_values():
    n, sources = 300, [0, 5, 17]
    rng = np.random.default_rng(31)
    key = np.unique(rng.integers(0, n, 1500) * n + rng.integers(0, n, 1500))
    src, dst = key // n, key % n
    plain = bref.csr_of_edges(n, src, dst, np.ones(src.size))
    base = bref.betweenness(*plain, n, sources)
    # stored zeros are no edges
    zs, zd = rng.integers(0, n, 400), rng.integers(0, n, 400)
    zeros = bref.csr_of_edges(n, np.concatenate([src, zs]), np.concatenate([dst, zd]), np.concatenate([np.ones(src.size), np.zeros(400)]))
    bc, _, ref = _run("stored zeros", zeros, sources)
    assert np.array_equal(ref.bc, base.bc)
    # a NaN weight is an edge
    va = plain[2].copy()
    va[::7] = math.nan
    bc, _, ref = _run("NaN weights", (plain[0], plain[1], va), sources)
    assert np.array_equal(ref.bc, base.bc)
    # repeated columns are parallel edges
    dup = rng.permutation(src.size)[:300]
    multi = bref.csr_of_edges(n, np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]]), np.ones(src.size + 300))
    bc, _, ref = _run("parallel edges", multi, sources)
    assert np.any(ref.bc != base.bc) and float(ref.sigma_max) > float(base.sigma_max)
    # update_values turns an entry to zero: the next call drops that edge (the handle had no stored zero before)
    A = _from_arrays(plain)
    _run("before the update", plain, sources, A=A, ref=base)
    rp, ci, _ = plain
    k = int(rp[0])                                                    # the first out-edge of source 0
    va2 = np.ones(ci.size)
    va2[k] = 0.0
    less = bref.betweenness(rp, ci, va2, n, sources)
    assert np.any(less.bc != base.bc)
    A.update_values(torch.from_numpy(va2).cuda())
    _run("after the update", (rp, ci, va2), sources, A=A, ref=less)
    A.update_values(torch.from_numpy(np.full(ci.size, 2.5)).cuda())
    _run("after the repair", plain, sources, A=A, ref=base)


# ---------------------------------------------------------------------------------------------- 4. scale and G4S_BC_ACCUMULATE
def test_scale_and_accumulate(tree, grid):
    sources = [0, 8190, 5, 4095]
    A = _from_arrays(tree)
    whole, _ = A.betweenness(sources)
    half, _ = A.betweenness(sources[:2])
    both, info = A.betweenness(sources[2:], out=half, accumulate=True)
    assert both is half and info["sources"] == 2
    assert torch.equal(both, whole)                                   # the δ are integers there
    ref = bref.betweenness(*tree, 8191, sources)
    assert np.array_equal(whole.cpu().numpy(), ref.bc.astype(np.float64))
    arrays, gsources, gref = grid
    G = _from_arrays(arrays)
    whole, _ = G.betweenness(gsources)
    part, _ = G.betweenness(gsources[:1])
    G.betweenness(gsources[1:], out=part, accumulate=True)
    w = whole.cpu().numpy()
    assert np.all(np.abs(part.cpu().numpy() - w) <= bref.PARITY * w)
    bref.check_parity("grid, two accumulating calls", part.cpu().numpy(), gref.bc)
    # scale = 0.5 is networkx's undirected value
    import networkx as nx
    rp, ci, _ = arrays
    n = len(rp) - 1
    U = nx.Graph()
    U.add_nodes_from(range(n))
    U.add_edges_from(zip(np.repeat(np.arange(n), np.diff(rp)).tolist(), ci.tolist()))
    b = nx.betweenness_centrality_subset(U, gsources, list(range(n)), normalized=False)
    want = np.array([b[v] for v in range(n)])
    halfbc, _ = G.betweenness(gsources, scale=0.5)
    got = halfbc.cpu().numpy()
    assert np.all(np.abs(got - want) <= bref.PARITY * want) and np.all(got[want == 0] == 0)
    bref.check_parity("grid, scale 0.5", got, bref.betweenness(*arrays, n, gsources, scale=0.5).bc)


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_same_bits_on_every_run_and_stream(grid, rmat13hub):
    for label, (arrays, sources, ref) in (("grid", grid), ("rmat13 + hub", rmat13hub)):
        A = _from_arrays(arrays)
        first, info = A.betweenness(sources)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            second, info2 = A.betweenness(sources)
        torch.cuda.synchronize()
        assert info["sigma_exact"] == 1 and info2["sigma_exact"] == 1, label
        assert torch.equal(first, second), label
        fresh, _ = _from_arrays(arrays).betweenness(sources)         # and on another handle
        assert torch.equal(first, fresh), label


# ---------------------------------------------------------------------------------------------- 6. large σ
def test_sigma_above_2_to_53_is_flagged():
    arrays = bref.grid(60, 60)
    _, info, ref = _run("grid 60x60 from a corner", arrays, [0])
    assert abs(float(ref.sigma_max) - math.comb(118, 59)) <= 1e-15 * math.comb(118, 59) and float(ref.sigma_max) > TWO53
    assert info["sigma_exact"] == 0 and math.isfinite(info["sigma_max"])
    assert abs(info["sigma_max"] - float(ref.sigma_max)) <= 1e-10 * float(ref.sigma_max)


def test_sigma_overflow_is_an_error_status_and_the_handle_stays_usable():
    capi, _ = _host()
    k = 1100
    arrays = bref.diamonds(k)
    assert len(arrays[0]) - 1 == 3301
    A = _from_arrays(arrays)
    with pytest.raises(capi.G4SError) as e:
        A.betweenness([0])
    assert e.value.status == capi.ERR_OVERFLOW and "sources[0]" in str(e.value)
    torch.cuda.synchronize()
    start = 3 * (k - 40)                                              # the last 40 diamonds: σ = 2^40 again
    bc, info = A.betweenness([start])
    assert info["sigma_max"] == 2.0 ** 40 and info["sigma_exact"] == 1 and info["max_depth"] == 80
    got = bc.cpu().numpy()
    assert not got[:start + 1].any()
    tail = bref.betweenness(*bref.diamonds(40), 121, [0])
    assert np.array_equal(got[start:], tail.bc.astype(np.float64))


# ---------------------------------------------------------------------------------------------- 7. workspace and contract corners
def test_workspace_is_reserved_once_and_counted(rmat13hub):
    capi, _ = _host()
    arrays, sources, ref = rmat13hub
    n, nnz = len(arrays[0]) - 1, arrays[1].size
    A = _from_arrays(arrays)
    bytes0 = A.info()["plan_bytes"]
    A.betweenness_reserve()
    hub = min(n, nnz // 4097) + 1
    documented = 4 * (3 * n + 2 + 2 * hub) + (n + 2) + 24 * n + 104   # include/g4s.h
    assert A.info()["plan_bytes"] == bytes0 + documented
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    A.betweenness(sources, out=out)                                   # (the first launches load the kernels)
    torch.cuda.synchronize()
    for attempt in range(3):                                          # the device is shared: another tenant can move the figure, never hide a growth
        free0 = torch.cuda.mem_get_info()[0]
        _, info = A.betweenness(sources, out=out)
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        if free1 == free0:
            break
    assert free1 == free0, (free0, free1)
    assert A.info()["plan_bytes"] == bytes0 + documented
    _check_info("after the reserve", info, ref, len(sources))
    bref.check_parity("after the reserve", out.cpu().numpy(), ref.bc)
    A.betweenness_reserve()                                           # a second reserve adds nothing
    assert A.info()["plan_bytes"] == bytes0 + documented


def test_contract_corners(grid):
    capi, host = _host()
    lib = capi.load()
    arrays, sources, ref = grid
    n = len(arrays[0]) - 1
    A = _from_arrays(arrays)
    A.betweenness_reserve()
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    src = (C.c_int32 * 3)(*sources)
    # a non-square handle, a source outside [0, rows)
    R = host.CSR.from_host(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 1.0]), 2, 3)
    assert lib.g4s_betweenness(R.handle, src, 1, 1.0, C.c_void_p(out.data_ptr()), 0, None, None) == capi.ERR_INVALID
    assert "square" in lib.g4s_last_error().decode()
    assert lib.g4s_csr_betweenness_reserve(R.handle, 0) == capi.ERR_INVALID
    with pytest.raises(ValueError, match="square"):
        R.betweenness([0])
    for bad in (-1, n, 1 << 30):
        s2 = (C.c_int32 * 2)(0, bad)
        assert lib.g4s_betweenness(A.handle, s2, 2, 1.0, C.c_void_p(out.data_ptr()), 0, None, None) == capi.ERR_INVALID
        assert "sources" in lib.g4s_last_error().decode()
    with pytest.raises(ValueError, match="sources"):
        A.betweenness([0, n])
    assert not out.any()                                              # nothing ran
    # a capturing stream is refused, the capture stays valid and the handle still works
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_betweenness(A.handle, src, 3, 1.0, C.c_void_p(out.data_ptr()), 0, None, C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and "captured" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda")) and not out.any()
    _run("after the refused capture", arrays, sources, A=A, ref=ref)
    lvl, _ = A.bfs(sources[:1], direction="push")                     # the other kernels of the handle are untouched
    assert int(lvl.max()) == 48


CPP_BC = r"""
#include <cstdio>
#include <vector>
#include "g4s/csr.hpp"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    int n = 0, nnz = 0, ns = 0;
    if (!f || std::fscanf(f, "%d %d %d", &n, &nnz, &ns) != 3) return 2;
    std::vector<int32_t> rp(n + 1), ci(nnz), src(ns);
    std::vector<double> va(nnz, 1.0);
    for (auto &v : rp) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : ci) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : src) if (std::fscanf(f, "%d", &v) != 1) return 2;
    std::fclose(f);
    g4s::CSR<int32_t, double> a(rp.data(), ci.data(), va.data(), n, n, nnz);
    std::vector<double> bc(n, -7.0), half(n, -7.0);
    g4s_bc_info info;
    g4s::BetweennessCentrality(a, bc.data(), src.data(), (int32_t)ns, 1.0, &info);
    g4s::BetweennessCentrality(a, half.data(), src.data(), (int32_t)ns, 0.5);
    for (int i = 0; i < n; ++i) if (half[i] != 0.5 * bc[i]) return 3;
    std::printf("%d %d %d %lld %lld %.17g\n", info.sources, info.max_depth, info.sigma_exact, (long long)info.levels, (long long)info.reached, info.sigma_max);
    for (double v : bc) std::printf("%.17g\n", v);
    int32_t bad = n;
    try { g4s::BetweennessCentrality(a, bc.data(), &bad, (int32_t)1); return 4; } catch (const std::runtime_error &) {}
    g4s::CSR<int32_t, double> wide(rp.data(), ci.data(), va.data(), n, n + 1, nnz);
    try { g4s::BetweennessCentrality(wide, bc.data(), src.data(), (int32_t)ns); return 5; } catch (const std::runtime_error &) {}
    return 0;
}
"""


def test_cpp_header_form_runs(tmp_path, grid):
    arrays, sources, ref = grid
    rp, ci, _ = arrays
    n = len(rp) - 1
    src, exe, inp = tmp_path / "bc.cpp", str(tmp_path / "bc"), tmp_path / "a.txt"
    src.write_text(CPP_BC)
    lib = os.path.join(ROOT, "g4s_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lg4s_hip", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    inp.write_text(f"{n} {ci.size} {len(sources)}\n" + "\n".join(map(str, rp)) + "\n" + "\n".join(map(str, ci)) + "\n" + "\n".join(map(str, sources)) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split()
    assert [int(v) for v in lines[:5]] == [len(sources), ref.max_depth, 1, ref.levels, ref.reached]
    assert float(lines[5]) == float(ref.sigma_max)
    bref.check_parity("C++ form, grid", np.array(lines[6:6 + n], dtype=np.float64), ref.bc)
