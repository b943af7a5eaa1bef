"""g4s_connected_components on the device. Every comparison is exact: labels are canonical (the smallest vertex id of the component), so the
result is compared with == against tests/components_ref.py (pinned to scipy in test_components_cpu.py) or against canonicalised scipy itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import components_ref as cref
from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("G4S_CC_SAMPLE_ROUNDS", "G4S_CC_NO_SKIP")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _call(rp, ci, n, symmetric=False, device=True, fill=-7, check=True):
    """The C entry point itself, with `labels` pre-filled: (labels as numpy, info dict, status)."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.CCInfo()
    flags = capi.CC_SYMMETRIC if symmetric else 0
    if device:
        rp_t, ci_t = (rp if isinstance(rp, torch.Tensor) else _dev(rp)), (ci if isinstance(ci, torch.Tensor) else _dev(ci))
        lab = torch.full((max(n, 1),), fill, dtype=torch.int32, device="cuda")
        st = lib.g4s_connected_components(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), host._ptr_nn(lab), flags | capi.DEVICE_POINTERS, C.byref(info), host._stream())
        out = lab[:n].cpu().numpy()
    else:
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        out = np.full(max(n, 1), fill, np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.g4s_connected_components(n, P(rp_h), P(ci_h if ci_h.size else out), P(out), flags | capi.HOST_POINTERS, C.byref(info), None)
        out = out[:n]
    if check:
        capi.check(st)
    return out, {k: getattr(info, k) for k, _ in capi.CCInfo._fields_}, st


def _check_info(info, want):
    comps, largest, label = cref.stats(want)
    assert (info["components"], info["largest"], info["largest_label"]) == (comps, largest, label), info
    assert info["host_waits"] == 1, info


def _csr_from_edges(r, c, n):
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    order = np.argsort(r, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp).astype(np.int32), c[order].astype(np.int32)


def _symmetrised(rp, ci, n):
    import scipy.sparse as sp
    G = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    S = (G + G.T).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32)


# ------------------------------------------------------------------------------------------------ random graphs, both pointer kinds
@pytest.mark.parametrize("d,seed", [(0.5, 1), (1, 2), (2, 3), (4, 4)])
def test_random_graphs_device_and_host_pointers(d, seed):
    n = 50000
    rp, ci, _ = helpers.random_csr(n, n, d / n, seed)
    want, _ = cref.labels(rp, ci, n)
    for device, fill in ((True, -7), (True, n + 5), (False, -7), (False, n + 5)):
        got, info, _ = _call(rp, ci, n, device=device, fill=fill)
        assert np.array_equal(got, want), (device, fill)
        _check_info(info, want)
        assert info["skipped"] == 0 and info["sample_rounds"] == 2
        assert info["edges_linked"] == int(np.maximum(np.diff(rp) - 2, 0).sum())
    srp, sci = _symmetrised(rp, ci, n)
    got, info, _ = _call(srp, sci, n, symmetric=True)
    assert np.array_equal(got, want)
    _check_info(info, want)
    print(f"random d={d}: {info}")


def test_grid_is_one_component():
    from g4s_amd import host
    A = host.laplacian_csr(5, 1000, 1000)
    n = A.rows
    for sym in (False, True):
        lab, info = A.connected_components(symmetric=sym, return_info=True)
        assert lab.dtype == torch.int32 and lab.is_cuda and lab.numel() == n
        assert torch.equal(lab, torch.zeros(n, dtype=torch.int32, device="cuda"))
        assert (info["components"], info["largest"], info["largest_label"], info["host_waits"]) == (1, n, 0, 1)
        assert info["skipped"] == int(sym)
        print(f"grid symmetric={sym}: {info}")


def test_permuted_path_whole_and_in_pieces():
    n = 1 << 20
    perm = np.random.default_rng(20250101).permutation(n)
    rp, ci = _csr_from_edges(perm[:-1], perm[1:], n)                  # every vertex stores only the edge to its successor
    got, info, _ = _call(rp, ci, n)
    assert np.array_equal(got, np.zeros(n, np.int32))
    assert (info["components"], info["largest"], info["largest_label"]) == (1, n, 0)
    cuts = np.sort(np.random.default_rng(7).choice(n - 1, 999, replace=False))
    keep = np.ones(n - 1, bool)
    keep[cuts] = False
    rp, ci = _csr_from_edges(perm[:-1][keep], perm[1:][keep], n)
    want, k = cref.scipy_labels(rp, ci, n)
    assert k == 1000
    got, info, _ = _call(rp, ci, n)
    assert np.array_equal(got, want)
    _check_info(info, want)


def test_natural_order_path_and_banded_pattern():
    """Chains in vertex order: the deepest forest the sampling rounds can build (depth n before the compress)."""
    from g4s_amd import host
    n = 1 << 20
    rp, ci = _csr_from_edges(np.arange(n - 1), np.arange(1, n), n)
    got, info, _ = _call(rp, ci, n)
    assert np.array_equal(got, np.zeros(n, np.int32)) and info["components"] == 1
    rp, ci = _csr_from_edges(np.arange(1, n), np.arange(n - 1), n)    # stored from the other end
    got, info, _ = _call(rp, ci, n)
    assert np.array_equal(got, np.zeros(n, np.int32)) and info["components"] == 1
    B = host.banded_csr(200000, 3, 5)
    lab = B.connected_components(symmetric=True)
    assert torch.equal(lab, torch.zeros(200000, dtype=torch.int32, device="cuda"))


def test_star_with_the_hub_last():
    leaves = 1 << 20
    n, hub = leaves + 1, leaves
    from_hub = _csr_from_edges(np.full(leaves, hub), np.arange(leaves), n)
    from_leaves = _csr_from_edges(np.arange(leaves), np.full(leaves, hub), n)
    both = _symmetrised(*from_hub, n)
    zeros = np.zeros(n, np.int32)
    for (rp, ci), sym in ((from_hub, False), (from_leaves, False), (both, True), (both, False)):
        got, info, _ = _call(rp, ci, n, symmetric=sym)
        assert np.array_equal(got, zeros), sym
        assert (info["components"], info["largest"], info["largest_label"]) == (1, n, 0)
    got, info, _ = _call(*from_hub, n)
    assert info["edges_linked"] == leaves - 2                         # the hub row: everything behind the two sampled entries


@pytest.mark.parametrize("scale", [16, 20])
def test_rmat_as_given_transposed_and_symmetrised(scale):
    from g4s_amd import host
    n = 1 << scale
    A = host.rmat_csr(n, scale, 8 * n, 20240522)
    rp, ci, _ = A.to_host()
    want, k = cref.scipy_labels(rp, ci, n)
    lab, info = A.connected_components(return_info=True)
    assert np.array_equal(lab.cpu().numpy(), want)
    _check_info(info, want)
    assert info["skipped"] == 0 and info["edges_linked"] == int(np.maximum(np.diff(rp) - 2, 0).sum())
    trp, tci, _ = host.csr_transpose(A.rowptr, A.colids, None, n, n)
    lab_t = host.connected_components((trp, tci))
    srp, sci = _symmetrised(rp, ci, n)
    lab_s, info_s = host.connected_components((_dev(srp), _dev(sci)), symmetric=True, return_info=True)
    assert torch.equal(lab_t, lab) and torch.equal(lab_s, lab)
    _check_info(info_s, want)
    assert info_s["largest"] > n // 4                                 # a giant component: its rows are skipped
    assert info_s["skipped"] == 1 and info_s["edges_linked"] < sci.size
    lab_n, info_n = host.connected_components((_dev(srp), _dev(sci)), symmetric=False, return_info=True)
    assert torch.equal(lab_n, lab)
    assert info_n["skipped"] == 0 and info_n["edges_linked"] == int(np.maximum(np.diff(srp) - 2, 0).sum())
    lab_h = host.connected_components((rp, ci))                       # numpy arrays: host pointers
    assert torch.equal(lab_h, lab)
    print(f"rmat{scale}: {k} components, {info} / symmetric {info_s}")


def test_upper_triangle_and_odd_patterns():
    import scipy.sparse as sp
    n = 30000
    rp, ci, _ = helpers.random_csr(n, n, 1.5 / n, 11)
    srp, sci = _symmetrised(rp, ci, n)
    S = sp.csr_matrix((np.ones(sci.size), sci, srp), shape=(n, n))
    U = sp.triu(S).tocsr()
    full, _, _ = _call(srp, sci, n, symmetric=True)
    upper, _, _ = _call(U.indptr, U.indices, n)
    want, _ = cref.labels(srp, sci, n)
    assert np.array_equal(full, want) and np.array_equal(upper, want)
    # self-loops, duplicates, unsorted rows, empty rows, isolated vertices
    rp2 = [0, 1, 1, 5, 5, 6, 6, 8, 8]
    ci2 = [0, 6, 4, 4, 2, 1, 7, 7]
    want2 = np.array([0, 1, 1, 3, 1, 5, 1, 1], np.int32)
    assert np.array_equal(cref.labels(rp2, ci2, 8)[0], want2)
    for device in (True, False):
        got, info, _ = _call(rp2, ci2, 8, device=device)
        assert np.array_equal(got, want2)
        _check_info(info, want2)
    # a stored entry is an edge whatever its value: the pattern is all the call sees
    got, info, _ = _call([0, 1, 2, 2], [1, 2], 3)
    assert got.tolist() == [0, 0, 0] and info["components"] == 1


def test_sizes_of_zero_and_one():
    from g4s_amd import host
    for device in (True, False):
        got, info, _ = _call([0], [], 0, device=device)
        assert got.size == 0 and info["components"] == 0 and info["largest"] == 0
        got, info, _ = _call([0, 0], [], 1, device=device)
        assert got.tolist() == [0] and (info["components"], info["largest"], info["largest_label"]) == (1, 1, 0)
        got, info, _ = _call([0, 1], [0], 1, device=device)
        assert got.tolist() == [0] and info["components"] == 1
        got, info, _ = _call(np.zeros(1001, np.int32), [], 1000, device=device)          # nnz == 0: labels[v] = v
        assert np.array_equal(got, np.arange(1000)) and (info["components"], info["largest"], info["largest_label"]) == (1000, 1, 0)
        assert info["edges_linked"] == 0
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
    lab = host.CSR(i32(1), i32(0), torch.zeros(0, dtype=torch.float64, device="cuda"), 0, 0).connected_components()
    assert lab.numel() == 0 and lab.dtype == torch.int32


def test_invalid_patterns_are_refused_on_the_device():
    from g4s_amd import capi
    n = 20000
    rp, ci, _ = helpers.random_csr(n, n, 3.0 / n, 5)
    want, _ = cref.labels(rp, ci, n)
    r = int(np.flatnonzero(np.diff(rp) >= 2)[7])
    bad = []
    c = ci.copy(); c[rp[r]] = n; bad.append((rp, c, "column id"))
    c = ci.copy(); c[rp[r] + 1] = -1; bad.append((rp, c, "column id"))
    p = rp.copy(); p[r] = p[r + 1] + 3; bad.append((p, ci, "rowptr"))                       # row r has a negative length
    p = rp.copy(); p[0] = 1; bad.append((p, ci, "rowptr"))                                  # does not start at 0
    for device in (True, False):
        for brp, bci, word in bad:
            _, _, st = _call(brp, bci, n, device=device, check=False)
            assert st == capi.ERR_INVALID, word
            assert word in capi.load().g4s_last_error().decode()
            got, info, _ = _call(rp, ci, n, device=device)           # and the next valid call succeeds
            assert np.array_equal(got, want)


def test_every_tuning_setting_gives_the_same_labels_and_info_repeats():
    from g4s_amd import host
    n = 1 << 16
    A = host.rmat_csr(n, 16, 8 * n, 7)
    rp, ci, _ = A.to_host()
    want, _ = cref.scipy_labels(rp, ci, n)
    srp, sci = _symmetrised(rp, ci, n)
    graphs = {"given": (A.rowptr, A.colids, False), "symmetric": (_dev(srp), _dev(sci), True)}
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for rounds in range(5):
            for no_skip in (0, 1):
                os.environ["G4S_CC_SAMPLE_ROUNDS"], os.environ["G4S_CC_NO_SKIP"] = str(rounds), str(no_skip)
                for name, (grp, gci, sym) in graphs.items():
                    got, info, _ = _call(grp, gci, n, symmetric=sym)
                    assert np.array_equal(got, want), (rounds, no_skip, name)
                    _check_info(info, want)
                    assert info["sample_rounds"] == rounds and info["skipped"] == int(sym and not no_skip)
                    again, info2, _ = _call(grp, gci, n, symmetric=sym, fill=n + 5)
                    assert np.array_equal(again, want) and info2 == info, (info, info2)
                    nnz = int(gci.numel())
                    deg = (grp[1:] - grp[:-1]).cpu().numpy()
                    if info["skipped"]:
                        assert info["edges_linked"] < nnz
                    else:
                        assert info["edges_linked"] == int(np.maximum(deg - rounds, 0).sum())
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n = 5000
    rp, ci, _ = helpers.random_csr(n, n, 2.0 / n, 9)
    rp_t, ci_t = _dev(rp), _dev(ci)
    lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    info = capi.CCInfo()
    info.components = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_connected_components(n, host._ptr(rp_t), host._ptr(ci_t), host._ptr(lab), capi.DEVICE_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.components == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(lab == -7)                                       # nothing was enqueued
    got, _, _ = _call(rp_t, ci_t, n)                                  # and the library still works
    assert np.array_equal(got, cref.labels(rp, ci, n)[0])


def test_min_plus_label_propagation_ends_at_the_same_labels():
    """The loop a caller could write before: l := l ⊕ (A ⊗ l) ⊕ (Aᵀ ⊗ l) over min-plus on a copy of the pattern with all values 0.0."""
    from g4s_amd import host
    n = 4000
    rp, ci, _ = helpers.random_csr(n, n, 1.2 / n, 21)
    Z = host.CSR.from_host(rp, ci, np.zeros(ci.size), n, n)
    l = torch.arange(n, dtype=torch.float64, device="cuda")
    rounds = 0
    while True:
        prev = l.clone()
        Z.spmv_semiring(prev, l, semiring="min_plus", accumulate=True)
        Z.spmv_semiring_transpose(prev, l, semiring="min_plus", accumulate=True)
        rounds += 1
        if torch.equal(l, prev):
            break
    fresh = host.CSR.from_host(rp, ci, np.ones(ci.size), n, n)        # its handle is never built
    lab = fresh.connected_components()
    assert fresh._handle is None
    assert torch.equal(lab, l.to(torch.int32)) and rounds > 3
    assert np.array_equal(lab.cpu().numpy(), cref.labels(rp, ci, n)[0])


CPP_CC = r"""
#include <cstdio>
#include <vector>
#include "g4s/csr.hpp"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    int n = 0, nnz = 0;
    if (!f || std::fscanf(f, "%d %d", &n, &nnz) != 2) return 2;
    std::vector<int32_t> rp(n + 1), ci(nnz);
    std::vector<double> va(nnz, 0.0);
    for (auto &v : rp) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : ci) if (std::fscanf(f, "%d", &v) != 1) return 2;
    std::fclose(f);
    g4s::CSR<int32_t, double> a(rp.data(), ci.data(), va.data(), n, n, nnz);
    std::vector<int32_t> lab(n, -7), lab2(n, -7);
    g4s_cc_info info;
    g4s::ConnectedComponents(a, lab.data(), false, &info);
    g4s::ConnectedComponents(a, lab2.data());
    if (lab != lab2) return 3;
    std::printf("%lld %lld %d %d\n", (long long)info.components, (long long)info.largest, info.largest_label, info.host_waits);
    for (int v : lab) std::printf("%d\n", v);
    g4s::CSR<int32_t, double> wide(rp.data(), ci.data(), va.data(), n, n + 1, nnz);
    try { g4s::ConnectedComponents(wide, lab.data()); return 4; } catch (const std::runtime_error &) {}
    g4s::CSR<int32_t, double> empty;
    g4s::ConnectedComponents(empty, nullptr);
    return 0;
}
"""


def test_cpp_header_form_runs(tmp_path):
    src, exe, inp = tmp_path / "cc.cpp", str(tmp_path / "cc"), tmp_path / "a.txt"
    src.write_text(CPP_CC)
    lib = os.path.join(ROOT, "g4s_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lg4s_hip", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    n = 3000
    rp, ci, _ = helpers.power_law_csr(n, n, 37, 600)
    inp.write_text(f"{n} {ci.size}\n" + "\n".join(map(str, rp)) + "\n" + "\n".join(map(str, ci)) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split()
    want, _ = cref.labels(rp, ci, n)
    comps, largest, label = cref.stats(want)
    assert [int(v) for v in lines[:4]] == [comps, largest, label, 1]
    assert np.array_equal(np.array(lines[4:4 + n], dtype=np.int32), want)
