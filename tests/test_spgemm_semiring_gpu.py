"""SpGEMM over the min-plus, max-plus and or-and semirings (include/g4s.h, G4S_SEMIRING_*) on every numeric path, both call forms.
The pattern must be the plus-times product's (checked against the oracle); the values must equal the numpy reference (tests/semiring_ref.py)
bit for bit — min, max and or do not depend on the order in which the products arrive."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import semiring_ref as ref
from tests.helpers import power_law_csr, random_csr
from tests.test_spgemm_gpu import _rank_cut_case, _shuffle_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("min_plus", "max_plus", "or_and")


def _run(A, B, M, K, N, semiring, two_phase):
    from g4s_amd import host
    a = host.CSR.from_host(*A, M, K)
    b = host.CSR.from_host(*B, K, N)
    return host.HashSpGEMM(a, b, two_phase=two_phase, semiring=semiring).to_host()


def _check(oracle, A, B, M, K, N, semiring, two_phase):
    crpt, ccol, cval = _run(A, B, M, K, N, semiring, two_phase)
    orpt, ocol, _ = oracle.spgemm(A, B, N, sort_output=True)
    assert np.array_equal(crpt, orpt), "row pointer differs from the plus-times pattern"
    assert np.array_equal(ccol, ocol), "column ids differ from the plus-times pattern"
    rrpt, rcol, rval = ref.spgemm(A, B, M, semiring)
    assert np.array_equal(rrpt, orpt) and np.array_equal(rcol, ocol)   # (the reference's own pattern)
    bad = np.flatnonzero((cval + 0.0) != (rval + 0.0))
    assert bad.size == 0, f"{bad.size} values differ, first at {bad[0]}: {cval[bad[0]]!r} vs {rval[bad[0]]!r}"
    return crpt, ccol, cval


def _with_zeros(A, seed, frac=0.2):
    """the same matrix with a fraction of its stored values set to 0.0 (structural zeros: or-and must keep the entries)"""
    rng = np.random.default_rng(seed)
    v = A[2].copy()
    v[rng.random(v.size) < frac] = 0.0
    return A[0], A[1], v


@pytest.fixture(params=["windows", "tables"])
def mid_row_kernels(request, monkeypatch):
    if request.param == "tables":
        monkeypatch.setenv("G4S_SPGEMM_WINDOW_MAX_N", "0")
    return request.param


def _all_row_classes_case():
    """the input of test_spgemm_all_row_classes: empty, tiny, small, medium, large, overflow → windows, window class and hub rows"""
    rng = np.random.default_rng(7)
    K, N = 3000, 60000
    bl = np.full(K, 100)
    bl[0] = 0
    brp = np.concatenate([[0], np.cumsum(bl)]).astype(np.int32)
    bci = np.concatenate([np.sort(rng.choice(N, l, replace=False)) for l in bl]).astype(np.int32)
    bva = rng.uniform(-1, 1, brp[-1])
    lens = [0, 1, 1, 4, 30, 120, 1000, 2900, 2999] + [2] * 50
    rows = [np.array([0]) if i == 1 else np.sort(rng.choice(np.arange(1, K), l, replace=False)) for i, l in enumerate(lens)]
    arp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    aci = np.concatenate(rows).astype(np.int32)
    ava = rng.uniform(-1, 1, arp[-1])
    return (arp, aci, ava), (brp, bci, bva), len(lens), K, N


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_all_row_classes(oracle, mid_row_kernels, semiring, two_phase):
    A, B, M, K, N = _all_row_classes_case()
    if semiring == "or_and":
        A, B = _with_zeros(A, 1), _with_zeros(B, 2)
    crpt, _, _ = _check(oracle, A, B, M, K, N, semiring, two_phase)
    nz = np.diff(crpt)
    assert nz[0] == 0 and nz[1] == 0 and nz[6] > 24576 and nz[5] > 4096


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_hub_path(oracle, semiring, two_phase):
    """one row of more than 2 M products: the HBM bitmap-rank path, global atomics"""
    rng = np.random.default_rng(11)
    K, N = 2000, 9000
    brp = (np.arange(K + 1) * 1100).astype(np.int32)
    bci = np.concatenate([np.sort(rng.choice(N, 1100, replace=False)) for _ in range(K)]).astype(np.int32)
    bva = rng.uniform(0, 1, brp[-1])
    arp = np.array([0, 1950, 1953, 1953], np.int32)
    aci = np.concatenate([np.sort(rng.choice(K, 1950, replace=False)), [3, 7, 9]]).astype(np.int32)
    ava = rng.uniform(-1, 1, arp[-1])
    A, B = (arp, aci, ava), (brp, bci, bva)
    if semiring == "or_and":
        A, B = _with_zeros(A, 3, 0.9), _with_zeros(B, 4, 0.9)      # most products false: entries with value 0.0 and with 1.0 in the hub row
    crpt, _, cval = _check(oracle, A, B, 3, K, N, semiring, two_phase)
    assert np.diff(crpt)[0] > 8000
    if semiring == "or_and":
        assert 0.0 in cval[:crpt[1]] and 1.0 in cval[:crpt[1]]


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("path", ["rank", "columns"])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_rank_kernel_cuts(oracle, monkeypatch, semiring, path, two_phase):
    if path == "columns":
        monkeypatch.setenv("G4S_SPGEMM_NO_RANK", "1")
    A, B, M, K, N = _rank_cut_case(1)
    rng = np.random.default_rng(5)
    A = (A[0], A[1], rng.uniform(-1, 1, A[2].size))               # signed values: the maxima and minima are not all at one end
    if semiring == "or_and":
        A, B = _with_zeros(A, 5), _with_zeros(B, 6)
    crpt, _, _ = _check(oracle, A, B, M, K, N, semiring, two_phase)
    assert list(np.diff(crpt)[:6]) == [8192, 8193, 12000, 20000, 8192 + 936 + 6000, 2000]


def _short_rows_case():
    rng = np.random.default_rng(71)
    M = K = N = 3000
    lens = rng.integers(0, 5, M)
    lens[[5, 900]] = [20, 100]
    arp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    aci = np.concatenate([np.sort(rng.choice(K, n, replace=False)) for n in lens]).astype(np.int32)
    blens = rng.integers(0, 5, K)
    brp = np.concatenate([[0], np.cumsum(blens)]).astype(np.int32)
    bci = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in blens]).astype(np.int32)
    return (arp, aci, rng.uniform(-1, 1, aci.size)), (brp, bci, rng.uniform(-1, 1, bci.size)), M, K, N


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("short_rows", ["wave", "tables"])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_short_rows_only(oracle, monkeypatch, semiring, short_rows, two_phase):
    """rows of at most 512 products: the wavefront merge (register combine in run order) or the hash-table kernels (G4S_SPGEMM_NO_WAVE_ROWS)"""
    if short_rows == "tables":
        monkeypatch.setenv("G4S_SPGEMM_NO_WAVE_ROWS", "1")
    A, B, M, K, N = _short_rows_case()
    if semiring == "or_and":
        A, B = _with_zeros(A, 7, 0.5), _with_zeros(B, 8, 0.5)
    _check(oracle, A, B, M, K, N, semiring, two_phase)


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("column_map", ["colmap", "plain"])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_column_map(oracle, monkeypatch, semiring, column_map, two_phase):
    """B with every other column empty: the window kernels run on renumbered columns, or on B's own ids with G4S_SPGEMM_NO_COLMAP"""
    if column_map == "plain":
        monkeypatch.setenv("G4S_SPGEMM_NO_COLMAP", "1")
    rp, ci, va = power_law_csr(6000, 6000, 29, 1500)
    B = (rp, (ci * 2).astype(np.int32), va)
    if semiring == "or_and":
        B = _with_zeros(B, 9)
    _check(oracle, (rp, ci, va), B, 6000, 6000, 12000, semiring, two_phase)


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_power_law_square(oracle, mid_row_kernels, semiring, two_phase):
    A = power_law_csr(6000, 6000, 23, 1500)
    if semiring == "or_and":
        A = _with_zeros(A, 10)
    _check(oracle, A, A, 6000, 6000, 6000, semiring, two_phase)


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_unsorted_b(oracle, semiring, two_phase):
    rp, ci, va = power_law_csr(6000, 6000, 23, 1500)
    B = _shuffle_rows(rp, ci, va, 11)
    if semiring == "or_and":
        B = _with_zeros(B, 11)
    _check(oracle, (rp, ci, va), B, 6000, 6000, 6000, semiring, two_phase)


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("semiring", NEW)
def test_semiring_repeated_columns_and_empty_rows(oracle, semiring, two_phase):
    """repeated columns inside rows of A and of B (combined like any other product), empty rows of A and B, an empty output row
    whose A row is not empty, and rows long enough for the table and window kernels"""
    rng = np.random.default_rng(13)
    M = K = N = 2500
    arp, aci, ava = random_csr(M, K, 0.004, 14, empty_rows=[0, 7, 100])
    brp, bci, bva = random_csr(K, N, 0.004, 15, empty_rows=[1, 2, 3])
    aci, bci = aci.copy(), bci.copy()
    for rp, ci in ((arp, aci), (brp, bci)):
        for r in rng.choice(np.flatnonzero(np.diff(rp) >= 2), 200, replace=False):
            ci[rp[r] + 1] = ci[rp[r]]                              # a repeated column (rows stay sorted: the copy sits next to its original)
    dense = random_csr(1, K, 0.6, 16)
    arp = np.concatenate([arp, [arp[-1] + dense[0][-1], arp[-1] + dense[0][-1] + 3]]).astype(np.int32)
    aci = np.concatenate([aci, dense[1], [1, 2, 3]]).astype(np.int32)   # a row of 1 500 entries, and a row that only meets empty B rows
    ava = np.concatenate([ava, dense[2], [0.5, 0.5, 0.5]])
    A, B = (arp, aci, ava), (brp, bci, bva)
    if semiring == "or_and":
        A, B = _with_zeros(A, 17), _with_zeros(B, 18)
    crpt, _, _ = _check(oracle, A, B, M + 2, K, N, semiring, two_phase)
    nz = np.diff(crpt)
    assert nz[0] == 0 and nz[-1] == 0 and nz[-2] > 2000


@pytest.mark.parametrize("semiring", NEW)
def test_semiring_rmat17(oracle, semiring):
    """a 2^17-row R-MAT A·A, one-call and two-call forms"""
    from g4s_amd import host
    n = 1 << 17
    A = host.rmat_csr(n, 17, 3 * n, 20240522)
    Ah = A.to_host()
    if semiring == "or_and":
        Ah = _with_zeros(Ah, 19)
        A = host.CSR.from_host(*Ah, n, n)
    orpt, ocol, _ = oracle.spgemm(Ah, Ah, n, sort_output=True)
    rrpt, rcol, rval = ref.spgemm(Ah, Ah, n, semiring)
    assert np.array_equal(rrpt, orpt) and np.array_equal(rcol, ocol)
    for two_phase in (False, True):
        crpt, ccol, cval = host.HashSpGEMM(A, A, two_phase=two_phase, semiring=semiring).to_host()
        assert np.array_equal(crpt, orpt) and np.array_equal(ccol, ocol)
        assert ref.same_values(cval, rval), two_phase


@pytest.mark.parametrize("two_phase", [False, True])
def test_min_plus_infinite_entries(oracle, two_phase):
    """+inf weights (no edge): an output whose products all involve +inf is +inf; one finite product is enough for a finite value"""
    A, B, M, K, N = _all_row_classes_case()
    rng = np.random.default_rng(21)
    ava, bva = A[2].copy(), B[2].copy()
    ava[rng.random(ava.size) < 0.3] = np.inf
    bva[rng.random(bva.size) < 0.3] = np.inf
    A, B = (A[0], A[1], ava), (B[0], B[1], bva)
    _, _, cval = _check(oracle, A, B, M, K, N, "min_plus", two_phase)
    assert np.isinf(cval).any() and np.isfinite(cval).any()
    _, _, cval = _check(oracle, (A[0], A[1], np.full(A[2].size, np.inf)), B, M, K, N, "min_plus", two_phase)
    assert np.all(cval == np.inf)


@pytest.mark.parametrize("two_phase", [False, True])
def test_or_and_keeps_structural_zeros(oracle, two_phase):
    """all-zero values: every entry of the pattern stays, with the value 0.0; NaN counts as true"""
    A, B, M, K, N = _all_row_classes_case()
    crpt, _, cval = _check(oracle, (A[0], A[1], np.zeros(A[2].size)), B, M, K, N, "or_and", two_phase)
    assert cval.size == crpt[-1] > 0 and np.all(cval == 0.0)
    ava = A[2].copy()
    ava[::2] = np.nan
    _, _, cval = _check(oracle, (A[0], A[1], ava), B, M, K, N, "or_and", two_phase)
    assert np.all((cval == 0.0) | (cval == 1.0))


def test_carried_state_switches_semirings(oracle):
    """symbolic once, then numeric plus-times → min-plus → max-plus → plus-times on the same arrays: the carried state is structural only.
    Integer values keep every plus-times sum exact, so the two plus-times results are bit-identical whatever the order of the atomics."""
    from g4s_amd import capi, host
    import ctypes as C
    lib = capi.load()
    rng = np.random.default_rng(31)
    rp, ci, _ = power_law_csr(6000, 6000, 23, 1500)
    va = rng.integers(-4, 5, ci.size).astype(np.float64)
    A = host.CSR.from_host(rp, ci, va, 6000, 6000)
    crpt = torch.empty(6001, dtype=torch.int32, device="cuda")
    cnnz = C.c_int64(0)
    p = host._ptr
    capi.check(lib.g4s_spgemm_symbolic(6000, 6000, 6000, p(A.rowptr), p(A.colids), p(A.rowptr), p(A.colids), p(crpt), C.byref(cnnz), host._stream()))
    orpt, ocol, oval = oracle.spgemm((rp, ci, va), (rp, ci, va), 6000, sort_output=True)
    assert np.array_equal(crpt.cpu().numpy(), orpt)
    results = []
    for name in ("plus_times", "min_plus", "max_plus", "plus_times"):
        ccol = torch.empty(cnnz.value, dtype=torch.int32, device="cuda")
        cval = torch.empty(cnnz.value, dtype=torch.float64, device="cuda")
        capi.check(lib.g4s_spgemm_numeric(6000, 6000, 6000, p(A.rowptr), p(A.colids), p(A.values), p(A.rowptr), p(A.colids), p(A.values), p(crpt), p(ccol),
                                          p(cval), capi.DEVICE_POINTERS | capi.SORT_OUTPUT | host.SEMIRINGS[name], host._stream()))
        torch.cuda.synchronize()
        want = oval if name == "plus_times" else ref.spgemm((rp, ci, va), (rp, ci, va), 6000, name)[2]
        assert np.array_equal(ccol.cpu().numpy(), ocol), name
        assert ref.same_values(cval.cpu().numpy(), want), name
        results.append(cval.cpu().numpy())
    assert np.array_equal(results[0].view(np.int64), results[3].view(np.int64))
    capi.check(lib.g4s_trim())


def test_explicit_plus_times_flag_is_the_default(oracle):
    """G4S_SEMIRING_PLUS_TIMES is 0: spelled out, it gives what flags without semiring bits give, through both entry points"""
    from g4s_amd import capi, host
    rng = np.random.default_rng(33)
    A, B, M, K, N = _all_row_classes_case()
    A = (A[0], A[1], rng.integers(-4, 5, A[2].size).astype(np.float64))
    B = (B[0], B[1], rng.integers(-4, 5, B[2].size).astype(np.float64))
    assert capi.SEMIRING_PLUS_TIMES == 0
    a, b = host.CSR.from_host(*A, M, K), host.CSR.from_host(*B, K, N)
    for two_phase in (False, True):
        c0 = host.HashSpGEMM(a, b, two_phase=two_phase)
        c1 = host.HashSpGEMM(a, b, two_phase=two_phase, semiring="plus_times")
        assert torch.equal(c0.rowptr, c1.rowptr) and torch.equal(c0.colids, c1.colids)
        assert torch.equal(c0.values.view(torch.int64), c1.values.view(torch.int64))
        _, _, oval = oracle.spgemm(A, B, N, sort_output=True)
        assert np.array_equal(c0.values.cpu().numpy(), oval)       # integer values: every order of summation is exact


# ------------------------------------------------------------------------------------------------ applications
def _clustered_graph(n=2000, size=25, seed=41):
    """a directed graph of integer weights 1 … 9: components of `size` vertices (about three edges per vertex), chained three by three with one edge
    each, so that its closure stays sparse"""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for c0 in range(0, n, size):
        m = min(size, n - c0)
        for v in range(m):
            for w in rng.choice(m, 3, replace=False):
                if w != v:
                    src.append(c0 + v)
                    dst.append(c0 + w)
        if (c0 // size) % 3 != 2 and c0 + size < n:
            src.append(c0 + int(rng.integers(m)))
            dst.append(c0 + size + int(rng.integers(min(size, n - c0 - size))))
    import scipy.sparse as sp
    G = sp.coo_matrix((rng.integers(1, 10, len(src)).astype(np.float64), (src, dst)), shape=(n, n)).tocsr()
    G.sum_duplicates()
    G.sort_indices()
    return G


def _with_diagonal(G, d):
    """G (no diagonal entries) with the diagonal stored explicitly as d: CSR arrays, rows sorted"""
    n = G.shape[0]
    Gc = G.tocoo()
    r = np.concatenate([Gc.row, np.arange(n)])
    c = np.concatenate([Gc.col, np.arange(n)])
    v = np.concatenate([Gc.data, np.full(n, d)])
    order = np.lexsort((c, r))
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return rp, c[order].astype(np.int32), v[order]


def _square_to_fixed_point(D, n, semiring):
    from g4s_amd import host
    for _ in range(20):
        c = host.HashSpGEMM(D, D, semiring=semiring)
        if torch.equal(c.rowptr, D.rowptr) and torch.equal(c.colids, D.colids) and torch.equal(c.values, D.values):
            return c
        D = c
    raise AssertionError("no fixed point after 20 squarings")


def test_min_plus_all_pairs_shortest_paths():
    """D ← D ⊗ D over (min, +) from A with a zero diagonal, until nothing changes: every finite entry of scipy's shortest_path, exactly"""
    from scipy.sparse import csgraph
    from g4s_amd import host
    n = 2000
    G = _clustered_graph(n)
    rp, ci, va = _with_diagonal(G, 0.0)
    D = _square_to_fixed_point(host.CSR.from_host(rp, ci, va, n, n), n, "min_plus")
    crpt, ccol, cval = D.to_host()
    want = csgraph.shortest_path(G, method="D", directed=True)
    fin = np.isfinite(want)
    assert np.array_equal(np.diff(crpt), fin.sum(axis=1))
    dense = np.full((n, n), np.inf)
    dense[np.repeat(np.arange(n), np.diff(crpt)), ccol] = cval
    assert np.array_equal(dense, want)


def test_or_and_transitive_closure():
    """R ← R ⊗ R over (or, and) from A ∪ I: the reflexive-transitive closure, equal to breadth-first reachability from every vertex"""
    from scipy.sparse import csgraph
    from g4s_amd import host
    n = 2000
    G = _clustered_graph(n, seed=43)
    rp, ci, _ = _with_diagonal(G, 1.0)
    R = _square_to_fixed_point(host.CSR.from_host(rp, ci, np.ones(ci.size), n, n), n, "or_and")
    crpt, ccol, cval = R.to_host()
    assert np.all(cval == 1.0)
    for i in range(n):
        reach = np.sort(csgraph.breadth_first_order(G, i, directed=True, return_predecessors=False))
        assert np.array_equal(ccol[crpt[i]:crpt[i + 1]], reach), i


# ------------------------------------------------------------------------------------------------ the C++ header
CPP_MIN_PLUS = r"""
#include <cstdio>
#include <vector>
#include "g4s/csr.hpp"
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[1], "r");
    int n = 0, nnz = 0;
    if (std::fscanf(f, "%d %d", &n, &nnz) != 2) return 2;
    std::vector<int> rp(n + 1), ci(nnz);
    std::vector<double> va(nnz);
    for (auto &x : rp) if (std::fscanf(f, "%d", &x) != 1) return 2;
    for (int k = 0; k < nnz; ++k) if (std::fscanf(f, "%d %lf", &ci[k], &va[k]) != 2) return 2;
    std::fclose(f);
    g4s::CSR<int32_t, double> a(rp.data(), ci.data(), va.data(), n, n, nnz), c;
    g4s::HashSpGEMM(a, a, c, std::plus<double>(), g4s::min_op<double>());
    std::printf("%d %d\n", c.rows, c.nnz);
    for (int i = 0; i <= c.rows; ++i) std::printf("%d\n", c.rowptr[i]);
    for (int k = 0; k < c.nnz; ++k) std::printf("%d %.17g\n", c.colids[k], c.values[k]);
    return 0;
}
"""


def test_cpp_header_min_plus_runs(tmp_path):
    """g4s::HashSpGEMM with (std::plus, g4s::min_op) through include/g4s/csr.hpp on host arrays, against the numpy reference"""
    src, exe, inp = tmp_path / "minplus.cpp", str(tmp_path / "minplus"), tmp_path / "a.txt"
    src.write_text(CPP_MIN_PLUS)
    lib = os.path.join(ROOT, "g4s_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lg4s_hip", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    rp, ci, va = power_law_csr(3000, 3000, 37, 600)
    inp.write_text(f"{3000} {ci.size}\n" + "\n".join(map(str, rp)) + "\n" + "\n".join(f"{c} {float(v)!r}" for c, v in zip(ci, va)) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rows, nnz = map(int, lines[0].split())
    crpt = np.array(lines[1:rows + 2], dtype=np.int64)
    ent = [l.split() for l in lines[rows + 2:rows + 2 + nnz]]
    ccol, cval = np.array([int(c) for c, _ in ent]), np.array([float(v) for _, v in ent])
    rrpt, rcol, rval = ref.spgemm((rp, ci, va), (rp, ci, va), 3000, "min_plus")
    assert np.array_equal(crpt, rrpt) and np.array_equal(ccol, rcol) and ref.same_values(cval, rval)
