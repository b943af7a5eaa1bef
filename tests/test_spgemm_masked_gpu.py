"""g4s_spgemm_masked (C⟨M⟩ = A ⊗ B at the positions of a pattern M) and g4s_triangle_count on the device, against tests/masked_ref.py.
Values are compared as the semiring tests do: min-plus, max-plus and or-and bit for bit (semiring_ref.same_values); plus-times bit for bit on
integer-valued and pattern-only inputs, and within 1e-10·Σ|a·b| per entry on real values (the Σ computed by the reference). Every row class —
wave, LDS, global, split — is reached by at least one test, shown by g4s_masked_info; the inputs here are statistical. Rows AT and just past every
limit between the seven classes (and the counts of each class, which g4s_masked_info merges) are pinned by tests/test_spgemm_masked_limits_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import masked_ref as mref
from tests import semiring_ref as ref
from tests.helpers import power_law_csr, random_csr
from tests.test_spgemm_gpu import _shuffle_rows
from tests.test_spgemm_semiring_gpu import _all_row_classes_case, _with_zeros

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ref.NAMES


def _ints(A, seed):
    """the same pattern with integer values in −4 … 4: every plus-times partial sum is exact"""
    return A[0], A[1], np.random.default_rng(seed).integers(-4, 5, len(A[1])).astype(np.float64)


def _run(A, B, M, K, N, mask, semiring, pattern_only=False):
    from g4s_amd import host
    a, b = host.CSR.from_host(*A, M, K), host.CSR.from_host(*B, K, N)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    c, info = host.spgemm_masked(a, b, (t(mask[0]), t(mask[1])), semiring=semiring, pattern_only=pattern_only, return_info=True)
    assert info["mask_nnz"] == len(mask[1])
    return c.values.cpu().numpy(), info


def _run_host_pointers(A, B, M, K, N, mask, semiring, pattern_only=False):
    from g4s_amd import capi, host
    arrs = [np.ascontiguousarray(x, dt) for x, dt in ((A[0], np.int32), (A[1], np.int32), (A[2], np.float64), (B[0], np.int32), (B[1], np.int32),
                                                      (B[2], np.float64), (mask[0], np.int32), (mask[1], np.int32))]
    cval = np.full(max(len(mask[1]), 1), 123.0)
    P = lambda a: C.c_void_p(a.ctypes.data)
    null = C.c_void_p(0)
    info = capi.MaskedInfo()
    capi.check(capi.load().g4s_spgemm_masked(M, K, N, P(arrs[0]), P(arrs[1]), null if pattern_only else P(arrs[2]), P(arrs[3]), P(arrs[4]),
                                             null if pattern_only else P(arrs[5]), P(arrs[6]), P(arrs[7]), P(cval), capi.HOST_POINTERS | host.SEMIRINGS[semiring],
                                             C.byref(info), None))
    return cval[:len(mask[1])], info


def _compare(got, A, B, M, N, mask, semiring, pattern_only=False, exact=False):
    want, hit = mref.spgemm_masked(A, B, M, N, mask, semiring, pattern_only)
    assert got.shape == want.shape
    if semiring != "plus_times":
        bad = np.flatnonzero((got + 0.0) != (want + 0.0))
        assert bad.size == 0, f"{semiring}: {bad.size} values differ, first at {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"
    elif exact or pattern_only:
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"plus_times: {bad.size} values differ, first at {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"
    else:
        scale = mref.abs_sums(A, B, M, N, mask)
        err = np.abs(got - want)
        print(f"plus_times: max |err| {err.max():.3e}, max err / (1e-10·Σ|a·b|) {np.max(err / np.maximum(1e-10 * scale, 1e-300)):.3e}")
        assert np.all(err <= 1e-10 * scale)
    return want, hit


def _check(A, B, M, K, N, mask, semiring, pattern_only=False, exact=False):
    got, info = _run(A, B, M, K, N, mask, semiring, pattern_only)
    want, hit = _compare(got, A, B, M, N, mask, semiring, pattern_only, exact)
    return got, hit, info


def _prepare(A, B, semiring, seeds=(1, 2), frac=0.2):
    """or-and gets stored zeros (entries that exist with the value 0.0), as in the semiring tests"""
    if semiring == "or_and":
        return _with_zeros(A, seeds[0], frac), _with_zeros(B, seeds[1], frac)
    return A, B


def _product_pattern(A, B, M):
    crpt, ccol, _ = ref.spgemm((A[0], A[1], np.ones(len(A[1]))), (B[0], B[1], np.ones(len(B[1]))), M, "plus_times")
    return crpt, ccol


def _sample_and_extend(pattern, N, seed, keep=0.3, extra=0.15):
    """a seeded sample of `pattern`'s entries merged with random columns (most of which receive no product): strictly ascending rows"""
    rng = np.random.default_rng(seed)
    crpt, ccol = pattern
    rows, lens = [], []
    for i in range(len(crpt) - 1):
        c = ccol[crpt[i]:crpt[i + 1]]
        kept = c[rng.random(c.size) < keep]
        add = rng.integers(0, N, int(extra * c.size) + 2)
        r = np.unique(np.concatenate([kept, add]))
        rows.append(r)
        lens.append(r.size)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate(rows).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1: mask = A, both pointer forms
@pytest.mark.parametrize("semiring", ALL)
def test_mask_is_a_power_law_square_device_and_host_forms(semiring):
    n = 6000
    A = _ints(power_law_csr(n, n, 23, 1500), 5)
    A, _ = _prepare(A, A, semiring)
    mask = (A[0], A[1])
    got, hit, info = _check(A, A, n, n, n, mask, semiring, exact=True)
    assert got.size == 207804 and 0 < hit.sum() < got.size
    assert info["products"] > 0 and info["rows_wave"] > 0 and info["rows_lds"] > 0
    got_h, info_h = _run_host_pointers(A, A, n, n, n, mask, semiring)
    assert np.array_equal(got.view(np.int64), got_h.view(np.int64))
    assert {k: info[k] for k in info} == {n_: getattr(info_h, n_) for n_ in info}


def test_real_valued_plus_times_is_within_the_atomic_bound():
    n = 6000
    A = power_law_csr(n, n, 23, 1500)
    _check(A, A, n, n, n, (A[0], A[1]), "plus_times")


# ------------------------------------------------------------------------------------------------ 2: every row class of the SpGEMM tests
@pytest.mark.parametrize("semiring", ALL)
def test_all_row_classes_full_pattern_equals_hash_spgemm(semiring):
    """mask = the pattern of the full product: the values must be those of host.HashSpGEMM of the same inputs (integer values for plus-times, so that
    both sums are exact)"""
    from g4s_amd import host
    A, B, M, K, N = _all_row_classes_case()
    if semiring == "plus_times":
        A, B = _ints(A, 3), _ints(B, 4)
    A, B = _prepare(A, B, semiring)
    a, b = host.CSR.from_host(*A, M, K), host.CSR.from_host(*B, K, N)
    full = host.HashSpGEMM(a, b, semiring=semiring)
    c, info = host.spgemm_masked(a, b, full, semiring=semiring, return_info=True)
    assert c.rowptr.data_ptr() == full.rowptr.data_ptr() and c.colids.data_ptr() == full.colids.data_ptr()   # the pattern is shared, not copied
    assert c.values.data_ptr() != full.values.data_ptr()
    want, got = full.values.cpu().numpy(), c.values.cpu().numpy()
    assert ref.same_values(got, want)
    assert info["mask_nnz"] == full.nnz and info["rows_lds"] >= 1 and info["rows_global"] >= 1 and info["rows_split"] == 0
    _compare(got, A, B, M, N, (full.rowptr.cpu().numpy(), full.colids.cpu().numpy()), semiring, exact=True)


@pytest.mark.parametrize("semiring", ALL)
def test_all_row_classes_sampled_mask(semiring):
    """a 30 % sample of the product's pattern merged with columns that receive no product: hits and identities in every row"""
    A, B, M, K, N = _all_row_classes_case()
    A, B = _prepare(A, B, semiring)
    mask = _sample_and_extend(_product_pattern(A, B, M), N, 17)
    got, hit, info = _check(A, B, M, K, N, mask, semiring)
    assert hit.any() and not hit.all()
    assert np.all(got[~hit] == mref.IDENTITY[semiring])
    assert info["rows_wave"] >= 1 and info["rows_lds"] >= 1, info       # the wave and the LDS classes both ran


@pytest.mark.parametrize("semiring", ALL)
def test_mask_rows_where_the_product_has_none(semiring):
    """mask rows empty where A's row is not, and non-empty where A's row is empty or meets only empty rows of B: all identity"""
    A, B, M, K, N = _all_row_classes_case()
    A, B = _prepare(A, B, semiring)
    rng = np.random.default_rng(19)
    pattern = _product_pattern(A, B, M)
    mrpt, mcol = _sample_and_extend(pattern, N, 23)
    rows = [mcol[mrpt[i]:mrpt[i + 1]] for i in range(M)]
    rows[0] = np.unique(rng.integers(0, N, 50))                        # A's row 0 is empty
    rows[1] = np.unique(rng.integers(0, N, 700))                       # A's row 1 meets the empty row 0 of B
    for i in (3, 6, 10, 11):
        rows[i] = np.zeros(0, np.int32)                                # rows of A with products, nothing asked for
    mask = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), np.concatenate(rows).astype(np.int32))
    got, hit, info = _check(A, B, M, K, N, mask, semiring)
    assert np.all(got[:mask[0][2]] == mref.IDENTITY[semiring]) and not hit[:mask[0][2]].any()
    assert info["products"] < mref.mask_rows(A[0]).size * 100


# ------------------------------------------------------------------------------------------------ 3: a mask row longer than the LDS table
@pytest.mark.parametrize("semiring", ALL)
def test_full_mask_row_takes_the_global_class(semiring):
    A, B, M, K, N = _all_row_classes_case()
    A, B = _prepare(A, B, semiring)
    mrpt, mcol = _sample_and_extend(_product_pattern(A, B, M), N, 29)
    rows = [mcol[mrpt[i]:mrpt[i + 1]] for i in range(M)]
    rows[7] = np.arange(N, dtype=np.int32)                             # every column of the 2 900-entry row
    rows[4] = np.arange(N, dtype=np.int32)[::2]
    mask = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), np.concatenate(rows).astype(np.int32))
    got, hit, info = _check(A, B, M, K, N, mask, semiring)
    assert info["rows_global"] >= 2, info


# ------------------------------------------------------------------------------------------------ 4: a hub row is split
def _hub_case():
    """the input of test_semiring_hub_path: one row of more than 2 M products"""
    rng = np.random.default_rng(11)
    K, N = 2000, 9000
    brp = (np.arange(K + 1) * 1100).astype(np.int32)
    bci = np.concatenate([np.sort(rng.choice(N, 1100, replace=False)) for _ in range(K)]).astype(np.int32)
    bva = rng.uniform(0, 1, brp[-1])
    arp = np.array([0, 1950, 1953, 1953], np.int32)
    aci = np.concatenate([np.sort(rng.choice(K, 1950, replace=False)), [3, 7, 9]]).astype(np.int32)
    ava = rng.uniform(-1, 1, arp[-1])
    return (arp, aci, ava), (brp, bci, bva), 3, K, N


@pytest.mark.parametrize("mask_row", ["short", "long"])
@pytest.mark.parametrize("semiring", ALL)
def test_hub_row_is_split(semiring, mask_row):
    A, B, M, K, N = _hub_case()
    if semiring == "or_and":
        A, B = _with_zeros(A, 3, 0.9), _with_zeros(B, 4, 0.9)
    rng = np.random.default_rng(31)
    hub = np.unique(rng.integers(0, N, 40)).astype(np.int32) if mask_row == "short" else np.arange(N, dtype=np.int32)
    rows = [hub, np.unique(rng.integers(0, N, 3000)).astype(np.int32), np.unique(rng.integers(0, N, 10)).astype(np.int32)]
    mask = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), np.concatenate(rows))
    got, hit, info = _check(A, B, M, K, N, mask, semiring)
    assert info["rows_split"] >= 1, info
    assert (info["rows_lds"] >= 2) if mask_row == "short" else (info["rows_global"] >= 1), info
    assert hit[:len(hub)].all()                                        # 1 950 rows of 1 100 of 9 000 columns: every column is reached
    if semiring == "or_and":
        assert 0.0 in got[:len(hub)] or mask_row == "short"


# ------------------------------------------------------------------------------------------------ 5: repeated columns, unsorted A and B, empty rows
def _repeated_columns_case():
    """the construction of test_semiring_repeated_columns_and_empty_rows"""
    rng = np.random.default_rng(13)
    M = K = N = 2500
    arp, aci, ava = random_csr(M, K, 0.004, 14, empty_rows=[0, 7, 100])
    brp, bci, bva = random_csr(K, N, 0.004, 15, empty_rows=[1, 2, 3])
    aci, bci = aci.copy(), bci.copy()
    for rp, ci in ((arp, aci), (brp, bci)):
        for r in rng.choice(np.flatnonzero(np.diff(rp) >= 2), 200, replace=False):
            ci[rp[r] + 1] = ci[rp[r]]
    dense = random_csr(1, K, 0.6, 16)
    arp = np.concatenate([arp, [arp[-1] + dense[0][-1], arp[-1] + dense[0][-1] + 3]]).astype(np.int32)
    aci = np.concatenate([aci, dense[1], [1, 2, 3]]).astype(np.int32)
    ava = np.concatenate([ava, dense[2], [0.5, 0.5, 0.5]])
    return (arp, aci, ava), (brp, bci, bva), M + 2, K, N


@pytest.mark.parametrize("order", ["sorted", "unsorted_b", "unsorted_a", "unsorted_both"])
@pytest.mark.parametrize("semiring", ALL)
def test_repeated_columns_unsorted_rows_and_empty_rows(semiring, order):
    A, B, M, K, N = _repeated_columns_case()
    A, B = _prepare(A, B, semiring, (17, 18))
    mask = _sample_and_extend(_product_pattern(A, B, M), N, 37, keep=0.5)
    if order in ("unsorted_a", "unsorted_both"):
        A = _shuffle_rows(*A, 41)
    if order in ("unsorted_b", "unsorted_both"):
        B = _shuffle_rows(*B, 43)
    got, hit, info = _check(A, B, M, K, N, mask, semiring)
    assert hit.any() and not hit.all()


# ------------------------------------------------------------------------------------------------ 6: the mask aliases A's arrays
@pytest.mark.parametrize("semiring", ALL)
def test_mask_and_b_alias_the_arrays_of_a(semiring):
    from g4s_amd import host
    n = 6000
    A = _ints(power_law_csr(n, n, 29, 1500), 7)
    a = host.CSR.from_host(*A, n, n)
    c = host.spgemm_masked(a, a, a, semiring=semiring)
    assert c.rowptr.data_ptr() == a.rowptr.data_ptr() and c.colids.data_ptr() == a.colids.data_ptr()
    _compare(c.values.cpu().numpy(), A, A, n, n, (A[0], A[1]), semiring, exact=True)
    c2 = host.spgemm_masked(a, a, (a.rowptr, a.colids), semiring=semiring)
    assert torch.equal(c.values.view(torch.int64), c2.values.view(torch.int64))
    assert np.array_equal(a.values.cpu().numpy(), A[2])                # the inputs are untouched


# ------------------------------------------------------------------------------------------------ 7: invalid masks
def test_invalid_masks_are_refused_and_the_next_call_works():
    from g4s_amd import capi, host
    n = 3000
    A = power_law_csr(n, n, 37, 600)
    a = host.CSR.from_host(*A, n, n)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    long_rows = np.flatnonzero(np.diff(A[0]) >= 3)
    r = int(long_rows[len(long_rows) // 2])
    k = int(A[0][r])

    def swapped():
        c = A[1].copy()
        c[k], c[k + 1] = c[k + 1], c[k]
        return A[0], c

    def repeated():
        c = A[1].copy()
        c[k + 1] = c[k]
        return A[0], c

    def too_large():
        c = A[1].copy()
        c[int(A[0][r + 1]) - 1] = n
        return A[0], c

    def decreasing():
        p = A[0].copy()
        p[r + 1] = p[r] - 1
        return p, A[1]

    def negative():
        c = A[1].copy()
        c[k] = -1
        return A[0], c

    for make in (swapped, repeated, too_large, decreasing, negative):
        mrp, mci = make()
        with pytest.raises(capi.G4SError) as e:
            host.spgemm_masked(a, a, (t(mrp), t(mci)))
        assert e.value.status == capi.ERR_INVALID, make.__name__
        assert "mask" in str(e.value)
        c = host.spgemm_masked(a, a, a, semiring="min_plus")           # a valid call afterwards still succeeds
        _compare(c.values.cpu().numpy(), A, A, n, n, (A[0], A[1]), "min_plus")
    bad = A[1].copy()                                                  # A and B are range-checked too
    bad[5] = n + 7
    with pytest.raises(capi.G4SError) as e:
        host.spgemm_masked(host.CSR.from_host(A[0], bad, A[2], n, n), a, a)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.G4SError) as e:
        host.spgemm_masked(a, host.CSR.from_host(A[0], bad, A[2], n, n), a)
    assert e.value.status == capi.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 8: pattern-only
@pytest.mark.parametrize("case", ["power_law", "row_classes"])
def test_pattern_only_counts_and_hits(case):
    if case == "power_law":
        n = 6000
        A = power_law_csr(n, n, 23, 1500)
        B, M, K, N = A, n, n, n
        mask = (A[0], A[1])
    else:
        A, B, M, K, N = _all_row_classes_case()
        mask = _sample_and_extend(_product_pattern(A, B, M), N, 47)
    ones = lambda X: (X[0], X[1], np.ones(len(X[1])))
    cnt, hit, info = _check(A, B, M, K, N, mask, "plus_times", pattern_only=True)
    want, _ = mref.spgemm_masked(ones(A), ones(B), M, N, mask, "plus_times")
    assert np.array_equal(cnt, want) and np.array_equal(cnt > 0, hit) and cnt.max() > 1
    marks, _, _ = _check(A, B, M, K, N, mask, "or_and", pattern_only=True)
    assert np.array_equal(marks, hit.astype(np.float64))
    for name in ("min_plus", "max_plus"):
        v, _, _ = _check(A, B, M, K, N, mask, name, pattern_only=True)
        assert np.all(v[hit] == 2.0)
    cnt_h, _ = _run_host_pointers(A, B, M, K, N, mask, "plus_times", pattern_only=True)
    assert np.array_equal(cnt_h, cnt)
    # stored zeros do not matter to the pattern-only product
    z, _, _ = _check(_with_zeros(A, 1, 0.5), _with_zeros(B, 2, 0.5), M, K, N, mask, "or_and", pattern_only=True)
    assert np.array_equal(z, marks)


# ------------------------------------------------------------------------------------------------ 9: +inf entries
def test_min_plus_infinite_entries():
    A, B, M, K, N = _all_row_classes_case()
    rng = np.random.default_rng(21)
    ava, bva = A[2].copy(), B[2].copy()
    ava[rng.random(ava.size) < 0.3] = np.inf
    bva[rng.random(bva.size) < 0.3] = np.inf
    A, B = (A[0], A[1], ava), (B[0], B[1], bva)
    mask = _sample_and_extend(_product_pattern(A, B, M), N, 53)
    got, hit, _ = _check(A, B, M, K, N, mask, "min_plus")
    assert np.isinf(got[hit]).any() and np.isfinite(got[hit]).any()
    got, _, _ = _check((A[0], A[1], np.full(A[2].size, np.inf)), B, M, K, N, mask, "min_plus")
    assert np.all(got == np.inf)


# ------------------------------------------------------------------------------------------------ 10: R-MAT scale 17
@pytest.mark.parametrize("semiring", ALL)
def test_rmat17_mask_is_a(semiring):
    from g4s_amd import host
    n = 1 << 17
    A = host.rmat_csr(n, 17, 3 * n, 20240522)
    Ah = A.to_host()
    if semiring == "or_and":
        Ah = _with_zeros(Ah, 19)
        A = host.CSR.from_host(*Ah, n, n)
    c, info = host.spgemm_masked(A, A, A, semiring=semiring, return_info=True)
    want, hit = _compare(c.values.cpu().numpy(), Ah, Ah, n, n, (Ah[0], Ah[1]), semiring)
    assert hit.any() and not hit.all()
    assert info["rows_wave"] > 0 and info["rows_lds"] > 0
    print(f"rmat17 {semiring}: {info}")


# ------------------------------------------------------------------------------------------------ 11: capture, sizes of 0
def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n = 2000
    A = power_law_csr(n, n, 3, 300)
    a = host.CSR.from_host(*A, n, n)
    cval = torch.full((a.nnz,), 5.0, dtype=torch.float64, device="cuda")
    count = C.c_int64(-3)
    p = host._ptr
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_spgemm_masked(n, n, n, p(a.rowptr), p(a.colids), p(a.values), p(a.rowptr), p(a.colids), p(a.values), p(a.rowptr), p(a.colids), p(cval),
                                   capi.DEVICE_POINTERS, None, C.c_void_p(stream.cuda_stream))
        st2 = lib.g4s_triangle_count(n, p(a.rowptr), p(a.colids), C.byref(count), capi.DEVICE_POINTERS, None, C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and st2 == capi.ERR_INVALID and count.value == -3
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(cval == 5.0)                                      # nothing was enqueued
    c = host.spgemm_masked(a, a, a)                                    # and the library still works
    _compare(c.values.cpu().numpy(), A, A, n, n, (A[0], A[1]), "plus_times")


@pytest.mark.parametrize("semiring", ALL)
def test_sizes_of_zero(semiring):
    from g4s_amd import host
    n = 500
    A = power_law_csr(n, n, 9, 100)
    a = host.CSR.from_host(*A, n, n)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
    ident = mref.IDENTITY[semiring]
    empty = host.CSR(i32(n + 1), i32(0), f64(0), n, n)
    c, info = host.spgemm_masked(empty, a, a, semiring=semiring, return_info=True)          # nnz(A) == 0
    assert torch.all(c.values == ident) and c.nnz == a.nnz and info["products"] == 0
    c = host.spgemm_masked(a, empty, a, semiring=semiring)                                  # nnz(B) == 0
    assert torch.all(c.values == ident)
    c, info = host.spgemm_masked(a, a, empty, semiring=semiring, return_info=True)          # nnz(M) == 0
    assert c.nnz == 0 and c.values.numel() == 0 and info["mask_nnz"] == 0
    none = host.CSR(i32(1), i32(0), f64(0), 0, n)                                           # M == 0
    c = host.spgemm_masked(none, a, none, semiring=semiring)
    assert c.rows == 0 and c.nnz == 0
    k0a, k0b = host.CSR(i32(n + 1), i32(0), f64(0), n, 0), host.CSR(i32(1), i32(0), f64(0), 0, n)   # K == 0
    c = host.spgemm_masked(k0a, k0b, a, semiring=semiring)
    assert torch.all(c.values == ident)
    n0 = host.CSR(i32(n + 1), i32(0), f64(0), n, 0)                                         # N == 0: B and the mask have no columns
    c = host.spgemm_masked(a, n0, n0, semiring=semiring)
    assert c.nnz == 0


# ------------------------------------------------------------------------------------------------ 12: triangles
def _csr_of(G):
    G = G.tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int32), G.indices.astype(np.int32), np.ones(G.nnz)


def _count(G, n, return_info=False):
    from g4s_amd import host
    return host.CSR.from_host(*_csr_of(G), n, n).triangle_count(return_info=return_info)


def test_triangles_of_a_power_law_graph_in_every_presentation():
    import scipy.sparse as sp
    from g4s_amd import capi, host
    n = 4000
    rp, ci, _ = power_law_csr(n, n, 31, 800)
    G = mref.symmetric_simple_graph(rp, ci, n)
    assert G.nnz == 2 * 100398 and mref.triangles_trace(G) == mref.triangles_lower(G) == 298117
    count, info = _count(G, n, return_info=True)
    assert count == 298117
    L = sp.tril(G, k=-1)
    assert info["mask_nnz"] == L.nnz == 100398
    assert info["products"] == int((L @ (L @ np.ones(n))).sum())       # Σ_i Σ_{p ∈ L(i,:)} nnz(L(p,:))
    assert _count(L, n) == 298117                                      # the lower triangle alone
    assert _count(G + sp.identity(n), n) == 298117                     # with self-loops
    assert _count(L + sp.identity(n), n) == 298117
    rev = n - 1 - np.arange(n)                                         # vertex ids reversed: another orientation of every triangle
    Gc = G.tocoo()
    assert _count(sp.coo_matrix((Gc.data, (rev[Gc.row], rev[Gc.col])), shape=(n, n)), n) == 298117
    # host pointers, and the functional form
    g = _csr_of(G)
    cnt = C.c_int64(0)
    capi.check(capi.load().g4s_triangle_count(n, C.c_void_p(g[0].ctypes.data), C.c_void_p(g[1].ctypes.data), C.byref(cnt), capi.HOST_POINTERS, None, None))
    assert cnt.value == 298117
    assert host.triangle_count(host.CSR.from_host(*g, n, n)) == 298117
    # per-edge counts are one masked call on L away: their sum is the count
    l = host.CSR.from_host(*_csr_of(L), n, n)
    per_edge = host.spgemm_masked(l, l, l, pattern_only=True)
    assert int(per_edge.values.sum().item()) == 298117


def test_triangles_of_a_grid_a_clique_and_an_empty_graph():
    import scipy.sparse as sp
    from g4s_amd import host
    side = 300
    idx = np.arange(side * side).reshape(side, side)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    grid = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(side * side, side * side))
    assert _count(grid + grid.T, side * side) == 0
    k = 300
    count, info = _count(sp.csr_matrix(np.ones((k, k)) - np.eye(k)), k, return_info=True)
    assert count == 4455100 == k * (k - 1) * (k - 2) // 6
    assert info["rows_lds"] > 0
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
    assert host.CSR(i32(11), i32(0), torch.zeros(0, dtype=torch.float64, device="cuda"), 10, 10).triangle_count() == 0
    assert _count(sp.identity(50), 50) == 0                            # self-loops only: L is empty


def test_triangles_rmat17_equal_scipy():
    from g4s_amd import host
    n = 1 << 17
    A = host.rmat_csr(n, 17, 3 * n, 20240522)
    rp, ci, _ = A.to_host()
    G = mref.symmetric_simple_graph(rp, ci, n)
    want = mref.triangles_lower(G)
    count, info = _count(G, n, return_info=True)
    print(f"rmat17 symmetrised: {G.nnz // 2} edges, {want} triangles, info {info}")
    assert count == want and want > 0


def test_triangles_refuse_unsorted_rows():
    from g4s_amd import capi, host
    n = 4000
    rp, ci, _ = power_law_csr(n, n, 31, 800)
    g = _csr_of(mref.symmetric_simple_graph(rp, ci, n))
    r = int(np.flatnonzero(np.diff(g[0]) >= 3)[5])
    for kind in ("swapped", "repeated", "range"):
        c = g[1].copy()
        k = int(g[0][r])
        if kind == "swapped":
            c[k], c[k + 1] = c[k + 1], c[k]
        elif kind == "repeated":
            c[k + 1] = c[k]
        else:
            c[int(g[0][r + 1]) - 1] = n
        with pytest.raises(capi.G4SError) as e:
            host.CSR.from_host(g[0], c, g[2], n, n).triangle_count()
        assert e.value.status == capi.ERR_INVALID, kind
    assert host.CSR.from_host(*g, n, n).triangle_count() == 298117


# ------------------------------------------------------------------------------------------------ class boundaries moved by the environment
@pytest.mark.parametrize("switch", [("G4S_MASKED_WAVE_FLOP", "0"), ("G4S_MASKED_LDS_LARGE", "0"), ("G4S_MASKED_LDS_SMALL", "0"), ("G4S_MASKED_SPLIT_FLOP", "20000"),
                                    ("G4S_MASKED_SPLIT_WAYS", "3")])
def test_forced_class_cuts_give_the_same_values(monkeypatch, switch):
    """every class against another: the same inputs with a boundary moved must give the same bits (integer values), and info must show the move"""
    A, B, M, K, N = _all_row_classes_case()
    A, B = _ints(A, 3), _ints(B, 4)
    mask = _sample_and_extend(_product_pattern(A, B, M), N, 17)
    base, _, info0 = _check(A, B, M, K, N, mask, "plus_times", exact=True)
    monkeypatch.setenv(*switch)
    if switch[0] == "G4S_MASKED_SPLIT_WAYS":
        monkeypatch.setenv("G4S_MASKED_SPLIT_FLOP", "20000")
    got, _, info = _check(A, B, M, K, N, mask, "plus_times", exact=True)
    assert np.array_equal(got, base)
    for name in ("min_plus", "or_and"):
        _check(A, B, M, K, N, mask, name)
    if switch[0] == "G4S_MASKED_WAVE_FLOP":
        assert info0["rows_wave"] > 0 and info["rows_wave"] == 0 and info["rows_lds"] == info0["rows_lds"] + info0["rows_wave"]
    elif switch[0] == "G4S_MASKED_LDS_LARGE":
        assert info["rows_global"] > info0["rows_global"]
    elif switch[0] == "G4S_MASKED_LDS_SMALL":
        assert info["rows_lds"] > 0 and info["rows_global"] == info0["rows_global"]
    else:
        assert info0["rows_split"] == 0 and info["rows_split"] >= 3


# ------------------------------------------------------------------------------------------------ 13: the C++ header
CPP_MASKED = r"""
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
    g4s_masked_info info;
    g4s::MaskedSpGEMM(a, a, a, c, std::plus<double>(), g4s::min_op<double>(), &info);
    std::printf("%d %d %lld %lld\n", c.rows, c.nnz, (long long)info.mask_nnz, (long long)g4s::TriangleCount(a));
    for (int i = 0; i <= c.rows; ++i) std::printf("%d\n", c.rowptr[i]);
    for (int k = 0; k < c.nnz; ++k) std::printf("%d %.17g\n", c.colids[k], c.values[k]);
    return 0;
}
"""


def test_cpp_header_masked_min_plus_and_triangles_run(tmp_path):
    """g4s::MaskedSpGEMM with (std::plus, g4s::min_op) and g4s::TriangleCount through include/g4s/csr.hpp on host arrays"""
    src, exe, inp = tmp_path / "masked.cpp", str(tmp_path / "masked"), tmp_path / "a.txt"
    src.write_text(CPP_MASKED)
    lib = os.path.join(ROOT, "g4s_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lg4s_hip", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    n = 3000
    rp, ci, _ = power_law_csr(n, n, 37, 600)
    G = mref.symmetric_simple_graph(rp, ci, n)
    rp, ci, _ = _csr_of(G)
    va = np.random.default_rng(3).uniform(0.1, 2.0, ci.size)
    inp.write_text(f"{n} {ci.size}\n" + "\n".join(map(str, rp)) + "\n" + "\n".join(f"{c} {float(v)!r}" for c, v in zip(ci, va)) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rows, nnz, mask_nnz, tri = map(int, lines[0].split())
    assert (rows, nnz, mask_nnz) == (n, ci.size, ci.size)
    assert tri == mref.triangles_lower(G) > 0
    crpt = np.array(lines[1:rows + 2], dtype=np.int64)
    ent = [l.split() for l in lines[rows + 2:rows + 2 + nnz]]
    ccol, cval = np.array([int(c) for c, _ in ent]), np.array([float(v) for _, v in ent])
    assert np.array_equal(crpt, rp) and np.array_equal(ccol, ci)
    want, hit = mref.spgemm_masked((rp, ci, va), (rp, ci, va), n, n, (rp, ci), "min_plus")
    assert ref.same_values(cval, want) and hit.any()
