"""g4s_spgemm_masked and g4s_triangle_count on the cases of tests/masked_cases.py: rows AT and JUST PAST every cut between the seven row classes, on the tile,
pad, clip, part and fold edges of each kernel, over every semiring, with values and pattern-only, and under the G4S_MASKED_* switches that move the cuts
(masked_cases.RUNS). Each run calls the C entry point on arrays it owns, cval pre-filled with NaN, and compares every entry bit for bit with
tests/masked_ref.py (integer values: every sum is exact; −0 and +0 taken as equal) — and the `g4s masked classes:` line the library prints under G4S_DEBUG
with masked_cases.expected_counts, count for count, and g4s_masked_info with masked_cases.expected_info: a row that drifts into the neighbouring class still
gives the right values, and g4s_masked_info adds three classes into one field, so without the line the edge it was built for would go untested unnoticed.
tests/test_masked_cases_cpu.py proves the cases themselves.

No run failed against the library as it stood before these tests: all cases, modes, semirings and both pointer forms, and every triangle count, came out
bit-equal with the class counts the model predicts."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from tests import masked_cases as mc
from tests import masked_ref

pytestmark = pytest.mark.gpu

LINE = re.compile(r"g4s masked classes: skip (\d+) wave (\d+) lds_small (\d+) lds_large (\d+) global (\d+) split_lds (\d+) split_global (\d+) \(products (\d+)\)")
KEYS = mc.CLASSES + ("products",)
INFO = ("rows_wave", "rows_lds", "rows_global", "rows_split")


def _forms(name):
    """values over every semiring the case declares; pattern-only as counts (plus-times) and as marks (or-and)"""
    sems = mc.semirings_of(name)
    return [(s, False) for s in sems] + [(s, True) for s in ("plus_times", "or_and") if s in sems]


RUNS = [(name, mode, semiring, pattern_only) for name in mc.NAMES for mode in mc.RUNS[name] for semiring, pattern_only in _forms(name)]
HOST_RUNS = [(name, mode) for name in mc.HOST_FORM for mode in mc.RUNS[name][-1:]]
_id = lambda r: "-".join(str(x) for x in r[:3]) + ("-pattern_only" if r[3] else "-values")


@functools.lru_cache(maxsize=None)
def _want(name, semiring, pattern_only):
    """the reference (computed once per case, semiring and form, read-only)"""
    c = mc.build(name)
    A, B = mc.operands(c, semiring)
    out = masked_ref.spgemm_masked(A, B, c.M, c.N, c.mask, semiring, pattern_only)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def _on_device(name, zeros):
    c = mc.build(name)
    A, B = mc.operands(c, "or_and" if zeros else "plus_times")
    return tuple(torch.from_numpy(x.copy()).cuda() for x in A + B + c.mask)   # (the case's arrays are read-only; torch wants writable ones)


def _bits(v):
    return (np.asarray(v, np.float64) + 0.0).view(np.int64)           # −0 and +0 taken as equal, as in semiring_ref.same_values


def _counts_of_line(err):
    lines = LINE.findall(err)
    assert len(lines) == 1, f"exactly one class line per call, got {len(lines)}: {err[-2000:]}"
    return dict(zip(KEYS, map(int, lines[0])))


def _call(name, semiring, pattern_only, device_form, capfd):
    """one g4s_spgemm_masked call into a cval of NaN; returns (cval, the counts of the debug line, info)"""
    from g4s_amd import capi, host
    c = mc.build(name)
    info = capi.MaskedInfo()
    null = C.c_void_p(0)
    flags = host.SEMIRINGS[semiring]
    if device_form:
        arrs = _on_device(name, semiring == "or_and")
        cval = torch.full((len(c.mask[1]),), float("nan"), dtype=torch.float64, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())
        flags |= capi.DEVICE_POINTERS
        torch.cuda.synchronize()
    else:
        A, B = mc.operands(c, semiring)
        arrs = [x.copy() for x in A + B + c.mask]
        cval = np.full(len(c.mask[1]), np.nan)
        P = lambda a: C.c_void_p(a.ctypes.data)
        flags |= capi.HOST_POINTERS
    capfd.readouterr()
    capi.check(capi.load().g4s_spgemm_masked(c.M, c.K, c.N, P(arrs[0]), P(arrs[1]), null if pattern_only else P(arrs[2]), P(arrs[3]), P(arrs[4]),
                                             null if pattern_only else P(arrs[5]), P(arrs[6]), P(arrs[7]), P(cval), flags, C.byref(info), None))
    if device_form:
        torch.cuda.synchronize()
        cval = cval.cpu().numpy()
    return cval, _counts_of_line(capfd.readouterr().err), info


def _check(name, mode, semiring, pattern_only, got, line, info):
    c = mc.build(name)
    want, hit = _want(name, semiring, pattern_only)
    rows_of = lambda idx: sorted({c.rows[r].tag for r in np.searchsorted(c.mask[0], idx, side="right") - 1})
    left = np.flatnonzero(np.isnan(got))
    assert left.size == 0, f"{left.size} entries of cval were never written, first {left[0]}; rows {rows_of(left)[:6]}"
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{bad.size} values differ, first at entry {bad[0]}: {got[bad[0]]!r} for {want[bad[0]]!r}; rows {rows_of(bad)[:6]}"
    stray = np.flatnonzero(~hit & (got != mc.IDENTITY[semiring]))
    assert stray.size == 0, f"{stray.size} entries without a product are not the identity; rows {rows_of(stray)[:6]}"
    counts = mc.expected_counts(c, mode)
    print(f"{name} {mode} {semiring} {'pattern-only' if pattern_only else 'values'}: {mc.debug_line(line)}")
    assert line == counts, f"class line {line}, expected {counts}"
    want_info = mc.expected_info(c, mode)
    assert {k: getattr(info, k) for k in INFO} == want_info and info.products == counts["products"] and info.mask_nnz == len(c.mask[1]), \
        f"info {[(k, getattr(info, k)) for k, _ in info._fields_]}, expected {want_info}"


def _set(mode, monkeypatch):
    for k, v in mc.MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("G4S_DEBUG", "1")


@pytest.mark.parametrize("name,mode,semiring,pattern_only", RUNS, ids=[_id(r) for r in RUNS])
def test_masked_rows_on_the_class_limits(name, mode, semiring, pattern_only, monkeypatch, capfd):
    _set(mode, monkeypatch)
    got, line, info = _call(name, semiring, pattern_only, True, capfd)
    _check(name, mode, semiring, pattern_only, got, line, info)


@pytest.mark.parametrize("semiring", ["plus_times", "min_plus"])
@pytest.mark.parametrize("name,mode", HOST_RUNS)
def test_host_pointer_form_gives_the_same_bits_and_the_same_info(name, mode, semiring, monkeypatch, capfd):
    """one case per class through the host-pointer form: the values, the class line and the info of the device form"""
    _set(mode, monkeypatch)
    got_d, line_d, info_d = _call(name, semiring, False, True, capfd)
    got_h, line_h, info_h = _call(name, semiring, False, False, capfd)
    _check(name, mode, semiring, False, got_h, line_h, info_h)
    assert np.array_equal(got_h.view(np.int64), got_d.view(np.int64)) and line_h == line_d
    assert all(getattr(info_h, k) == getattr(info_d, k) for k, _ in info_h._fields_)


# ------------------------------------------------------------------------------------------------ triangles
def _triangles(n, rp, ci, monkeypatch, capfd, mode="default", host_form=False):
    """(count, the counts of the class line or None where no product ran, info) of one g4s_triangle_count call"""
    from g4s_amd import capi
    _set(mode, monkeypatch)
    count, info = C.c_int64(-1), capi.MaskedInfo()
    if host_form:
        arrs, P, flags = (rp.copy(), ci.copy()), (lambda a: C.c_void_p(a.ctypes.data)), capi.HOST_POINTERS
    else:
        arrs = (torch.from_numpy(rp.copy()).cuda(), torch.from_numpy(np.concatenate([ci, np.zeros(1, np.int32)])).cuda())   # (never an empty tensor)
        P, flags = (lambda t: C.c_void_p(t.data_ptr())), capi.DEVICE_POINTERS
        torch.cuda.synchronize()
    capfd.readouterr()
    capi.check(capi.load().g4s_triangle_count(n, P(arrs[0]), P(arrs[1]), C.byref(count), flags, C.byref(info), None))
    err = capfd.readouterr().err
    return count.value, (_counts_of_line(err) if LINE.search(err) else None), info


def _scipy_count(n, rp, ci):
    import scipy.sparse as sp
    return masked_ref.triangles_lower(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n)))


def _check_triangles(n, edges, monkeypatch, capfd, mode="default", want=None, host_form=False):
    rp, ci = mc.graph_csr(n, edges)
    count, line, info = _triangles(n, rp, ci, monkeypatch, capfd, mode, host_form)
    mlen, flop = mc.lower_rows(rp, ci)
    counts = mc.counts_of(mlen, flop, mc.cuts_of(mc.MODES[mode]))
    print(f"n {n} {mode}: {count} triangles; {line}")
    assert count == _scipy_count(n, rp, ci) and (want is None or count == want)
    assert info.mask_nnz == int(mlen.sum()) and info.products == counts["products"]      # nnz(L), and Σ_i Σ_{p ∈ L(i,:)} nnz(L(p,:)) over the rows with work
    if mlen.sum() == 0:
        assert line is None and count == 0, "an empty L runs no product"
    else:
        assert line == counts, f"class line {line}, expected {counts}"
        assert {k: getattr(info, k) for k in INFO} == mc.info_of(counts)
    return count, counts


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33])
def test_triangles_of_small_cliques_at_the_grid_of_the_lower_pass(n, monkeypatch, capfd):
    """n / 32 + 1 workgroups of 32 rows, and lcnt[n] written by the row behind the last: n on either side of one workgroup's rows"""
    for host_form in (False, True):
        _check_triangles(*mc.clique(n), monkeypatch, capfd, want=n * (n - 1) * (n - 2) // 6, host_form=host_form)


def test_triangles_of_an_upper_triangle_are_none(monkeypatch, capfd):
    n, edges = mc.clique(40)
    rp = np.concatenate([[0], np.cumsum(np.arange(n - 1, -1, -1))]).astype(np.int32)      # row i holds i + 1 … n − 1
    ci = np.concatenate([np.arange(i + 1, n) for i in range(n)]).astype(np.int32)
    count, line, info = _triangles(n, rp, ci, monkeypatch, capfd)
    assert count == 0 and line is None and (info.mask_nnz, info.products, info.rows_wave, info.rows_lds) == (0, 0, 0, 0)


@pytest.mark.parametrize("k", [65, 66, 67])
def test_triangles_of_cliques_across_the_wave_cut(k, monkeypatch, capfd):
    """the longest rows of L have 64, 65 and 66 entries"""
    count, counts = _check_triangles(*mc.clique(k), monkeypatch, capfd, want=k * (k - 1) * (k - 2) // 6)
    assert counts["lds_small"] == k - 65 and counts["wave"] == k - 2 - counts["lds_small"]


def test_triangles_with_rows_of_4095_4096_and_4097_products(monkeypatch, capfd):
    n, edges, extra = mc.rows_with_products()
    count, counts = _check_triangles(n, edges, monkeypatch, capfd)
    base = _check_triangles(*mc.clique(128), monkeypatch, capfd)[1]
    assert (counts["wave"], counts["lds_small"]) == (base["wave"] + 2, base["lds_small"] + 1), "the rows of 4 095 and 4 096 products are wave rows, that of 4 097 is not"


@pytest.mark.parametrize("h,cls", [(1024, "lds_small"), (1025, "lds_large"), (8192, "lds_large"), (8193, "global")])
def test_triangles_of_a_hub_over_a_ring(h, cls, monkeypatch, capfd):
    """One hub whose lower neighbourhood is a ring of h vertices: h triangles, the hub row in the class of its h mask entries. A plain ring gives the hub row
    only h products, fewer than 20 000 at all four sizes — so the split run takes the ring in which every vertex is joined to the 24 before it (24·h products,
    its triangles counted by the reference): unsplit and split, the same count."""
    count, counts = _check_triangles(*mc.hub_over_ring(h), monkeypatch, capfd, want=h)
    assert counts[cls] == 1 and counts["wave"] == h - 2 and counts["skip"] == 2   # (vertex 1 meets only vertex 0, which has no lower neighbour)
    n, edges = mc.hub_over_ring(h, 24)
    whole, counts = _check_triangles(n, edges, monkeypatch, capfd)
    assert counts[cls] == 1 and counts["split_lds"] + counts["split_global"] == 0
    split, counts = _check_triangles(n, edges, monkeypatch, capfd, mode="split_flop_20000")
    assert counts["split_lds" if h <= 1024 else "split_global"] == 1 and counts[cls] == 0
    assert split == whole > h
