"""SpGEMM on the cases of tests/spgemm_cases.py: rows AT and JUST PAST every row-class limit, in both call forms, over every semiring and under the switches
that move those rows to another kernel (spgemm_cases.RUNS). Each run compares C bit for bit with tests/semiring_ref.py (integer values: every sum is exact),
the index arrays of the plus-times product with the oracle's, the flop count with the declared products — and both class histograms that the library prints
under G4S_DEBUG with spgemm_cases.expected_histograms, count for count: a row that drifts into the neighbouring class still gives the right C, and without
that last comparison the edge it was built for would go untested unnoticed. tests/test_spgemm_cases_cpu.py proves the cases themselves."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from tests import semiring_ref
from tests import spgemm_cases as sc

pytestmark = pytest.mark.gpu

SYM_LINE = re.compile(r"g4s symbolic classes: empty (\d+) tiny (\d+) small (\d+) medium (\d+) large (\d+) window (\d+) hub (\d+) \(flop (\d+)\)")
NUM_LINE = re.compile(r"g4s numeric classes: empty (\d+) <=32 (\d+) <=512 (\d+) <=1024 (\d+) <=2048 (\d+) <=4096 (\d+) <=1M (\d+) hub (\d+) rank (\d+)")
RUNS = [(name, mode, semiring) for name in sc.NAMES for mode in sc.RUNS[name] for semiring in sc.semirings_of(name)]


@functools.lru_cache(maxsize=None)
def _want(name, semiring):
    """the reference product (computed once per case and semiring, read-only)"""
    c = sc.build(name)
    out = semiring_ref.spgemm(c.A, c.B, c.M, semiring)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def _on_device(name):
    from g4s_amd import host
    c = sc.build(name)
    own = lambda X: tuple(x.copy() for x in X)                         # (the case's arrays are read-only; torch wants writable ones)
    return host.CSR.from_host(*own(c.A), c.M, c.K), host.CSR.from_host(*own(c.B), c.K, c.N)


@functools.lru_cache(maxsize=None)
def _oracle_pattern(name):
    from tests import oracle_lib
    c = sc.build(name)
    orpt, ocol, _ = oracle_lib.load().spgemm(c.A, c.B, c.N, sort_output=True)
    return orpt, ocol


def _two_call(a, b, semiring, between=None):
    """g4s_spgemm_symbolic + g4s_spgemm_numeric into arrays this test owns: ccol and cval are filled with sentinels first, so that an entry the numeric phase
    leaves unwritten shows as a difference, not as stale memory that happens to be right. between: called after the symbolic call has returned"""
    from g4s_amd import capi, host
    lib = capi.load()
    crpt = torch.full((a.rows + 1,), -7, dtype=torch.int32, device="cuda")
    cnnz = C.c_int64(0)
    torch.cuda.synchronize()
    capi.check(lib.g4s_spgemm_symbolic(a.rows, a.cols, b.cols, host._ptr(a.rowptr), host._ptr(a.colids), host._ptr(b.rowptr), host._ptr(b.colids), host._ptr(crpt),
                                       C.byref(cnnz), None))
    ccol = torch.full((cnnz.value,), -7, dtype=torch.int32, device="cuda")
    cval = torch.full((cnnz.value,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if between:
        between()
    capi.check(lib.g4s_spgemm_numeric(a.rows, a.cols, b.cols, host._ptr(a.rowptr), host._ptr(a.colids), host._ptr(a.values), host._ptr(b.rowptr), host._ptr(b.colids),
                                      host._ptr(b.values), host._ptr(crpt), host._ptr(ccol), host._ptr(cval),
                                      capi.DEVICE_POINTERS | capi.SORT_OUTPUT | host.SEMIRINGS[semiring], None))
    torch.cuda.synchronize()
    return crpt.cpu().numpy(), ccol.cpu().numpy(), cval.cpu().numpy()


def _bits(v):
    return (np.asarray(v, np.float64) + 0.0).view(np.int64)           # −0 and +0 taken as equal, as in semiring_ref.same_values


def _run(name, mode, one_call, semiring, monkeypatch, capfd):
    from g4s_amd import host
    c = sc.build(name)
    a, b = _on_device(name)
    for k, v in sc.MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("G4S_DEBUG", "1")
    capfd.readouterr()
    got = host.HashSpGEMM(a, b, semiring=semiring).to_host() if one_call else _two_call(a, b, semiring)
    err = capfd.readouterr().err
    monkeypatch.delenv("G4S_DEBUG")

    want = _want(name, semiring)
    assert np.array_equal(got[0], want[0]), "row pointer differs"
    rows_of = lambda idx: sorted({c.rows[r].tag for r in np.searchsorted(want[0], idx, side="right") - 1})
    bad = np.flatnonzero(got[1] != want[1])
    assert bad.size == 0, f"{bad.size} column ids differ, first at entry {bad[0]}: {got[1][bad[0]]} for {want[1][bad[0]]}; rows {rows_of(bad)[:6]}"
    bad = np.flatnonzero(_bits(got[2]) != _bits(want[2]))
    assert bad.size == 0, f"{bad.size} values differ, first at entry {bad[0]}: {got[2][bad[0]]!r} for {want[2][bad[0]]!r}; rows {rows_of(bad)[:6]}"
    if semiring == "plus_times":
        orpt, ocol = _oracle_pattern(name)
        assert np.array_equal(got[0], orpt) and np.array_equal(got[1], ocol), "the oracle's index arrays differ"
    flop = sum(r.F for r in c.rows)
    assert host.get_flop(a, b) == flop

    sym_want, num_want = sc.expected_histograms(c, mode, one_call)
    sym, num = SYM_LINE.findall(err), NUM_LINE.findall(err)
    assert len(sym) == 1 and len(num) == 1, err
    sym_got = dict(zip(sc.SYM_CLASSES, map(int, sym[0][:7])))
    num_got = dict(zip(sc.NUM_CLASSES, map(int, num[0])))
    print(f"{name} {mode} {'one-call' if one_call else 'two-call'} {semiring}: symbolic {sym_got} flop {sym[0][7]}; numeric {num_got}")
    assert sym_got == sym_want and int(sym[0][7]) == flop, f"symbolic classes {sym_got}, expected {sym_want}"
    assert num_got == num_want, f"numeric classes {num_got}, expected {num_want}"


@pytest.mark.parametrize("one_call", [True, False], ids=["one_call", "two_call"])
@pytest.mark.parametrize("name,mode,semiring", RUNS)
def test_spgemm_rows_on_the_class_limits(name, mode, one_call, semiring, monkeypatch, capfd):
    """hub_beside_rank_* under mid_tables_4: before this test existed the numeric limit of the "<= 4096" class went to 8 192 whenever the rank path was on, also
    when G4S_SPGEMM_MID_TABLES=4 sends that class to the 8 192-slot key table, whose dense copy and sort hold 4 096 entries: the symbolic hub rows of 4 097 and
    8 192 outputs came back with 4 096 entries written and the rest of ccol / cval untouched. The limit now moves only while the window kernel takes the class."""
    assert semiring in sc.build(name).semirings
    _run(name, mode, one_call, semiring, monkeypatch, capfd)


@pytest.mark.parametrize("semiring", ["plus_times", "min_plus"])
def test_no_rank_set_between_the_two_calls(semiring, monkeypatch, capfd):
    """g4s_spgemm_symbolic under the default environment writes cuts for the long rows of `long`; G4S_SPGEMM_NO_RANK is set before the g4s_spgemm_numeric call on
    the same arrays. Cuts are read by the rank kernel alone: the numeric call must not take the carried state over (it used to, and handed the rows with cuts to
    the window kernel without columns) — it runs as an uncarried numeric call, rank 0 and the rows classed by outputs with the 4 096 limit."""
    c = sc.build("long")
    a, b = _on_device("long")
    monkeypatch.setenv("G4S_DEBUG", "1")
    capfd.readouterr()
    got = _two_call(a, b, semiring, between=lambda: monkeypatch.setenv("G4S_SPGEMM_NO_RANK", "1"))
    err = capfd.readouterr().err
    monkeypatch.delenv("G4S_DEBUG")

    want = _want("long", semiring)
    assert np.array_equal(got[0], want[0]), "row pointer differs"
    assert np.array_equal(got[1], want[1]), f"{np.count_nonzero(got[1] != want[1])} column ids differ"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), f"{np.count_nonzero(_bits(got[2]) != _bits(want[2]))} values differ"
    sym, num = SYM_LINE.findall(err), NUM_LINE.findall(err)
    assert len(sym) == 1 and len(num) == 1, err
    sym_got = dict(zip(sc.SYM_CLASSES, map(int, sym[0][:7])))
    num_got = dict(zip(sc.NUM_CLASSES, map(int, num[0])))
    print(f"long, NO_RANK set between the calls, {semiring}: symbolic {sym_got}; numeric {num_got}")
    assert sc.rank_on(c, "default") and sym_got == sc.expected_histograms(c, "default", False)[0], f"symbolic classes {sym_got}"
    assert num_got == sc.expected_histograms(c, "no_rank", False)[1] and num_got["rank"] == 0, f"numeric classes {num_got}"
    assert "its carried state is not used" in err
