"""The cases of tests/structured_cases.py have the properties their names claim, sit on the intended side of every selection threshold by at
least one whole entry, and the oracle's product on each equals a numpy.longdouble row-by-row product (1e-14·Σ|terms|) — so that
tests/test_spmv_structured_gpu.py compares the device with a checked reference on checked inputs. No GPU."""
import re

import numpy as np
import pytest

from tests import structured_cases as sc

DIA = [c.name for c in sc.dia_cases()]
BLOCK = [c.name for c in sc.block_cases()]


def _offsets(m):
    return np.unique(m.colids.astype(np.int64) - sc.row_of(m.rowptr))


def _longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def _check_common(m, c):
    assert m.rowptr.dtype == np.int32 and m.colids.dtype == np.int32 and m.values.dtype == np.float64
    assert len(m.rowptr) == m.rows + 1 and m.rowptr[0] == 0 and m.rowptr[-1] == len(m.colids) == len(m.values)
    assert np.all(np.diff(m.rowptr) >= 0)
    assert len(m.colids) == 0 or (m.colids.min() >= 0 and m.colids.max() < m.cols)
    assert np.all(np.abs(m.values) < 1.0)
    ascending = np.ones(len(m.colids), bool)
    ascending[1:] = np.diff(m.colids.astype(np.int64)) > 0
    ascending[m.rowptr[:-1][m.rowptr[:-1] < len(m.colids)]] = True
    assert bool(ascending.all()) != bool(c.claims.get("unsorted", False)), "rows are sorted unless the case says otherwise"
    for key in ("rows", "cols"):
        if key in c.claims:
            assert getattr(m, key) == c.claims[key]
    if "nnz" in c.claims:
        assert len(m.colids) == c.claims["nnz"]
    assert sc.expected_path(m.rows, m.cols, m.rowptr, m.colids) == c.path


@pytest.mark.parametrize("name", DIA)
def test_diagonal_case_has_its_claimed_properties(name):
    c, m = sc.case(name), sc.build(name)
    _check_common(m, c)
    cl = c.claims
    offs = _offsets(m)
    nnz, lens = len(m.colids), np.diff(m.rowptr)
    assert len(offs) == cl["nd"], "distinct offsets"
    if c.path == sc.PATH_DIAGONAL:
        assert np.array_equal(sc.dia_offsets(m.rows, m.cols, m.rowptr, m.colids), offs)
    if cl.get("far_offsets"):
        assert offs.max() >= 1000 and offs.min() <= -1000 and np.any(np.diff(offs) > 1)
        assert lens[0] < len(offs) and lens[-1] < len(offs)             # boundary rows lose entries on both sides
    # every case at least one whole entry away from the fill threshold: float rounding cannot decide the path
    thr = sc.DIA_MIN_FILL * len(offs) * m.rows
    assert abs(nnz - thr) >= 1.0
    if "fill_side" in cl:
        assert (nnz > thr) == (cl["fill_side"] == "above") and abs(nnz - thr) <= 2.5, "just beside the threshold"
        assert m.rows >= sc.DIA_MIN_ROWS and nnz >= sc.DIA_MIN_NNZ and len(offs) <= sc.DIA_MAX_DIAGS    # nothing else decides
    elif c.path == sc.PATH_DIAGONAL:
        assert nnz > thr
    if "fill" in cl:
        assert cl["fill"][0] <= nnz / (len(offs) * m.rows) <= cl["fill"][1]
    if cl.get("masks_with_holes"):
        # interior rows (every offset inside the matrix) that miss some, but not all, of their entries
        r = np.arange(m.rows)
        inside = (r + offs.min() >= 0) & (r + offs.max() < m.cols)
        assert np.sum(inside & (lens > 0) & (lens < len(offs))) > 50
    if "trailing_empty" in cl:
        t = cl["trailing_empty"]
        assert np.all(lens[-t:] == 0) and lens[-t - 1] > 0
        assert np.all(m.rowptr[-t - 1:] == nnz)                          # the refill kernel's k0 of these rows is nnz
    if "empty_run" in cl:
        inner = lens[:m.rows - cl.get("trailing_empty", 0)]
        assert _longest_run(inner == 0) == cl["empty_run"] and inner[0] > 0 and inner[-1] > 0
    if "workgroups2" in cl:
        assert sc.dia_workgroups(m.rows, True)[0] == cl["workgroups2"]
    if "ld_remainder" in cl:
        assert m.rows % 64 == cl["ld_remainder"] and m.rows % 2 == 1
    if "odd_row" in cl:
        r, S = cl["odd_row"], sc.DIA_SAMPLE_ROWS
        sampled = [(a, min(m.rows, a + S)) for a in (0, max(0, m.rows // 2 - S // 2), max(0, m.rows - S))]
        assert not any(a <= r < b for a, b in sampled), "the candidate scan must not visit the row"
        k = m.rowptr[r]
        pair = m.colids[k:k + 2]
        assert pair[1] <= pair[0] and (pair[1] < pair[0]) == name.startswith("swap")
        # the only defect: every other row is ascending
        bad = [q for q in range(m.rows) if np.any(np.diff(m.colids[m.rowptr[q]:m.rowptr[q + 1]].astype(np.int64)) <= 0)]
        assert bad == [r]
    if name == "inst_nd33_rows4098":
        assert len(offs) == sc.DIA_MAX_DIAGS + 1 and nnz > thr           # only the offset count refuses it


def test_instantiation_cases_cover_every_template():
    """ND = 8, 16, 32 of spmv_dia_kernel / dia_refill_kernel and 8, 16 of spmv_dia2_kernel are chosen by nd <= 8, <= 16, else: both sides of both limits."""
    assert set(sc.INSTANTIATION_ND) >= {1, 8, 9, 16, 17, 32} and set(sc.REFRESH_ND) >= {8, 9, 16, 17, 32}
    for nd in sc.INSTANTIATION_ND:
        rows = {sc.build(f"inst_nd{nd}_rows{r}").rows % 2 for r in (4098, 4097)}
        assert rows == {0, 1}
    assert sorted(sc.case(n).claims["workgroups2"] for n in DIA if n.startswith("geometry_") and "wg" in n) == [2, 7, 8, 9]
    # 2 workgroups is the fewest the path can launch: below 1024 rows it is not taken
    assert sc.dia_workgroups(sc.DIA_MIN_ROWS, True)[0] == 2 and sc.dia_workgroups(sc.DIA_MIN_ROWS - 1, True)[0] == 2
    assert [sc.dia_workgroups(sc.build(n).rows, True)[1] for n in DIA if n.startswith("geometry_") and "wg" in n] == [8, 8, 8, 16]


@pytest.mark.parametrize("name", BLOCK)
def test_block_case_has_its_claimed_properties(name):
    c, m = sc.case(name), sc.build(name)
    _check_common(m, c)
    cl = c.claims
    nnz, lens = len(m.colids), np.diff(m.rowptr)
    assert sc.bcsr_block(m.rows, m.cols, m.rowptr, m.colids) == cl["block"]
    found = re.search(r"_b(\d)", name)
    b = int(found.group(1)) if found else 3                              # the block size the case was generated with
    if m.rows % b == 0:
        nb = lens[::b] // b                                             # blocks per block-row
        assert np.all(np.repeat(nb * b, b) == lens)
    if "max_blocks" in cl:
        assert nb.max() == cl["max_blocks"] and np.sum(nb == nb.max()) == 1
        assert abs(cl["max_blocks"] - sc.tile_blocks(b)) <= 1 or name == "over_b4_and_b2"
        assert nnz >= sc.BCSR_MIN_BLOCKS * b * m.rows                    # the tile decides, not the nnz floor
    if "mod4" in cl:
        assert {int(v) % 4 for v in nb if v > 0} == cl["mod4"] and set(range(1, 9)) <= set(nb.tolist())
        assert _longest_run(nb == 0) == cl["empty_brow_run"] > sc.BCSR_MAX_BROWS
        assert np.all(nb[:cl["leading_empty"]] == 0) and nb[cl["leading_empty"]] > 0
        assert np.all(nb[-cl["trailing_empty_brows"]:] == 0) and nb[-cl["trailing_empty_brows"] - 1] > 0
        assert sc.dia_offsets(m.rows, m.cols, m.rowptr, m.colids) is None
    if name.startswith("gate_nnz"):
        floor = sc.BCSR_MIN_BLOCKS * b * m.rows
        assert nnz == floor - (b * b if "below" in name else 0)
    if "misaligned_brow" in cl:
        n = cl["misaligned_brow"]
        bad = [q for q in range(m.rows // b) if np.any((m.colids[m.rowptr[q * b]:m.rowptr[q * b + 1]][::b]) % b)]
        assert bad == [n]
        # the b rows still agree and stay ascending: only the alignment test refuses it
        rows_n = [m.colids[m.rowptr[n * b + d]:m.rowptr[n * b + d + 1]] for d in range(b)]
        assert all(np.array_equal(rows_n[0], r) for r in rows_n) and np.all(np.diff(rows_n[0]) > 0)
    if "descending_brow" in cl:
        n = cl["descending_brow"]
        first = m.colids[m.rowptr[n * b]:m.rowptr[n * b + 1]]
        assert first[b] < first[0] and np.all(first % b == np.arange(len(first)) % b)
    if name == "rect_cols_2rows":
        assert m.cols == 2 * m.rows and m.colids.max() >= m.rows
    if name in ("gate_rows_mod_b", "gate_cols_mod_b"):
        assert (m.rows % 3 != 0) == (name == "gate_rows_mod_b") and (m.cols % 3 != 0) == (name == "gate_cols_mod_b")
        assert all(getattr(m, "rows" if "rows" in name else "cols") % q for q in (2, 3, 4))


def test_tile_limits_are_the_documented_ones():
    assert [sc.tile_blocks(b) for b in (2, 3, 4)] == [256, 113, 64]
    assert sc.case("over_b4").claims["block"] == 2                       # aligned 4×4 blocks are aligned 2×2 blocks: the smaller form still fits its tile


@pytest.mark.parametrize("name", DIA + BLOCK)
def test_oracle_equals_longdouble_rows(oracle, name):
    m = sc.build(name)
    x = np.random.default_rng(7).uniform(-1, 1, m.cols)
    got = oracle.spmv(m.rowptr, m.colids, m.values, x)
    row = sc.row_of(m.rowptr)
    terms = m.values.astype(np.longdouble) * x[m.colids].astype(np.longdouble)
    want, asum = np.zeros(m.rows, np.longdouble), np.zeros(m.rows, np.longdouble)
    np.add.at(want, row, terms)
    np.add.at(asum, row, np.abs(terms))
    err = np.abs(got.astype(np.longdouble) - want)
    assert np.all(err <= 1e-14 * asum), f"max err / sum|terms| {float(np.max(err / np.maximum(asum, 1e-300)))}"
    assert np.all(got[np.diff(m.rowptr) == 0] == 0.0)
