"""The blocked SpMV path (g4s_amd/csrc/spmv_pb.hip) where its x comes from and its y goes: hot_x gathered at the ranks the producer reads it at, and the
16-byte forms of the producer's staging loads (hot_x always, the caller's x when it is 16-byte aligned) and of the consumer's y stores and old-y reads (y
16-byte aligned), with the 8-byte forms beside them.

One matrix per band width W, the smallest on which that can go wrong: rows = cols = 2·9·W + 1 (odd: the last natural column band and the last row band
are ONE column / row wide, so neither holds a whole pair), G4S_PB_HOT_BANDS=9, G4S_PB_PCHUNK=8192 (every hot band has at least three full items and a
tail), 4–5·10^5 entries. The hot columns are every other column of the first 18·W (but column W), of degree 2 or 3 in a pattern that does not follow the
column id, so that rank order and column order differ everywhere; the cold columns have degree 0 or 1. Even row bands are heavy enough to be split over
several consumer items (atomics), odd ones are written once (the 16-byte stores). A second shape, 2·9·W + 3, puts an odd last column / row behind a
whole pair.

  * the plan's G4S_DEBUG line equals the numpy model of tests/pb_cases.py;
  * integer values and x[c] = (c mod 1021) + 1: the product equals the oracle bit for bit — a wrong gather position or a shifted pair is a wrong integer —
    with x and y each 16-byte aligned or only 8-byte aligned (a view one element into a buffer), beta 0 (incoming y all NaN) and beta 1;
  * a NaN in x at a column of hot band 8, at the last and the first column of two neighbouring natural bands, at the last column of the matrix: exactly
    the rows that reference the column become NaN;
  * min-plus and or-and equal tests/spmv_semiring_ref.py, aligned and not, with and without SPMV_ACCUMULATE.
(A deal of the hot items over the XCDs and a gather of hot_x in column order were measured and not kept, DESIGN §4.1 (b): they left no switch to test.)"""
import types

import numpy as np
import pytest
import torch

from tests import pb_cases as pc
from tests import spmv_semiring_ref as ref
from tests.test_spmv_pb_limits_gpu import PLAN_LINE, FIELDS, TOL, NAN, _semiring_inputs

pytestmark = pytest.mark.gpu
HOT, PCHUNK = 9, 8192


@pytest.fixture(params=["device", "16384"])
def band(request, monkeypatch):
    monkeypatch.setenv("G4S_DEBUG", "1")
    monkeypatch.setenv("G4S_PB_HOT_BANDS", str(HOT))
    monkeypatch.setenv("G4S_PB_PCHUNK", str(PCHUNK))
    monkeypatch.delenv("G4S_PB_CCHUNK", raising=False)
    if request.param == "16384":
        monkeypatch.setenv("G4S_PB_BAND", "16384")
    else:
        monkeypatch.delenv("G4S_PB_BAND", raising=False)
    return pc.BAND_NARROW if request.param == "16384" else pc.BAND_WIDE


_MATRIX = {}


def _matrix(W, tail=1):
    """(rowptr, colids, integer values, integer x, integer y0, the model's plan), built once per (W, tail) and read-only."""
    if (W, tail) not in _MATRIX:
        n = 2 * HOT * W + tail
        rng = np.random.default_rng(11 + tail)
        col = np.arange(n, dtype=np.int64)
        hot = (col < 2 * HOT * W) & (col % 2 == 0)
        deg = np.where(hot, 2 + ((col // 2) * 2654435761 >> 7) % 2, 0)
        cold = np.flatnonzero(~hot)
        deg[cold[rng.random(cold.size) < 0.2]] = 1
        deg[[W - 1, W]] = 1                                              # the neighbours across a natural band boundary, both cold (NaN cases)
        deg[n - tail:] = 1
        ci = np.repeat(col, deg)
        # rows: even row bands three times as heavy as odd ones, the last band's rows (one, or three) a few entries each
        RB = (n + W - 1) // W
        weight = np.where(np.arange(RB) % 2 == 0, 3.0, 1.0)
        weight[RB - 1] = 0.0
        rb = rng.choice(RB, size=ci.size, p=weight / weight.sum())
        ri = rb * W + rng.integers(0, W, ci.size)
        ri[rng.choice(ci.size, 5 * tail, replace=False)] = n - 1 - (np.arange(5 * tail) % tail)
        key = np.unique(ri * n + ci)                                     # CSR order, no duplicate entries
        ri, ci = key // n, key % n
        assert ci[-1] == n - 1 or (ci == n - 1).any()
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(ri, minlength=n))]).astype(np.int32)
        va = rng.integers(-4, 5, ci.size).astype(np.float64)
        va[va == 0] = 3.0
        x = (col % 1021 + 1).astype(np.float64)
        y0 = rng.integers(-50, 51, n).astype(np.float64)
        P = pc.plan(rowptr, ci, n, n, W, hot=HOT, pchunk=PCHUNK)
        full = [it for it in P.pitems if it[2] - it[1] == P.kPC]
        per_band = np.bincount([it[0] for it in full], minlength=P.CB)
        assert P.H == HOT and per_band[:HOT].min() >= 3, per_band[:HOT]
        assert P.split and len(P.split) < P.RB                           # both kinds of row band
        assert not np.array_equal(P.hot_cols, np.sort(P.hot_cols)) and not np.array_equal(P.hot_cols, np.sort(P.hot_cols)[::-1])
        out = (rowptr, ci.astype(np.int32), va, x, y0, P)
        for a in out[:5]:
            a.setflags(write=False)
        _MATRIX[W, tail] = out
    return _MATRIX[W, tail]


def _create(capfd, W, tail=1, values=None):
    from g4s_amd import capi, host
    rowptr, ci, va, _, _, P = _matrix(W, tail)
    n = len(rowptr) - 1
    capfd.readouterr()
    A = host.CSR.from_host(np.array(rowptr), np.array(ci), np.array(va if values is None else values), n, n, spmv_flags=capi.SPMV_BLOCKED)
    inf = A.info()
    lines = PLAN_LINE.findall(capfd.readouterr().err)
    assert inf["spmv_path"] == pc.PATH_BLOCKED and len(lines) == 1, (inf, lines)
    got, want = tuple(int(v) for v in lines[0]), P.debug_fields()
    print(f"W={W} tail={tail}: plan {dict(zip(FIELDS, got))}")
    assert got == want, "the plan differs from the model: " + ", ".join(f"{f} {g} (model {w})" for f, g, w in zip(FIELDS, got, want) if g != w)
    return A


def _view(a, aligned):
    """a on the device, 16-byte aligned, or 8-byte-only aligned: a view one element into a buffer."""
    buf = torch.empty(len(a) + 2, dtype=torch.float64, device="cuda")
    off = (0 if buf.data_ptr() % 16 == 0 else 1) + (0 if aligned else 1)
    v = buf[off:off + len(a)]
    v.copy_(torch.from_numpy(np.array(a)))
    assert (v.data_ptr() % 16 == 0) == aligned and v.data_ptr() % 8 == 0
    return v


def _exact(W, tail, x=None):
    rowptr, ci, va, ix, _, _ = _matrix(W, tail)
    out = np.zeros(len(rowptr) - 1, np.int64)
    np.add.at(out, pc.row_of(rowptr), va.astype(np.int64) * (ix if x is None else x).astype(np.int64)[ci])
    return out.astype(np.float64)


@pytest.mark.parametrize("tail", [1, 3])
def test_integer_product_is_exact_at_every_alignment(oracle, capfd, band, tail):
    rowptr, ci, va, x, y0, _ = _matrix(band, tail)
    A = _create(capfd, band, tail)
    want = {b: oracle.spmv(rowptr, ci, va, x, None if b == 0.0 else y0, 1.0, b) for b in (0.0, 1.0)}
    assert np.array_equal(want[0.0], _exact(band, tail)) and np.array_equal(want[1.0], _exact(band, tail) + y0)
    for x_aligned in (True, False):
        for y_aligned in (True, False):
            for beta in (0.0, 1.0):
                xd = _view(x, x_aligned)
                yd = _view(np.full(len(y0), NAN) if beta == 0.0 else y0, y_aligned)
                y = A.spmv(xd, yd, 1.0, beta).cpu().numpy()
                bad = np.flatnonzero(y != want[beta])
                assert bad.size == 0, (f"W={band} x aligned {x_aligned} y aligned {y_aligned} beta {beta}: {bad.size} rows differ from the exact product, "
                                       f"first row {bad[0]}: {y[bad[0]]!r} vs {want[beta][bad[0]]!r}")


def test_nan_in_x_reaches_exactly_the_rows_that_reference_it(capfd, band):
    rowptr, ci, va, x, _, P = _matrix(band)
    W, n = band, len(rowptr) - 1
    A = _create(capfd, band)
    want = _exact(band, 1)
    deg = np.bincount(ci, minlength=n)
    picks = {"hot band 8": int(P.hot_cols[8 * W + W // 3]), "last column of a natural band": W - 1, "first column of the next band": W,
             "last column of the matrix": n - 1}
    assert P.col_band[picks["hot band 8"]] == 8
    for what, c in picks.items():
        assert deg[c] > 0 and (what == "hot band 8" or P.col_band[c] >= P.H), (what, c)
        xn = np.array(x)
        xn[c] = NAN
        hit = np.zeros(n, bool)
        hit[pc.row_of(rowptr)[ci == c]] = True
        y = A.spmv(_view(xn, True), _view(np.full(n, NAN), True)).cpu().numpy()
        assert np.array_equal(np.isnan(y), hit), f"{what} (column {c}): NaN in rows {np.flatnonzero(np.isnan(y) != hit)[:8]} against the rows that reference it"
        assert np.array_equal(y[~hit], want[~hit]), what


@pytest.mark.parametrize("semiring", ["min_plus", "or_and"])
def test_semiring_products_equal_the_reference(capfd, band, semiring):
    rowptr, ci, _, _, _, _ = _matrix(band)
    n = len(rowptr) - 1
    rng = np.random.default_rng(5)
    va, x, y0 = _semiring_inputs(types.SimpleNamespace(colids=ci, cols=n, rows=n), semiring, rng)
    A = _create(capfd, band, values=va)
    for accumulate in (False, True):
        for aligned in (True, False):
            yd = _view(y0 if accumulate else np.full(n, NAN), aligned)
            out = A.spmv_semiring(_view(x, aligned), yd, semiring=semiring, accumulate=accumulate).cpu().numpy()
            expect = ref.spmv(rowptr, ci, va, x, semiring, y0 if accumulate else None)
            bad = np.flatnonzero((out + 0.0) != (expect + 0.0))
            assert bad.size == 0, f"W={band} {semiring} accumulate={accumulate} aligned={aligned}: {bad.size} rows differ, first {bad[0]}: {out[bad[0]]!r} vs {expect[bad[0]]!r}"
            assert ref.same_values(out, expect)
