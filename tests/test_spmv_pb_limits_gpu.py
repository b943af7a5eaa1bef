"""The blocked SpMV path (g4s_amd/csrc/spmv_pb.hip, spmv_path 1) on the cases of tests/pb_cases.py, which sit on the edges of its plan builder and of
its two kernels; tests/test_pb_cases_cpu.py proves that the cases reach those edges. Every case runs at the device's band width (20 448 on an MI355X)
and with G4S_PB_BAND=16384, under the G4S_PB_HOT_BANDS / G4S_PB_PCHUNK / G4S_PB_CCHUNK its edge needs:

  * the plan's G4S_DEBUG line must EQUAL the numpy model of pb_build field by field — band width, column × row bands, hot bands, nnz, padded length,
    micro-runs, producer and consumer items, split bands: this is what makes the plan builder observable (a wrong column degree, hot-band decision,
    rank order or padding rule leaves the product right and shows only here);
  * y = alpha·A·x + beta·y0 within the project's bar of the oracle, |err_i| <= 1e-10·(|alpha|·Σ_k|a_ik x_k| + |beta|·|y0_i|) + 1e-300, for
    (alpha, beta) in {(1, 0), (−2.5, 0.75)}; with beta == 0 the incoming y is all NaN and none may survive (split bands, unsplit bands, empty bands);
  * with integer-valued data (pb_cases.integer_data: every partial sum an exact fp64 integer, whatever the order of the LDS atomics) the result
    equals the reference exactly, for beta 0 and 1;
  * NaN in x on columns no entry references changes nothing; NaN on one referenced cold column and one referenced hot column turns exactly the rows
    that reference them into NaN;
  * min-plus, max-plus and or-and equal tests/spmv_semiring_ref.py exactly, with and without SPMV_ACCUMULATE;
  * one case per edge group again as SPMV_UPDATABLE, through update_values;
  * without a path flag, the path of matrices at the size gates of pb_should_use and just beside its ratio threshold is the one pb_cases.should_use
    gives.
The one edge left to the full-size configuration test is the binned degree count (cols >= 2^20 and nnz >= 2^24): see tests/pb_cases.py."""
import re

import numpy as np
import pytest
import torch

from tests import pb_cases as pc
from tests import spmv_semiring_ref as ref
from tests import structured_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-10
NAN = float("nan")
ALPHA_BETA = ((1.0, 0.0), (-2.5, 0.75))
PLAN_LINE = re.compile(r"g4s blocked SpMV plan: band (\d+), (\d+) x (\d+) bands \((\d+) hot\), nnz (\d+), padded (\d+), micro-runs (\d+) \([0-9.]+ per nonzero\), "
                       r"(\d+) producer / (\d+) consumer items, (\d+) split bands")
FIELDS = ("band", "column bands", "row bands", "hot bands", "nnz", "padded", "micro-runs", "producer items", "consumer items", "split bands")
ENV = ("G4S_PB_HOT_BANDS", "G4S_PB_PCHUNK", "G4S_PB_CCHUNK")


@pytest.fixture(params=["device", "16384"])
def band(request, monkeypatch):
    """The band width the plans of a test are built with: the device's (an MI355X grants a workgroup 160 KiB of LDS: 20 448) or the forced narrow one."""
    monkeypatch.setenv("G4S_DEBUG", "1")
    if request.param == "16384":
        monkeypatch.setenv("G4S_PB_BAND", "16384")
    else:
        monkeypatch.delenv("G4S_PB_BAND", raising=False)
    return pc.BAND_NARROW if request.param == "16384" else pc.BAND_WIDE


def _create(monkeypatch, capfd, name, W, values=None, updatable=False):
    """A blocked-path handle of the case under its environment; the plan's debug line must equal the model's numbers."""
    from g4s_amd import capi, host
    c, m = pc.case(name), pc.build(name, W)
    for var, v in zip(ENV, (c.hot, c.pchunk, c.cchunk)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))
    capfd.readouterr()
    flags = capi.SPMV_BLOCKED | (capi.SPMV_UPDATABLE if updatable else 0)
    A = host.CSR.from_host(np.array(m.rowptr), np.array(m.colids), np.array(m.values if values is None else values), m.rows, m.cols, spmv_flags=flags)
    inf = A.info()                                                      # creates the handle while the variables are set
    lines = PLAN_LINE.findall(capfd.readouterr().err)
    assert inf["spmv_path"] == pc.PATH_BLOCKED, inf
    assert len(lines) == 1, lines
    got, want = tuple(int(v) for v in lines[0]), pc.model(name, W).debug_fields()
    print(f"{name} W={W}: plan {dict(zip(FIELDS, got))}")
    assert got == want, "the plan differs from the model: " + ", ".join(f"{f} {g} (model {w})" for f, g, w in zip(FIELDS, got, want) if g != w)
    return A


_REFERENCE = {}


def _reference(oracle, name, W):
    """Per case and band width, computed once and shared (read-only): {(alpha, beta): oracle product}, Σ|terms| per row, and the integer-data products
    for beta 0 and 1 (the oracle's, which must equal an int64 product)."""
    if (name, W) not in _REFERENCE:
        m = pc.build(name, W)
        want = {(a, b): oracle.spmv(m.rowptr, m.colids, m.values, m.x, None if b == 0.0 else m.y0, a, b) for a, b in ALPHA_BETA}
        _, asum = oracle.spmv_ld(m.rowptr, m.colids, m.values, m.x)
        exact = np.zeros(m.rows, np.int64)
        np.add.at(exact, pc.row_of(m.rowptr), m.ivalues.astype(np.int64) * m.ix.astype(np.int64)[m.colids])
        iwant = {b: oracle.spmv(m.rowptr, m.colids, m.ivalues, m.ix, None if b == 0.0 else m.iy0, 1.0, b) for b in (0.0, 1.0)}
        for b in (0.0, 1.0):
            assert np.array_equal(iwant[b], (exact + (m.iy0.astype(np.int64) if b else 0)).astype(np.float64))
        for a in (asum, *want.values(), *iwant.values()):
            a.setflags(write=False)
        _REFERENCE[name, W] = (want, asum, iwant)
    return _REFERENCE[name, W]


def _spmv(A, x, alpha=1.0, beta=0.0, y0=None):
    """One product; with beta == 0 the incoming y is all NaN."""
    xd = torch.from_numpy(np.array(x)).cuda()
    y = torch.full((A.rows,), NAN, dtype=torch.float64, device="cuda") if beta == 0.0 else torch.from_numpy(np.array(y0)).cuda()
    return A.spmv(xd, y, alpha, beta).cpu().numpy()


def _within(y, want, scale, what):
    err = np.abs(y - want)
    bad = np.flatnonzero(~(err <= TOL * scale + 1e-300))
    print(f"{what}: max err / scale {float(np.max(err / (scale + 1e-300), initial=0.0)):.3e}")
    assert bad.size == 0, f"{what}: {bad.size} rows miss the bar, first row {bad[0]}: {y[bad[0]]!r} vs {want[bad[0]]!r} (Σ|terms| {scale[bad[0]]!r})"


def _check_tolerance(oracle, A, name, W, values=None):
    m = pc.build(name, W)
    if values is None:
        want, asum, _ = _reference(oracle, name, W)
    else:
        want = {(a, b): oracle.spmv(m.rowptr, m.colids, values, m.x, None if b == 0.0 else m.y0, a, b) for a, b in ALPHA_BETA}
        _, asum = oracle.spmv_ld(m.rowptr, m.colids, values, m.x)
    for alpha, beta in ALPHA_BETA:
        y = _spmv(A, m.x, alpha, beta, m.y0)
        assert not np.isnan(y).any(), f"NaN in y (alpha {alpha}, beta {beta}): rows {np.flatnonzero(np.isnan(y))[:8]}"
        _within(y, want[alpha, beta], abs(alpha) * asum + abs(beta) * np.abs(m.y0) * (beta != 0.0), f"{name} W={W} alpha {alpha} beta {beta}")


def _check_integers(oracle, A, name, W):
    m = pc.build(name, W)
    _, _, iwant = _reference(oracle, name, W)
    for beta in (0.0, 1.0):
        y = _spmv(A, m.ix, 1.0, beta, m.iy0)
        bad = np.flatnonzero(y != iwant[beta])
        assert bad.size == 0, f"{name} W={W} beta {beta}: {bad.size} rows differ from the exact integer product, first row {bad[0]}: {y[bad[0]]!r} vs {iwant[beta][bad[0]]!r}"


def _semiring_inputs(m, semiring, rng, sparse=False):
    """Values, x and the y to accumulate into: min-plus in [1, 2] and max-plus in [−2, −1], so that a stray 0.0 (a pad taken for a real slot) or a
    missing identity wins the reduction and shows; or-and with false entries on both sides (sparse: so few true x that hub rows come out false too)."""
    nnz = len(m.colids)
    if semiring == "min_plus":
        return rng.uniform(1, 2, nnz), rng.uniform(1, 2, m.cols), rng.uniform(2, 4, m.rows)
    if semiring == "max_plus":
        return rng.uniform(-2, -1, nnz), rng.uniform(-2, -1, m.cols), rng.uniform(-4, -2, m.rows)
    va = np.where(rng.random(nnz) < 0.2, 0.0, rng.uniform(-1, 1, nnz))
    x = np.where(rng.random(m.cols) < (0.0005 if sparse else 0.08), rng.uniform(0.5, 1, m.cols), 0.0)
    return va, x, np.where(rng.random(m.rows) < 0.7, 0.0, 5.0)


def _check_semiring(A, m, semiring, va, x, y0, what):
    xd = torch.from_numpy(x).cuda()
    for accumulate in (False, True):
        yd = torch.from_numpy(y0.copy()).cuda() if accumulate else torch.full((m.rows,), NAN, dtype=torch.float64, device="cuda")
        out = A.spmv_semiring(xd, yd, semiring=semiring, accumulate=accumulate).cpu().numpy()
        expect = ref.spmv(m.rowptr, m.colids, va, x, semiring, y0 if accumulate else None)
        bad = np.flatnonzero((out + 0.0) != (expect + 0.0))
        assert bad.size == 0, (f"{what} {semiring} accumulate={accumulate}: {bad.size} rows differ, first {bad[0]}: {out[bad[0]]!r} vs {expect[bad[0]]!r} "
                               f"(row length {m.rowptr[bad[0] + 1] - m.rowptr[bad[0]]})")
        assert ref.same_values(out, expect)


@pytest.mark.parametrize("name", pc.NAMES)
def test_plan_equals_the_model(monkeypatch, capfd, band, name):
    A = _create(monkeypatch, capfd, name, band)
    m = pc.build(name, band)
    inf = A.info()
    assert (inf["rows"], inf["cols"], inf["nnz"]) == (m.rows, m.cols, len(m.colids))


@pytest.mark.parametrize("name", pc.NAMES)
def test_product_within_the_bar_and_no_nan_survives(oracle, monkeypatch, capfd, band, name):
    A = _create(monkeypatch, capfd, name, band)
    _check_tolerance(oracle, A, name, band)


@pytest.mark.parametrize("name", pc.NAMES)
def test_integer_data_is_exact(oracle, monkeypatch, capfd, band, name):
    m = pc.build(name, band)
    A = _create(monkeypatch, capfd, name, band, values=m.ivalues)
    _check_integers(oracle, A, name, band)


@pytest.mark.parametrize("name", pc.NAMES)
def test_nan_in_x_reaches_exactly_the_rows_that_reference_it(oracle, monkeypatch, capfd, band, name):
    m, P = pc.build(name, band), pc.model(name, band)
    _, _, iwant = _reference(oracle, name, band)
    A = _create(monkeypatch, capfd, name, band, values=m.ivalues)
    deg = np.bincount(m.colids, minlength=m.cols)
    unreferenced = np.flatnonzero(deg == 0)
    if unreferenced.size:                                               # (one_by_one, one_row, one_col have none)
        x = m.ix.copy()
        x[unreferenced] = NAN
        y = _spmv(A, x)
        assert np.array_equal(y, iwant[0.0]), f"NaN on unreferenced columns changed rows {np.flatnonzero(y != iwant[0.0])[:8]}"
    picks = []
    for hot in (False, True):                                            # one referenced cold column, one referenced hot column where the plan has hot bands
        cand = np.flatnonzero((deg > 0) & ((P.col_band < P.H) == hot))
        if cand.size:
            picks.append(int(cand[cand.size // 2]))
    assert picks and (not P.H or P.col_band[picks[-1]] < P.H)              # (every referenced column of hot_clamped is hot: it has no cold pick)
    x = m.ix.copy()
    x[np.array(picks)] = NAN
    hit = np.zeros(m.rows, bool)
    hit[pc.row_of(m.rowptr)[np.isin(m.colids, picks)]] = True
    y = _spmv(A, x)
    assert np.array_equal(np.isnan(y), hit), f"NaN in rows {np.flatnonzero(np.isnan(y) != hit)[:8]} against the rows that reference columns {picks}"
    assert np.array_equal(y[~hit], iwant[0.0][~hit])


@pytest.mark.parametrize("name", pc.NAMES)
def test_semirings_equal_the_reference(monkeypatch, capfd, band, name):
    m = pc.build(name, band)
    rng = np.random.default_rng(5)
    for semiring in ref.NEW:
        va, x, y0 = _semiring_inputs(m, semiring, rng)
        A = _create(monkeypatch, capfd, name, band, values=va)
        _check_semiring(A, m, semiring, va, x, y0, f"{name} W={band}")
        if semiring == "or_and":
            _, xs, _ = _semiring_inputs(m, semiring, rng, sparse=True)
            _check_semiring(A, m, semiring, va, xs, y0, f"{name} W={band} sparse x")


@pytest.mark.parametrize("name", pc.UPDATABLE_NAMES)
def test_updatable_handles_through_update_values(oracle, monkeypatch, capfd, band, name):
    m = pc.build(name, band)
    rng = np.random.default_rng(6)
    A = _create(monkeypatch, capfd, name, band, values=rng.uniform(-3, 3, len(m.colids)), updatable=True)
    A.update_values(torch.from_numpy(np.array(m.values)).cuda())
    _check_tolerance(oracle, A, name, band)
    A.update_values(torch.from_numpy(np.array(m.ivalues)).cuda())
    _check_integers(oracle, A, name, band)
    for semiring in ref.NEW:
        va, x, y0 = _semiring_inputs(m, semiring, rng)
        A.update_values(torch.from_numpy(va).cuda())
        _check_semiring(A, m, semiring, va, x, y0, f"{name} W={band} updated")
    vnew = rng.uniform(-2, 2, len(m.colids))
    A.update_values(torch.from_numpy(vnew).cuda())
    _check_tolerance(oracle, A, name, band, values=vnew)


@pytest.mark.parametrize("name", pc.AUTO_NAMES)
def test_automatic_path_is_the_probes_decision(oracle, monkeypatch, name):
    """No path flag: pb_should_use decides. The device samples the positions the model samples, and the ratio is exact in fp64: the decision is exact."""
    from g4s_amd import host
    for var in ENV + ("G4S_PB_BAND",):
        monkeypatch.delenv(var, raising=False)
    rp, ci, rows, cols = pc.build_auto(name)
    nnz = len(ci)
    use, ratio = pc.should_use(rows, cols, nnz, ci)
    va = 1.0 + (np.arange(nnz) % 7) / 8.0
    A = host.CSR.from_host(np.array(rp), np.array(ci), va, rows, cols)
    want_path = pc.PATH_BLOCKED if use else pc.PATH_STREAM
    print(f"{name}: modelled ratio {ratio}, path {A.info()['spmv_path']}")
    assert A.info()["spmv_path"] == want_path == sc.expected_path(rows, cols, rp, ci), (name, ratio, A.info())
    x = np.random.default_rng(8).uniform(-1, 1, cols)
    y = _spmv(A, x)
    want = oracle.spmv(rp, ci, va, x)
    _, asum = oracle.spmv_ld(rp, ci, va, x)
    _within(y, want, asum, name)
