"""The row-streaming SpMV path (g4s_amd/csrc/spmv.hip, spmv_path 0) on the cases of tests/stream_cases.py, which sit on its thresholds: every lanes-per-row
count at its first and last row count, both sides of the 16·nrows switch, 1 / 4 / 5 / 31 heavy rows in one block, every chunk-loop tail, every block
count around the XCD remap, and the device plan builder's run ends. tests/test_stream_cases_cpu.py proves that the cases reach those edges.

For each case, on the plan built from `CSR.from_host` arrays, on the host-built plan (G4S_PLAN_HOST) and on the device-built one (G4S_PLAN_DEVICE):
  * the plan has exactly the blocks, long rows and chunks the model of stream_cases.py says that builder produces;
  * y = alpha·A·x + beta·y is within the project's SpMV bar of the oracle, |err_i| <= 1e-10·(|alpha|·Σ_k|a_ik x_k| + |beta|·|y0_i|) + 1e-300 (as
    tests/test_spmv_gpu.py: _check), NaN in a y that beta == 0 must not read does not leak;
  * every row the model says one lane sums is BIT-identical to the oracle's fp64 left-to-right sum; rows summed by a lane group, a wavefront or in
    chunks are held to the tolerance against the oracle — and to the bits of stream_cases.emulate_spmv, the kernels' additions in their own order;
  * a second call, the plain-load handle (SPMV_NO_NT) and — wherever the model gives a row the same block and reduction in both — the other builder's
    plan give the same bits;
  * NaN in x on columns that one row per block (and one long row) alone references turns exactly those rows of y into NaN;
  * min-plus, max-plus and or-and equal tests/spmv_semiring_ref.py; SpMM on the same plans equals the oracle column by column."""
import numpy as np
import pytest
import torch

from tests import spmv_semiring_ref as ref
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-10
NAN = float("nan")
ALPHA_BETA = ((1.0, 0.0), (-2.5, 0.75))
PLANS = ("arrays", "host", "device")                                    # from_host arrays (the default builder), G4S_PLAN_HOST, G4S_PLAN_DEVICE
MODEL = {"arrays": sc.host_blocks, "host": sc.host_blocks, "device": sc.device_blocks}   # below 2^18 rows the default is the host builder (csr.hip)


def _handle(monkeypatch, m, plan, values=None, no_nt=False):
    from g4s_amd import capi, host
    flags = capi.SPMV_STREAM | (capi.SPMV_NO_NT if no_nt else 0)
    va = m.values if values is None else values
    for var in ("G4S_PLAN_HOST", "G4S_PLAN_DEVICE"):
        monkeypatch.delenv(var, raising=False)
    if plan != "arrays":
        monkeypatch.setenv("G4S_PLAN_HOST" if plan == "host" else "G4S_PLAN_DEVICE", "1")
    A = host.CSR.from_host(np.array(m.rowptr), np.array(m.colids), np.array(va), m.rows, m.cols, spmv_flags=flags)   # copies: the cases are read-only
    inf = A.info()                                                      # creates the handle while the variable is set
    for var in ("G4S_PLAN_HOST", "G4S_PLAN_DEVICE"):
        monkeypatch.delenv(var, raising=False)
    assert inf["spmv_path"] == 0, inf
    return A


_REFERENCE = {}


def _reference(oracle, name):
    """(y0, {(alpha, beta): want}, Σ|terms| per row) of a case, computed once and shared (read-only)."""
    if name not in _REFERENCE:
        m = sc.build(name)
        y0 = np.random.default_rng(99).uniform(-1, 1, m.rows)
        want = {(a, b): oracle.spmv(m.rowptr, m.colids, m.values, m.x, None if b == 0.0 else y0, a, b) for a, b in ALPHA_BETA}
        _, asum = oracle.spmv_ld(m.rowptr, m.colids, m.values, m.x)
        for a in (y0, asum, *want.values()):
            a.setflags(write=False)
        _REFERENCE[name] = (y0, want, asum)
    return _REFERENCE[name]


def _within(y, want, scale, what):
    err = np.abs(y - want)
    bad = np.flatnonzero(~(err <= TOL * scale + 1e-300))
    assert bad.size == 0, f"{what}: {bad.size} rows miss the bar, first row {bad[0]}: {y[bad[0]]!r} vs {want[bad[0]]!r} (Σ|terms| {scale[bad[0]]!r})"


def _spmv(A, x, alpha=1.0, beta=0.0, y0=None):
    rows = A.rows
    y = torch.full((rows,), NAN, dtype=torch.float64, device="cuda") if beta == 0.0 else torch.from_numpy(y0.copy()).cuda()
    return A.spmv(x, y, alpha, beta).cpu().numpy()


def _per_row_block(plan, rows):
    """Per row, its block as (row0, nrows) (−1, −1 for a long row)."""
    out = np.full((rows, 2), -1, np.int64)
    for r0, n, _ in plan.blocks:
        out[r0:r0 + n] = (r0, n)
    return out


@pytest.mark.parametrize("name", sc.NAMES)
def test_plan_equals_the_model(monkeypatch, name):
    m = sc.build(name)
    for plan in PLANS:
        inf = _handle(monkeypatch, m, plan).info()
        assert (inf["tile_nnz"], inf["tile_rows"], inf["long_chunk_nnz"]) == (sc.TILE_NNZ, sc.TILE_ROWS, sc.LONG_CHUNK)
        want = MODEL[plan](m.rowptr, inf["tile_nnz"], inf["tile_rows"], inf["long_chunk_nnz"])
        got = (inf["stream_blocks"], inf["long_rows"], inf["long_chunks"])
        assert got == (len(want.blocks), len(want.long_rows), len(want.chunks)), (plan, got)
        assert (inf["rows"], inf["cols"], inf["nnz"]) == (m.rows, m.cols, len(m.colids))


@pytest.mark.parametrize("name", sc.NAMES)
def test_values_bit_identity_and_variants(oracle, monkeypatch, name):
    m = sc.build(name)
    y0, want, asum = _reference(oracle, name)
    x = torch.from_numpy(m.x.copy()).cuda()
    first, kinds, blocks = {}, {}, {}
    for plan in PLANS:
        A = _handle(monkeypatch, m, plan)
        model = MODEL[plan](m.rowptr)
        kinds[plan], blocks[plan] = sc.row_kinds(m.rowptr, model), _per_row_block(model, m.rows)
        for alpha, beta in ALPHA_BETA:
            y = _spmv(A, x, alpha, beta, y0)
            scale = abs(alpha) * asum + abs(beta) * np.abs(y0) * (beta != 0.0)
            assert not np.isnan(y).any(), f"{plan}: NaN in y ({alpha}, {beta})"
            _within(y, want[alpha, beta], scale, f"{plan} plan, alpha {alpha}, beta {beta}")
            if (alpha, beta) == (1.0, 0.0):
                first[plan] = y
                lane = kinds[plan] == "lane"
                bad = np.flatnonzero(lane & (y != want[alpha, beta]))
                assert bad.size == 0, f"{plan}: {bad.size} one-lane rows differ from the oracle's bits, first row {bad[0]}"
                # every row, the rows several lanes share included: the additions of the kernels in their order, restated in numpy
                bad = np.flatnonzero(y != sc.emulate_spmv(m, model))
                assert bad.size == 0, f"{plan}: {bad.size} rows differ from the kernel's own summation order, first row {bad[0]} ({kinds[plan][bad[0]]})"
            assert np.array_equal(_spmv(A, x, alpha, beta, y0), y), f"{plan}: a second call gives other bits"
        if plan != "arrays":
            B = _handle(monkeypatch, m, plan, no_nt=True)
            assert np.array_equal(_spmv(B, x), first[plan]), f"{plan}: the plain-load kernel gives other bits than the nontemporal one"
    assert np.array_equal(first["arrays"], first["host"])
    same = (kinds["host"] == kinds["device"]) & (np.all(blocks["host"] == blocks["device"], axis=1) | (kinds["host"] == "lane"))
    assert same.any() or m.rows == 0
    assert np.array_equal(first["host"][same], first["device"][same]), "host-built and device-built plan differ on rows they reduce alike"


def _picks(m, model, which):
    """One non-empty row per block — its first or last by turns (which 0), its middle one (which 1) — and one long row."""
    lens = np.diff(m.rowptr)
    rows = []
    for i, (r0, n, _) in enumerate(model.blocks):
        ne = r0 + np.flatnonzero(lens[r0:r0 + n])
        if ne.size:
            rows.append(int(ne[ne.size // 2] if which else ne[0 if i % 2 else -1]))
    if model.long_rows:
        rows.append(model.long_rows[-1 if which else 0])
    return rows


@pytest.mark.parametrize("name", sc.NAMES)
def test_nan_stays_in_the_rows_that_reference_it(oracle, monkeypatch, name):
    m = sc.build(name)
    _, want, asum = _reference(oracle, name)
    for plan in ("host", "device"):
        A = _handle(monkeypatch, m, plan)
        model = MODEL[plan](m.rowptr)
        for which in (0, 1):
            picks = _picks(m, model, which)
            x = m.x.copy()
            x[np.array([c for r in picks for c in sc.private_cols(m, r)], np.int64)] = NAN
            y = _spmv(A, torch.from_numpy(x).cuda())
            hit = np.zeros(m.rows, bool)
            hit[np.array(picks, np.int64)] = True
            assert np.array_equal(np.isnan(y), hit), f"{plan} plan: NaN in rows {np.flatnonzero(np.isnan(y) != hit)[:8]} against the picked rows"
            _within(y[~hit], want[1.0, 0.0][~hit], asum[~hit], f"{plan} plan, rows without NaN")


def _semiring_inputs(m, semiring, sparse, rng):
    """Values, x and the y to accumulate into: min-plus in [1, 2] and max-plus in [−2, −1], so that a stray 0.0 or a missing identity wins the
    reduction and shows; or-and with false entries on both sides (sparse: so few true x that long rows come out false too)."""
    nnz = len(m.colids)
    if semiring == "min_plus":
        return rng.uniform(1, 2, nnz), rng.uniform(1, 2, m.cols), rng.uniform(2, 4, m.rows)
    if semiring == "max_plus":
        return rng.uniform(-2, -1, nnz), rng.uniform(-2, -1, m.cols), rng.uniform(-4, -2, m.rows)
    va = np.where(rng.random(nnz) < 0.2, 0.0, rng.uniform(-1, 1, nnz))
    x = np.where(rng.random(m.cols) < (0.0005 if sparse else 0.08), rng.uniform(0.5, 1, m.cols), 0.0)
    return va, x, np.where(rng.random(m.rows) < 0.7, 0.0, 5.0)


@pytest.mark.parametrize("name", sc.SEMIRING_NAMES)
def test_semirings_equal_the_reference(monkeypatch, name):
    m = sc.build(name)
    rng = np.random.default_rng(5)
    for semiring, sparse in (("min_plus", False), ("max_plus", False), ("or_and", False), ("or_and", True)):
        va, x, y0 = _semiring_inputs(m, semiring, sparse, rng)
        xd = torch.from_numpy(x).cuda()
        for plan, no_nt in (("host", False), ("host", True), ("device", False)):
            A = _handle(monkeypatch, m, plan, values=va, no_nt=no_nt)
            for accumulate in (False, True):
                yd = torch.from_numpy(y0.copy()).cuda() if accumulate else torch.full((m.rows,), NAN, dtype=torch.float64, device="cuda")
                out = A.spmv_semiring(xd, yd, semiring=semiring, accumulate=accumulate).cpu().numpy()
                expect = ref.spmv(m.rowptr, m.colids, va, x, semiring, y0 if accumulate else None)
                bad = np.flatnonzero((out + 0.0) != (expect + 0.0))
                assert bad.size == 0, (f"{semiring} accumulate={accumulate} {plan} plan no_nt={no_nt}: {bad.size} rows differ, first {bad[0]}: "
                                       f"{out[bad[0]]!r} vs {expect[bad[0]]!r} (row length {m.rowptr[bad[0] + 1] - m.rowptr[bad[0]]})")
                assert ref.same_values(out, expect)


# ------------------------------------------------------------------------------------------------ SpMM on the same plans
def _device_block(M, col_major, ld, fill):
    """A strided device view of the host block M (r × k) inside a larger buffer filled with `fill`, leading dimension ld."""
    r, k = M.shape
    extent = (k - 1) * ld + r if col_major else (r - 1) * ld + k
    buf = torch.full((extent + 3,), fill, dtype=torch.float64, device="cuda")
    view = torch.as_strided(buf, (r, k), (1, ld) if col_major else (ld, 1), 0)
    view.copy_(torch.from_numpy(np.ascontiguousarray(M)).cuda())
    return buf, view


def _layouts(k, rows, cols):
    """(name, column-major, ldx, ldy): row-major with an even ld (16-byte pairs from k = 2 on; k = 1 gets ld 2, so that it runs spmm_csr_kernel<1, 1>
    and not g4s_spmv), row-major with an odd ld > k (8-byte accesses), column-major with padded columns."""
    even = k + 1 if k % 2 else k + 2
    odd = k + 1 if k % 2 == 0 else k + 2
    return (("aligned", False, even, even), ("odd_ld", False, odd, odd), ("col_major", True, cols + 3, rows + 3))


@pytest.mark.parametrize("k", [1, 2, 3, 32, 33])
@pytest.mark.parametrize("name", sc.SPMM_NAMES)
def test_spmm_on_the_same_plans(oracle, monkeypatch, name, k):
    m = sc.build(name)
    rng = np.random.default_rng(100 + k)
    X = np.concatenate([m.x[:, None], rng.uniform(-1, 1, (m.cols, k - 1))], axis=1)
    Y0 = rng.uniform(-1, 1, (m.rows, k))
    want = {ab: np.zeros((m.rows, k)) for ab in ALPHA_BETA}
    asum = np.zeros((m.rows, k))
    for j in range(k):
        xj = np.ascontiguousarray(X[:, j])
        asum[:, j] = oracle.spmv_ld(m.rowptr, m.colids, m.values, xj)[1]
        for a, b in ALPHA_BETA:
            want[a, b][:, j] = oracle.spmv(m.rowptr, m.colids, m.values, xj, None if b == 0.0 else Y0[:, j], a, b)
    assert np.array_equal(want[1.0, 0.0][:, 0], _reference(oracle, name)[1][1.0, 0.0])
    for plan in ("host", "device"):
        A = _handle(monkeypatch, m, plan)
        kinds = sc.row_kinds(m.rowptr, MODEL[plan](m.rowptr))
        for layout, cm, ldx, ldy in _layouts(k, m.rows, m.cols):
            assert (ldx % 2 == 0) == (layout == "aligned") or cm
            # SpMM sums every unchunked row left to right, whatever the SpMV does — except that one unit-stride vector IS g4s_spmv (include/g4s.h)
            serial = kinds == "lane" if k == 1 and cm else kinds != "chunked"
            _, xd = _device_block(X, cm, ldx, NAN)
            for alpha, beta in ALPHA_BETA:
                ybuf, yd = _device_block(Y0 if beta != 0.0 else np.full((m.rows, k), NAN), cm, ldy, -7.25)
                before = ybuf.clone()
                A.spmm(xd, yd, alpha, beta)
                got = yd.cpu().numpy()
                what = f"{plan} plan, {layout}, alpha {alpha}, beta {beta}"
                scale = abs(alpha) * asum + abs(beta) * np.abs(Y0) * (beta != 0.0)
                assert not np.isnan(got).any(), what
                _within(got.ravel(), want[alpha, beta].ravel(), scale.ravel(), what)
                assert np.array_equal(got[serial], want[alpha, beta][serial]), f"{what}: unchunked rows differ from the oracle's bits"
                pad = torch.ones_like(ybuf, dtype=torch.bool)
                torch.as_strided(pad, yd.shape, yd.stride(), 0).fill_(False)
                assert torch.equal(ybuf[pad], before[pad]), f"{what}: padding of Y was touched"
                ybuf.copy_(before)
                A.spmm(xd, yd, alpha, beta)
                assert np.array_equal(yd.cpu().numpy(), got), f"{what}: a second call gives other bits"
