"""GPU parity of the blocked SpMV path's band layout: the band width W a plan takes from the device (20 448 columns / rows where a workgroup may have
160 KiB of LDS, 16 384 otherwise or with G4S_PB_BAND=16384), the micro-run heads carried in bit 15 of the local columns, and pads that read a zero
word in LDS instead of x. Every case runs at both band widths and compares with the oracle at the SpMV tolerance (1e-10 of sum |a_ik x_k|)."""
import numpy as np
import pytest
import torch

from tests.helpers import power_law_csr

pytestmark = pytest.mark.gpu
TOL = 1e-10
WIDE, NARROW = 20448, 16384


@pytest.fixture(params=["device", "16384"])
def band(request, monkeypatch, capfd):
    """The band width the plans of a test are built with; the plan's debug line (G4S_DEBUG) must name it."""
    monkeypatch.setenv("G4S_DEBUG", "1")
    if request.param == "16384":
        monkeypatch.setenv("G4S_PB_BAND", "16384")
    else:
        monkeypatch.delenv("G4S_PB_BAND", raising=False)
    want = NARROW if request.param == "16384" else WIDE       # the MI355X grants 160 KiB of LDS to one workgroup
    yield want
    err = capfd.readouterr().err
    assert f"blocked SpMV plan: band {want}," in err, err[-2000:]


def _blocked(rp, ci, va, rows, cols, updatable=False):
    from g4s_amd import capi, host
    flags = capi.SPMV_BLOCKED | (capi.SPMV_UPDATABLE if updatable else 0)
    A = host.CSR.from_host(rp, ci, va, rows, cols, spmv_flags=flags)
    assert A.info()["spmv_path"] == 1, A.info()
    return A


def _check(oracle, A, rp, ci, va, x, alpha=1.0, beta=0.0, y0=None):
    xd = torch.from_numpy(x).cuda()
    yd = None if y0 is None else torch.from_numpy(y0.copy()).cuda()
    y = A.spmv(xd, yd, alpha, beta).cpu().numpy()
    want = oracle.spmv(rp, ci, va, x, y0, alpha, beta)
    _, asum = oracle.spmv_ld(rp, ci, va, np.where(np.isfinite(x), x, 0.0))
    scale = abs(alpha) * asum + (abs(beta) * np.abs(y0) if y0 is not None else 0.0)
    assert np.array_equal(np.isnan(y), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(y[~fin], want[~fin]) or np.all(np.isnan(want[~fin]))
    err = np.abs(y[fin] - want[fin])
    assert np.all(err <= TOL * scale[fin] + 1e-300), f"max rel err {np.max(err / (scale[fin] + 1e-300))}"
    return y


@pytest.mark.parametrize("rows,cols", [(WIDE - 1, 2 * WIDE + 1), (WIDE + 1, 3 * WIDE - 1), (2 * NARROW - 1, NARROW + 1), (2 * NARROW + 1, 3 * NARROW - 1),
                                       (3 * WIDE, 3 * WIDE)])
def test_shapes_around_band_multiples(oracle, band, rows, cols):
    rp, ci, va = power_law_csr(rows, cols, rows + cols, 3000)
    # the last column and the last row of the matrix are populated: the last band's edge is read and written
    ci = ci.copy()
    if rp[-1] > rp[-2]:
        ci[rp[-1] - 1] = cols - 1
    A = _blocked(rp, ci, va, rows, cols)
    x = np.random.default_rng(1).uniform(-1, 1, cols)
    _check(oracle, A, rp, ci, va, x)


def _hot_matrix(rows, cols, seed, popular_n):
    """Rows of up to 12 entries, 60 % of them in a set of popular columns scattered over the natural bands, and one hub row."""
    rng = np.random.default_rng(seed)
    popular = rng.choice(cols, popular_n, replace=False)
    lens = rng.integers(0, 12, rows)
    lens[7] = 30000
    k = int(lens.sum())
    ci = np.where(rng.random(k) < 0.6, popular[rng.integers(0, popular_n, k)], rng.integers(0, cols, k)).astype(np.int64)
    row = np.repeat(np.arange(rows), lens)
    key = np.unique(row * cols + ci)                                 # sorted, duplicates merged
    row, ci = key // cols, key % cols
    rp = np.zeros(rows + 1, np.int64)
    np.add.at(rp, row + 1, 1)
    return np.cumsum(rp).astype(np.int32), ci.astype(np.int32), rng.uniform(-1, 1, len(ci))


@pytest.mark.parametrize("hot", ["0", "max"])
def test_zero_and_maximum_hot_bands(oracle, band, monkeypatch, hot):
    # 64 hot bands (kMaxHotBands) need at least 128 bands of columns
    cols = 130 * band if hot == "max" else 200000
    monkeypatch.setenv("G4S_PB_HOT_BANDS", "0" if hot == "0" else "64")
    rp, ci, va = _hot_matrix(60000, cols, 13, 64 * band + 1000 if hot == "max" else 3000)
    A = _blocked(rp, ci, va, 60000, cols)
    x = np.random.default_rng(2).uniform(-1, 1, cols)
    _check(oracle, A, rp, ci, va, x)


def test_runs_across_windows_and_cells(oracle, band):
    # row 3 holds every column of the first two bands and a stretch of the third: its run in one cell spans hundreds of 32-entry windows and goes on
    # in the next cell; rows 4–40 hold runs of 1–37 consecutive columns that start at every offset of a window
    rows, cols = 3 * band + 5, 3 * band + 7
    rng = np.random.default_rng(3)
    per_row = [np.array([], np.int64)] * rows
    per_row[3] = np.arange(0, 2 * band + 300)
    for r in range(4, 41):
        s = int(rng.integers(0, cols - 40))
        per_row[r] = np.arange(s, s + r - 3)
    per_row[rows - 1] = np.array([0, band - 1, band, cols - 1])
    for r in range(41, rows - 1, 7):
        per_row[r] = np.unique(rng.integers(0, cols, 5))
    lens = np.array([len(c) for c in per_row])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(per_row).astype(np.int32)
    va = rng.uniform(-1, 1, len(ci))
    A = _blocked(rp, ci, va, rows, cols)
    _check(oracle, A, rp, ci, va, rng.uniform(-1, 1, cols))


def test_pads_never_read_x(oracle, band):
    # Inf and NaN in every column without a nonzero and at the band edges a pad's local column could alias (0, W - 1, W): the products of pads read
    # the LDS zero word, so the rows that touch none of these columns stay finite
    rows, half = 50000, 2 * band + 6
    rp, ci, va = power_law_csr(rows, half, 29, 4000)
    ci, cols = 2 * ci, 2 * half                                      # every odd column is empty
    x = np.random.default_rng(4).uniform(-1, 1, cols)
    empty = np.setdiff1d(np.arange(cols), ci)
    assert len(empty) >= half
    x[empty] = np.where(np.arange(len(empty)) % 2 == 0, np.nan, np.inf)
    edges = np.array([c for c in (0, band - 1, band, 2 * band - 1, 2 * band, cols - 1) if c in set(empty.tolist())])
    x[edges] = np.nan
    A = _blocked(rp, ci, va, rows, cols)
    y = _check(oracle, A, rp, ci, va, x)
    assert np.all(np.isfinite(y))


def test_beta_and_split_row_bands(oracle, band, monkeypatch):
    # small consumer items: every row band with more than 2 048 micro-runs is split over several workgroups that add into y (pre-scaled by beta)
    monkeypatch.setenv("G4S_PB_CCHUNK", "2048")
    rows, cols = 2 * band + 100, 3 * band
    rp, ci, va = power_law_csr(rows, cols, 31, 6000)
    A = _blocked(rp, ci, va, rows, cols)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, cols)
    y0 = rng.uniform(-1, 1, rows)
    _check(oracle, A, rp, ci, va, x, alpha=-1.5, beta=0.75, y0=y0)
    _check(oracle, A, rp, ci, va, x, alpha=2.0, beta=0.0, y0=y0)


def test_update_values_after_create(oracle, band):
    rows, cols = 70000, 70000
    rp, ci, va = power_law_csr(rows, cols, 37, 9000)
    A = _blocked(rp, ci, va, rows, cols, updatable=True)
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, cols)
    _check(oracle, A, rp, ci, va, x)
    vnew = rng.uniform(-2, 2, len(ci))
    A.update_values(torch.from_numpy(vnew).cuda())
    _check(oracle, A, rp, ci, vnew, x)
