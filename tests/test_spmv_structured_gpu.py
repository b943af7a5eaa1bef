"""The two bit-identical SpMV paths — index-free diagonal (spmv_path 3, csrc/spmv_dia.hip) and block-row (spmv_path 4, csrc/spmv_bcsr.hip) — at every
kernel instantiation and on both sides of every selection threshold, on the cases of tests/structured_cases.py (whose claimed properties
tests/test_structured_cases_cpu.py proves).

Every product on path 3 or 4 must equal the oracle's BIT FOR BIT: one lane per row adds the row's products in stored order, multiply then add, as the
oracle does. Every case that must fall back to the row-streaming kernel (path 0) is held to the project's 1e-10·Σ|terms|. The path a handle takes must
be the one structured_cases.expected_path predicts from the documented selection rules."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spmv_semiring_ref as sref
from tests import structured_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-10
PAIRS = ((1.0, 0.0), (-0.5, 2.0))
PLAIN_LOADS = 4                                                        # G4S_SPMV_NO_NT
FORCE_STREAM = 16                                                      # G4S_SPMV_STREAM


def _handle(m, flags=0, values=None):
    from g4s_amd import host
    return host.CSR.from_host(m.rowptr, m.colids, m.values if values is None else values, m.rows, m.cols, spmv_flags=flags)


def _y_view(rows, misaligned):
    """A y of `rows` doubles that is 16-byte aligned, or 8 bytes past that (the diagonal path then takes its one-row kernel for every row)."""
    buf = torch.zeros(rows + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    y = buf[1:rows + 1] if misaligned else buf[:rows]
    assert y.data_ptr() % 16 == (8 if misaligned else 0)
    return y


def _product(A, x, alpha=1.0, beta=0.0, y0=None, misaligned=False):
    y = _y_view(A.rows, misaligned)
    y.copy_(torch.from_numpy(y0) if y0 is not None else torch.full((A.rows,), float("nan"), dtype=torch.float64))   # beta == 0 never reads y
    return A.spmv(torch.from_numpy(x).cuda(), y, alpha, beta).cpu().numpy()


def _check(oracle, A, m, x, alpha=1.0, beta=0.0, y0=None, exact=False, misaligned=False, values=None):
    """The comparison of tests/test_spmv_gpu.py::_check, restated: within 1e-10·Σ|terms| always, the oracle's bits where the path promises them."""
    va = m.values if values is None else values
    y = _product(A, x, alpha, beta, y0, misaligned)
    want = oracle.spmv(m.rowptr, m.colids, va, x, y0, alpha, beta)
    _, asum = oracle.spmv_ld(m.rowptr, m.colids, va, x)
    scale = abs(alpha) * asum + (abs(beta) * np.abs(y0) if y0 is not None else 0.0)
    err = np.abs(y - want)
    assert np.all(err <= TOL * scale + 1e-300), f"max rel err {np.max(err / (scale + 1e-300))}"
    if exact:
        bad = np.flatnonzero(y != want)
        assert bad.size == 0, f"{bad.size} rows differ from the oracle's bits, first {bad[0]}: {y[bad[0]]!r} vs {want[bad[0]]!r}"
    return y


def _check_both_pairs(oracle, A, m, seed, exact, alignments=(False,), values=None):
    rng = np.random.default_rng(seed)
    x, y0 = rng.uniform(-1, 1, m.cols), rng.uniform(-1, 1, m.rows)
    for alpha, beta in PAIRS:
        ys = [_check(oracle, A, m, x, alpha, beta, y0 if beta else None, exact, mis, values) for mis in alignments]
        assert all(np.array_equal(ys[0], y) for y in ys[1:]), "an 8-byte-aligned y changes the bits"


def _path(A):
    return A.info()["spmv_path"]


def _check_forced_stream(oracle, m, seed):
    """G4S_SPMV_STREAM keeps a matrix that has the structure on the row-streaming kernel, as expected_path(force_stream=True) says."""
    assert sc.expected_path(m.rows, m.cols, m.rowptr, m.colids, force_stream=True) == sc.PATH_STREAM
    S = _handle(m, flags=FORCE_STREAM)
    assert _path(S) == sc.PATH_STREAM
    _check_both_pairs(oracle, S, m, seed, exact=False)


def _assert_predicted(A, m, name):
    want = sc.case(name).path
    assert sc.expected_path(m.rows, m.cols, m.rowptr, m.colids) == want
    assert _path(A) == want, (name, A.info())
    return want


# ================================================================================================ diagonal path
@pytest.mark.parametrize("nd", sc.INSTANTIATION_ND)
def test_diagonal_instantiations(oracle, nd):
    """nd = 1, 8 | 9, 16 | 17, 32: both sides of the ND = 8 / 16 / 32 templates. An even and an odd row count (the odd last row goes to the one-row
    kernel), y 16-byte aligned (two rows per lane up to 16 diagonals) and 8 bytes off (spmv_dia_kernel<ND> for every row): equal bits, the oracle's."""
    for rows in (4098, 4097):
        name = f"inst_nd{nd}_rows{rows}"
        m = sc.build(name)
        A = _handle(m)
        assert _assert_predicted(A, m, name) == sc.PATH_DIAGONAL
        _check_both_pairs(oracle, A, m, nd, exact=True, alignments=(False, True))
        P = _handle(m, flags=PLAIN_LOADS)                              # the plain-load instantiations: the same arithmetic
        assert _path(P) == sc.PATH_DIAGONAL
        _check_both_pairs(oracle, P, m, nd, exact=True, alignments=(False, True))
    _check_forced_stream(oracle, m, nd)


def test_diagonal_33_offsets_stay_on_the_csr_kernel(oracle):
    m = sc.build("inst_nd33_rows4098")
    A = _handle(m)
    assert _assert_predicted(A, m, "inst_nd33_rows4098") == sc.PATH_STREAM
    _check_both_pairs(oracle, A, m, 33, exact=False)


@pytest.mark.parametrize("name", [c.name for c in sc.dia_cases() if c.name.startswith("geometry_")])
def test_diagonal_launch_geometry(oracle, name):
    """2, 7, 8 and 9 workgroups of the two-row kernel (grids of 8, 8, 8 and 16: the round-up to the XCD count leaves workgroups without rows), and row
    counts one past and one short of a multiple of 64 (the leading dimension of the diagonals is rounded up to it)."""
    m = sc.build(name)
    A = _handle(m)
    assert _assert_predicted(A, m, name) == sc.PATH_DIAGONAL
    _check_both_pairs(oracle, A, m, 3, exact=True, alignments=(False, True))


@pytest.mark.parametrize("name", ["rect_tall_trailing_empty", "rect_wide", "interior_empty_run", "holes_fill_0.9"])
def test_diagonal_rectangular_shapes_and_empty_rows(oracle, name):
    m = sc.build(name)
    A = _handle(m)
    assert _assert_predicted(A, m, name) == sc.PATH_DIAGONAL
    _check_both_pairs(oracle, A, m, 4, exact=True, alignments=(False, True))
    empty = np.diff(m.rowptr) == 0
    if empty.any():                                                    # an empty row: exactly beta·y
        y0 = np.random.default_rng(5).uniform(-1, 1, m.rows)
        y = _product(A, np.ones(m.cols), -0.5, 2.0, y0)
        assert np.array_equal(y[empty], 2.0 * y0[empty])


@pytest.mark.parametrize("name", ["inst_nd9_rows4097", "inst_nd8_rows4098", "inst_nd32_rows4097"])
def test_diagonal_nonfinite_x_reaches_only_the_rows_that_reference_it(oracle, name):
    """Absent entries of boundary rows read the clamped positions x[0] and x[cols − 1]: NaN there must show only in rows that hold those columns."""
    m = sc.build(name)
    A = _handle(m)
    assert _path(A) == sc.PATH_DIAGONAL
    x = np.random.default_rng(6).uniform(-1, 1, m.cols)
    x[0] = x[m.cols - 1] = np.nan
    want = oracle.spmv(m.rowptr, m.colids, m.values, x)
    touched = np.zeros(m.rows, bool)
    touched[sc.row_of(m.rowptr)[(m.colids == 0) | (m.colids == m.cols - 1)]] = True
    assert np.array_equal(np.isnan(want), touched) and 0 < touched.sum() < m.rows // 50
    for misaligned in (False, True):
        y = _product(A, x, misaligned=misaligned)
        assert np.array_equal(np.isnan(y), touched)
        assert np.array_equal(y[~touched], want[~touched])


@pytest.mark.parametrize("name", ["rows_1023", "rows_1024", "nnz_4095", "nnz_4096", "fill_just_above", "fill_just_below", "swap_in_unsampled_row",
                                  "duplicate_in_unsampled_row"])
def test_diagonal_selection_thresholds(oracle, name):
    m = sc.build(name)
    A = _handle(m)
    path = _assert_predicted(A, m, name)
    _check_both_pairs(oracle, A, m, 7, exact=path == sc.PATH_DIAGONAL, alignments=(False, True) if path == sc.PATH_DIAGONAL else (False,))


def _capi_product(lib, h, x, rows):
    from g4s_amd import capi
    y = torch.full((rows,), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(lib.g4s_spmv(h, x.data_ptr(), y.data_ptr(), 1.0, 0.0, None))
    return y.cpu().numpy()


def _capi_path(lib, h):
    from g4s_amd import capi
    inf = capi.CsrInfo()
    capi.check(lib.g4s_csr_get_info(h, C.byref(inf)))
    return inf.spmv_path


def _refresh_every_form(oracle, m, path, seed):
    """g4s_csr_update_values in the forms of tests/test_update_values_gpu.py — a handle that owns its copy (new values from a host array, from a device
    array), a handle that borrows (a new device array, then that array rewritten in place) — each time the bits of a handle
    created from the new values, which are the oracle's."""
    from g4s_amd import capi
    lib = capi.load()
    rng = np.random.default_rng(seed)
    nnz = len(m.colids)
    x = rng.uniform(-1, 1, m.cols)
    xd = torch.from_numpy(x).cuda()

    def expect(v):
        F = _handle(m, values=v)
        assert _path(F) == path
        fresh = F.spmv(xd).cpu().numpy()
        F.close()
        want = oracle.spmv(m.rowptr, m.colids, v, x)
        assert np.array_equal(fresh, want)
        return want

    h = C.c_void_p()
    capi.check(lib.g4s_csr_create(C.byref(h), m.rows, m.cols, nnz, m.rowptr.ctypes.data, m.colids.ctypes.data, m.values.ctypes.data, capi.HOST_POINTERS))
    assert _capi_path(lib, h) == path
    _capi_product(lib, h, xd, m.rows)                                  # a product with the old values first
    v1 = rng.uniform(-1, 1, nnz)
    capi.check(lib.g4s_csr_update_values(h, v1.ctypes.data, capi.HOST_POINTERS, None))
    assert np.array_equal(_capi_product(lib, h, xd, m.rows), expect(v1)), "owned copy, host array"
    v2 = rng.uniform(-1, 1, nnz) + 1.0
    v2d = torch.from_numpy(v2).cuda()
    capi.check(lib.g4s_csr_update_values(h, v2d.data_ptr(), capi.DEVICE_POINTERS, None))
    assert np.array_equal(_capi_product(lib, h, xd, m.rows), expect(v2)), "owned copy, device array"
    lib.g4s_csr_destroy(h)

    rpd, cid, vad = torch.from_numpy(m.rowptr.copy()).cuda(), torch.from_numpy(m.colids.copy()).cuda(), torch.from_numpy(m.values.copy()).cuda()
    torch.cuda.synchronize()
    capi.check(lib.g4s_csr_create(C.byref(h), m.rows, m.cols, nnz, rpd.data_ptr(), cid.data_ptr(), vad.data_ptr(), capi.DEVICE_POINTERS))
    assert _capi_path(lib, h) == path
    v3 = rng.uniform(-1, 1, nnz) - 1.0
    v3d = torch.empty(nnz, dtype=torch.float64, device="cuda")       # nnz doubles as the issue asks; the allocator rounds up, so a read at values[nnz] would not show here
    v3d.copy_(torch.from_numpy(v3))
    torch.cuda.synchronize()
    capi.check(lib.g4s_csr_update_values(h, v3d.data_ptr(), capi.DEVICE_POINTERS, None))
    assert np.array_equal(_capi_product(lib, h, xd, m.rows), expect(v3)), "borrowed, a new device array"
    v4 = rng.uniform(-1, 1, nnz) * 3.0
    v3d.copy_(torch.from_numpy(v4))
    torch.cuda.synchronize()
    capi.check(lib.g4s_csr_update_values(h, None, capi.DEVICE_POINTERS, None))
    assert np.array_equal(_capi_product(lib, h, xd, m.rows), expect(v4)), "borrowed, rewritten in place"
    assert _capi_path(lib, h) == path
    lib.g4s_csr_destroy(h)


@pytest.mark.parametrize("nd", sc.REFRESH_ND)
def test_diagonal_value_refresh(oracle, nd):
    """dia_refill_kernel<8 / 16 / 32> on masks with missing bits, interior empty rows and trailing empty rows (whose first entry would be entry nnz)."""
    _refresh_every_form(oracle, sc.build(f"refresh_nd{nd}"), sc.PATH_DIAGONAL, nd)


# ---- semirings (the conventions of tests/test_spmv_semiring_gpu.py)
def _semiring_x(semiring, cols, rng):
    x = rng.uniform(-1, 1, cols)
    if semiring == "or_and":
        x[rng.random(cols) < 0.5] = 0.0
    return x


def _semiring_y0(semiring, rows, rng):
    return np.where(rng.random(rows) < 0.7, 0.0, 5.0) if semiring == "or_and" else rng.uniform(-2, 2, rows)


def _check_semirings(A, m, seed, alignments=(False,)):
    rng = np.random.default_rng(seed)
    for semiring in sref.NEW:
        x, y0 = _semiring_x(semiring, m.cols, rng), _semiring_y0(semiring, m.rows, rng)
        xd = torch.from_numpy(x).cuda()
        for accumulate in (False, True):
            want = sref.spmv(m.rowptr, m.colids, m.values, x, semiring, y0 if accumulate else None)
            for misaligned in alignments:
                y = _y_view(m.rows, misaligned)
                y.copy_(torch.from_numpy(y0) if accumulate else torch.full((m.rows,), float("nan"), dtype=torch.float64))
                out = A.spmv_semiring(xd, y, semiring=semiring, accumulate=accumulate).cpu().numpy()
                bad = np.flatnonzero((out + 0.0) != (want + 0.0))
                assert bad.size == 0, f"{semiring} acc={accumulate} misaligned={misaligned}: {bad.size} rows differ, first {bad[0]}: {out[bad[0]]!r} vs {want[bad[0]]!r}"


@pytest.mark.parametrize("nd", [9, 16, 17])
def test_diagonal_semirings(nd):
    for rows in (4098, 4097):
        m = sc.build(f"inst_nd{nd}_rows{rows}")
        A = _handle(m)
        assert _path(A) == sc.PATH_DIAGONAL
        _check_semirings(A, m, nd, alignments=(False, True))


# ================================================================================================ block-row path
@pytest.fixture
def plan_lines(monkeypatch, capfd):
    """The block-row plan lines the library printed (G4S_DEBUG) since the last call: which block size a handle settled on."""
    monkeypatch.setenv("G4S_DEBUG", "1")

    def read():
        return [ln for ln in capfd.readouterr().err.splitlines() if "block-row SpMV plan" in ln]
    return read


def _assert_block(plan_lines, b):
    lines = plan_lines()
    if b:
        assert len(lines) == 1 and f"plan: {b} x {b} blocks" in lines[0], lines
    else:
        assert lines == []


@pytest.mark.parametrize("b", [2, 3, 4])
def test_block_row_structural_edges(oracle, plan_lines, b):
    """Blocks per block-row cycling through 1 … 8 and 0 (every remainder of the four-blocks-at-a-time row sum), 600 empty block-rows in a row (more
    than one work item holds), empty leading and trailing block-rows, one block-row that fills the tile exactly: the oracle's bits, with nontemporal
    and with plain loads. 2×2 and 3×3 matrices run as such; aligned 4×4 blocks pass the 2×2 check, which is tried first, so the 4×4 matrix runs as
    2×2 blocks with twice the block counts (remainders 0 and 2 only, 128 blocks in its fullest block-row); there is no 4×4 instantiation."""
    name = f"main_b{b}"
    m = sc.build(name)
    A = _handle(m)
    assert _assert_predicted(A, m, name) == sc.PATH_BLOCKROW
    _assert_block(plan_lines, sc.case(name).claims["block"])
    _check_both_pairs(oracle, A, m, b, exact=True)
    P = _handle(m, flags=PLAIN_LOADS)
    assert _path(P) == sc.PATH_BLOCKROW
    _check_both_pairs(oracle, P, m, b, exact=True)
    x = torch.from_numpy(np.random.default_rng(b).uniform(-1, 1, m.cols)).cuda()
    assert torch.equal(A.spmv(x), P.spmv(x))
    _check_forced_stream(oracle, m, b)


@pytest.mark.parametrize("name", ["over_b2", "over_b3", "over_b4", "over_b4_and_b2"])
def test_block_row_one_block_past_the_tile(oracle, plan_lines, name):
    """257 2×2 / 114 3×3 blocks in one block-row: the CSR kernel. 65 aligned 4×4 blocks are also 130 aligned 2×2 blocks, which fit the 2×2 tile (256):
    the handle takes the 2×2 form — still path 4, still the oracle's bits; 129 4×4 blocks are past both tiles."""
    m = sc.build(name)
    A = _handle(m)
    path = _assert_predicted(A, m, name)
    _assert_block(plan_lines, sc.case(name).claims["block"])
    _check_both_pairs(oracle, A, m, 8, exact=path == sc.PATH_BLOCKROW)


@pytest.mark.parametrize("name", [c.name for c in sc.block_cases() if c.name.startswith("gate_") or c.name.startswith("rect_")])
def test_block_row_gates(oracle, plan_lines, name):
    m = sc.build(name)
    A = _handle(m)
    path = _assert_predicted(A, m, name)
    _assert_block(plan_lines, sc.case(name).claims["block"])
    assert sc.bcsr_block(m.rows, m.cols, m.rowptr, m.colids) == sc.case(name).claims["block"]
    _check_both_pairs(oracle, A, m, 9, exact=path == sc.PATH_BLOCKROW)


@pytest.mark.parametrize("b", [2, 3, 4])
def test_block_row_value_refresh(oracle, b):
    _refresh_every_form(oracle, sc.build(f"main_b{b}"), sc.PATH_BLOCKROW, 20 + b)


@pytest.mark.parametrize("b", [2, 3, 4])
def test_block_row_semirings(b):
    m = sc.build(f"main_b{b}")
    A = _handle(m)
    assert _path(A) == sc.PATH_BLOCKROW
    _check_semirings(A, m, 30 + b)
