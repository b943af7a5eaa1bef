"""g4s_spmm / g4s_spmm_csr_i32_f64 argument rules that hold without a GPU: every check runs before any HIP call, so a bad argument is
G4S_ERR_INVALID with its own message even on a box without a device (a HIP call there would fail with G4S_ERR_HIP instead)."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    from g4s_amd import capi
    return capi, capi.load()


def _oneshot(rows, cols, k, ldx, ldy, flags=0, X=None, Y=None):
    capi, lib = _lib()
    rp = np.zeros(rows + 1, dtype=np.int32)
    ci = np.zeros(1, dtype=np.int32)
    va = np.zeros(1)
    X = np.zeros(max(1, cols * max(ldx, 1) * max(k, 1))) if X is None else X
    Y = np.zeros(max(1, rows * max(ldy, 1) * max(k, 1))) if Y is None else Y
    st = lib.g4s_spmm_csr_i32_f64(rows, cols, k, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, X.ctypes.data, ldx, Y.ctypes.data, ldy, 1.0, 0.0,
                                  flags)
    return st, lib.g4s_last_error().decode()


def test_spmm_null_handle_is_invalid():
    capi, lib = _lib()
    x = np.zeros(8)
    y = np.zeros(8)
    assert lib.g4s_spmm(None, 2, x.ctypes.data, 2, y.ctypes.data, 2, 1.0, 0.0, 0, None) == capi.ERR_INVALID
    assert "NULL handle" in lib.g4s_last_error().decode()
    assert lib.g4s_csr_spmm_reserve(None, 4) == capi.ERR_INVALID


def test_spmm_negative_k_is_invalid():
    capi, _ = _lib()
    st, msg = _oneshot(4, 4, -1, 4, 4)
    assert st == capi.ERR_INVALID and "k is negative" in msg


@pytest.mark.parametrize("ldx,ldy,needle", [(3, 4, "ldx >= k"), (4, 3, "ldy >= k")])
def test_spmm_row_major_leading_dimension_below_k_is_invalid(ldx, ldy, needle):
    capi, _ = _lib()
    st, msg = _oneshot(5, 6, 4, ldx, ldy)
    assert st == capi.ERR_INVALID and needle in msg


@pytest.mark.parametrize("ldx,ldy,needle", [(5, 5, "ldx >= cols"), (6, 4, "ldy >= rows")])
def test_spmm_column_major_leading_dimension_below_the_extent_is_invalid(ldx, ldy, needle):
    capi, _ = _lib()
    st, msg = _oneshot(5, 6, 3, ldx, ldy, flags=capi.SPMM_COL_MAJOR)
    assert st == capi.ERR_INVALID and needle in msg
    # the same leading dimensions are fine row-major for k = 3 — the rule follows the layout (stops at the first HIP call or succeeds)
    st2, msg2 = _oneshot(5, 6, 3, ldx, ldy)
    assert st2 != capi.ERR_INVALID or "ld" not in msg2


def test_spmm_overlapping_blocks_are_invalid():
    capi, _ = _lib()
    buf = np.zeros(64)
    st, msg = _oneshot(4, 4, 2, 2, 2, X=buf, Y=buf)
    assert st == capi.ERR_INVALID and "overlap" in msg
    base = buf.ctypes.data
    _, lib = _lib()
    rp = np.zeros(5, dtype=np.int32)
    # Y starts inside X's block (X: 4 rows of ld 4 → 16 doubles)
    st = lib.g4s_spmm_csr_i32_f64(4, 4, 2, rp.ctypes.data, None, None, C.c_void_p(base), 4, C.c_void_p(base + 8 * 10), 2, 1.0, 0.0, 0)
    assert st == capi.ERR_INVALID and "overlap" in lib.g4s_last_error().decode()


@pytest.mark.parametrize("col_major", [False, True])
def test_spmm_leading_dimension_beyond_the_address_space_is_invalid(col_major):
    """A huge ld would wrap the end address of the block (and the overlap check with it): refused before any address is formed."""
    capi, lib = _lib()
    buf = np.zeros(64)
    rp = np.zeros(5, dtype=np.int32)
    flags = capi.SPMM_COL_MAJOR if col_major else 0
    for ldx, ldy in ((1 << 62, 4), (4, 1 << 62)):
        st = lib.g4s_spmm_csr_i32_f64(4, 4, 3, rp.ctypes.data, None, None, C.c_void_p(buf.ctypes.data), ldx, C.c_void_p(buf.ctypes.data + 8 * 32), ldy,
                                      1.0, 0.0, flags)
        assert st == capi.ERR_INVALID and "address space" in lib.g4s_last_error().decode()


def test_spmm_misaligned_pointer_is_invalid():
    capi, lib = _lib()
    buf = np.zeros(64)
    rp = np.zeros(3, dtype=np.int32)
    st = lib.g4s_spmm_csr_i32_f64(2, 2, 2, rp.ctypes.data, None, None, C.c_void_p(buf.ctypes.data + 4), 2, C.c_void_p(buf.ctypes.data + 8 * 32), 2,
                                  1.0, 0.0, 0)
    assert st == capi.ERR_INVALID and "aligned" in lib.g4s_last_error().decode()


def test_spmm_empty_cases_need_no_device():
    capi, _ = _lib()
    assert _oneshot(4, 4, 0, 0, 0)[0] == capi.OK          # k == 0: nothing to do, no HIP call
    assert _oneshot(0, 4, 3, 3, 3)[0] == capi.OK          # rows == 0


def test_host_spmm_refuses_cpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from g4s_amd import host
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        host.spmm(None, torch.zeros(4, 2, dtype=torch.float64))
