"""The block forms g4s_sptrsv_solve_multi and g4s_ilu0_apply_multi (include/g4s.h), as far as they can be asked without a device: the
symbols, the ctypes table against the header, the flag bit, every refusal of the two entry points — they come before the first HIP call — and the
ValueErrors of g4s_amd.host. tests/test_trsv_multi_gpu.py and tests/test_ilu_multi_gpu.py compare the bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("g4s_sptrsv_solve_multi", "g4s_ilu0_apply_multi")


def test_both_symbols_are_exported():
    from g4s_amd import capi
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY) <= exported


def test_signatures_and_constants_equal_the_header():
    from g4s_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "g4s.h")).read(), flags=re.S)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (G4S_TRSV_(?:COL_MAJOR|RHS_TILE|MAX_RHS))\s+\(?(\d+)u?\)?", header)}
    assert defs == {"G4S_TRSV_COL_MAJOR": capi.TRSV_COL_MAJOR, "G4S_TRSV_RHS_TILE": capi.TRSV_RHS_TILE, "G4S_TRSV_MAX_RHS": capi.TRSV_MAX_RHS}
    assert capi.TRSV_MAX_RHS == 32768 and capi.TRSV_RHS_TILE >= 2                # the k of the GPU tests run from 1 to 2·KT + 3
    ctype = {"g4s_trsv_t": C.c_void_p, "g4s_ilu0_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const double *": C.c_void_p,
             "double *": C.c_void_p, "unsigned": C.c_uint, "void *": C.c_void_p}
    for name in ENTRY:
        m = re.search(r"g4s_status\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        args = []
        for a in m.group(1).split(","):
            t = re.sub(r"\w+$", "", " ".join(a.split())).strip()               # the declaration without the parameter's name
            args.append(ctype[t])
        assert capi.SIGNATURES[name] == (C.c_int, args), (name, args)
        assert getattr(capi.load(), name).argtypes == args
    vp = C.c_void_p
    assert capi.SIGNATURES[ENTRY[0]] == capi.SIGNATURES[ENTRY[1]] == (C.c_int, [vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.c_uint, vp])


def test_the_layout_flag_is_a_bit_of_its_own():
    from g4s_amd import capi
    header = open(os.path.join(ROOT, "include", "g4s.h")).read()
    f = capi.TRSV_COL_MAJOR
    assert f > 0 and f & (f - 1) == 0 and f < 2**32
    others = [capi.DEVICE_POINTERS, capi.SORT_OUTPUT, capi.SPMV_NO_NT, capi.SPMV_BLOCKED, capi.SPMV_STREAM, capi.DIST_LOOPBACK, capi.DIST_ALLGATHER, capi.SPMV_UPDATABLE,
              capi.SPMM_COL_MAJOR, capi.SEMIRING_MASK, capi.SPMV_ACCUMULATE, capi.TRAVERSE_PUSH, capi.TRAVERSE_PULL, capi.TRAVERSE_SYMMETRIC, capi.CC_SYMMETRIC,
              capi.PAGERANK_SYMMETRIC, capi.PAGERANK_WARM_START, capi.BC_ACCUMULATE, capi.COLOR_LARGEST_FIRST, capi.MSF_MAXIMUM,
              capi.TRSV_UPPER, capi.TRSV_UNIT_DIAGONAL, capi.TRSV_NO_CHAINS, capi.ILU0_NO_CHAINS]
    assert all(f & o == 0 for o in others)
    # and every flag the header defines as a plain unsigned literal, whatever call it belongs to
    every = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (G4S_\w+)\s+(\d+)u\b", header)}
    assert len(every) >= 25 and all(f & v == 0 for v in every.values()), [n for n, v in every.items() if f & v]


def _fake_handle(n):
    """Neither entry point reads anything of its handle but n — the first member of g4s_trsv_s and of g4s_ilu0_s — before the last of its refusals,
    and a handle cannot be made without a device: the refusals are asked with a zeroed block that holds n and nothing else. No call below gets past its
    refusal, so nothing else of the block is ever read."""
    buf = (C.c_int32 * 1024)()
    buf[0] = n
    return buf


@pytest.mark.parametrize("name", ENTRY)
def test_c_refusals_come_before_any_hip_call(name):
    from g4s_amd import capi
    lib = capi.load()
    fn = getattr(lib, name)
    n, k = 5, 3
    blk = np.zeros(64, np.float64)
    other = np.zeros(64, np.float64)
    P = lambda a: C.c_void_p(a.ctypes.data)
    buf = _fake_handle(n)
    h = C.cast(buf, C.c_void_p)
    CM = capi.TRSV_COL_MAJOR
    cases = (
        ((None, k, P(blk), k, P(other), k, 0, None), "handle is NULL"),
        ((h, -1, P(blk), k, P(other), k, 0, None), "k is negative or above"),
        ((h, capi.TRSV_MAX_RHS + 1, P(blk), capi.TRSV_MAX_RHS + 1, P(other), capi.TRSV_MAX_RHS + 1, 0, None), "k is negative or above"),
        ((h, k, P(blk), k, P(other), k, 1, None), "flags other than"),                      # G4S_DEVICE_POINTERS is not a flag of this call
        ((h, k, P(blk), k, P(other), k, CM | capi.TRSV_UPPER, None), "flags other than"),
        ((h, k, P(blk), k, P(other), k, CM << 1, None), "flags other than"),
        ((h, k, None, k, P(other), k, 0, None), "is NULL"),
        ((h, k, P(blk), k, None, k, 0, None), "is NULL"),
        ((h, k, P(blk), k - 1, P(other), k, 0, None), "leading dimension"),                 # row-major: ld >= k
        ((h, k, P(blk), k, P(other), k - 1, 0, None), "leading dimension"),
        ((h, k, P(blk), n - 1, P(other), n, CM, None), "leading dimension"),                # column-major: ld >= n, k is not enough
        ((h, k, P(blk), n, P(other), k, CM, None), "leading dimension"),
        ((h, k, P(blk), k, P(blk), k + 1, 0, None), "another leading dimension"),           # the same pointer, different leading dimensions
        ((h, k, P(blk), n + 1, P(blk), n, CM, None), "another leading dimension"),
    )
    for args, text in cases:
        assert fn(*args) == capi.ERR_INVALID and text in lib.g4s_last_error().decode() and name in lib.g4s_last_error().decode(), (text, lib.g4s_last_error())
    assert not blk.any() and not other.any()
    # k == 0 and n == 0 are valid and enqueue nothing: no device is there to enqueue on, NULL blocks and any leading dimension pass
    assert fn(h, 0, None, 0, None, 0, 0, None) == capi.OK
    assert fn(h, 0, None, 0, None, 0, CM, None) == capi.OK
    empty = C.cast(_fake_handle(0), C.c_void_p)
    assert fn(empty, k, None, 0, None, 0, 0, None) == capi.OK
    assert fn(empty, capi.TRSV_MAX_RHS, None, 0, None, 0, CM, None) == capi.OK
    assert fn(empty, capi.TRSV_MAX_RHS + 1, None, 0, None, 0, 0, None) == capi.ERR_INVALID   # the cap on k holds whatever n is
    assert list(buf) == [n] + [0] * 1023


def test_python_refusals_need_no_device():
    import torch
    from g4s_amd import capi, host
    n = 6
    plan = host.TriangularPlan(C.c_void_p(1), n, n, capi.TRSVInfo())        # a handle that no refused call reaches
    M = host.ILU0(C.c_void_p(1), n, n, capi.ILU0Info())
    try:
        z = lambda *shape, **kw: torch.zeros(*shape, dtype=kw.get("dtype", torch.float64))
        wide = z(1, capi.TRSV_MAX_RHS + 1).expand(n, capi.TRSV_MAX_RHS + 1)   # n × (cap + 1) without the memory
        for call in (plan.solve, M.apply):
            for b, out, text in ((z(n + 1, 3), None, "must be a float64 tensor"),                  # a wrong shape
                                 (z(n, 3, dtype=torch.float32), None, "must be a float64 tensor"),   # a wrong dtype
                                 (z(n, 3, 2), None, "entries"),                                      # three dimensions: neither form
                                 (z(n, 3), z(n, 4), "out must be"),
                                 (z(n, 3), z(n, 3, dtype=torch.float32), "out must be"),
                                 (z(n, 3), z(n), "out must be"),
                                 (z(n, 3), z(3, n).t(), "both be row-major"),                        # mixed layouts
                                 (z(3, n).t(), z(n, 3), "both be row-major"),
                                 (z(n, 6)[:, ::2], None, "both be row-major"),                       # strides (6, 2): neither layout
                                 (z(2 * n, 6)[::2, ::2], None, "both be row-major"),
                                 (z(n, 3), z(n, 6)[:, ::2], "both be row-major"),
                                 (wide, None, "more than")):
                with pytest.raises(ValueError, match=text):
                    call(b, out)
        rp, ci, va = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)
        with pytest.raises(ValueError, match=f"b must have {n} rows"):
            host.spsolve_triangular((rp, ci, va), np.ones((n + 1, 2)))
        with pytest.raises(ValueError, match="columns"):
            host.spsolve_triangular((rp, ci, va), np.broadcast_to(np.ones(1), (n, capi.TRSV_MAX_RHS + 1)))
        if not torch.cuda.is_available():                                  # a well-formed block gets as far as the device, and no further
            for call in (plan.solve, M.apply):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call(z(n, 3))
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call(z(3, n).t(), z(5, n)[:3].t())                       # column-major with ld = n, both
    finally:
        plan._handle = M._handle = None                                     # nothing to release


def test_gauss_seidel_refuses_blocks_that_do_not_match():
    import torch
    from g4s_amd import host
    n = 4
    A = host.CSR.__new__(host.CSR)                                          # what the checks read of a CSR; nothing gets as far as its arrays
    A.rows = A.cols = n
    A._handle = None
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    for b, x in ((z(n, 3), z(n, 2)), (z(n), z(n, 2)), (z(n, 2), z(n)), (z(n + 1, 2), z(n + 1, 2)), (z(n, 4)[:, ::2], z(n, 4)[:, ::2])):
        with pytest.raises(ValueError):
            host.gauss_seidel(A, b, x)


def test_trsm_example_compiles(tmp_path):
    _build_example("trsm.cpp", str(tmp_path / "trsm"))
