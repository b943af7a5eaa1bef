"""g4s_pagerank on the cases of tests/iteration_cases.py: the average degrees on both sides of the 4/16/64 lanes-per-row rule, rows of 4095, 4096, 4097
and 8195 entries on both sides of kLongRow — several in one wave, in two waves of a window, as the last vertex, one of stored zeros —, n just past every
capped grid of the strength pass, and the epilogue under its cap of 512 workgroups (n = 2^20 + 3·2048 + 5: the full s_part[2][512], nine ragged trips).
Every case goes through _run_fixed / _compare of tests/test_pagerank_gpu.py: the longdouble reference after the same iterations, the L1 error and
|Σr − 1| under γ / (1 − d), the residual within twice that, and the dangling count — the sharpest check of the strength kernels' two counters — exactly.
γ takes the depth of the mass and residual sums read off the code (iteration_cases.sum_depth), never a number the device returned. The product runs on
the streaming path (SPMV_STREAM), where the header of pagerank.hip promises the same bits on every run: each case runs twice and must repeat itself.
tests/test_iteration_cases_cpu.py proves that the cases stand on their limits for the CU count of the device."""
import functools

import numpy as np
import pytest
import torch

from tests import iteration_cases as ic
from tests import pagerank_ref
from tests.test_pagerank_gpu import _dev, _from_arrays, _host, _run_fixed

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _arrays(c):
    return tuple(a.copy() for a in c.arrays)                           # (the case's arrays are read-only; torch wants writable ones)


@functools.lru_cache(maxsize=None)
def _ref(name, cus):
    """the longdouble reference of a case: computed once, shared by the runs, never written"""
    c = ic.build(name, cus)
    rp, ci, va = c.arrays
    return pagerank_ref.pagerank(rp, ci, va, len(rp) - 1, tol=0.0, max_iterations=c.iters)


def _twice(label, A, arrays, iters, depth, **kw):
    """One checked run and a second one that must repeat it bit for bit; returns the first run's info."""
    r, info, ref = _run_fixed(label, A, arrays, iters=iters, depth=depth, **kw)
    r2, info2, _ = _run_fixed(label + ", again", A, arrays, iters=iters, depth=depth, ref=ref, **{k: v for k, v in kw.items() if k != "ref"})
    assert torch.equal(r, r2) and info2["residual"] == info["residual"] and info2["dangling"] == info["dangling"], label
    return info


@pytest.mark.parametrize("name", [n for n in ic.PR_NAMES if n != "capped_epilogue"])
def test_case_on_its_limit(name):
    capi, _ = _host()
    cus = _cus()
    c = ic.build(name, cus)
    f = ic.pr_facts(c, cus)
    print(f"pagerank limits {name}: cus {cus}, " + ", ".join(f"{k} {f[k]}" for k in ("n", "nnz", "avg", "lpr", "strength_grid", "strength_trips", "long_rows", "G", "dangling")))
    arrays = _arrays(c)
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM)
    info = _twice(name, A, arrays, c.iters, ic.sum_depth(f["n"]), ref=_ref(name, cus))
    assert A.transpose_info()["spmv_path"] == 0
    assert info["dangling"] == f["dangling"]                           # counted from the arrays, the reference's count apart


@pytest.fixture(scope="module")
def capped():
    """capped_epilogue and its handle, built once for the module"""
    capi, _ = _host()
    cus = _cus()
    c = ic.build("capped_epilogue", cus)
    arrays = _arrays(c)
    return c, arrays, _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM), ic.pr_facts(c, cus)


def test_capped_epilogue(capped):
    c, arrays, A, f = capped
    assert f["G"] == ic.MAX_GRID and f["epilogue_trips"] > ic.ITEMS and f["strength_trips"] >= 2 and f["first_trip_of_a_long_row"] >= 1
    print(f"pagerank limits capped_epilogue: cus {_cus()}, " + ", ".join(f"{k} {f[k]}" for k in ("n", "nnz", "lpr", "strength_trips", "long_trips", "G", "epilogue_trips", "dangling")))
    info = _twice("capped_epilogue", A, arrays, c.iters, ic.sum_depth(f["n"]), ref=_ref("capped_epilogue", _cus()))
    assert A.transpose_info()["spmv_path"] == 0 and info["dangling"] == f["dangling"]


def test_capped_epilogue_personalised_and_warm(capped):
    """vec_sum_kernel (twice), sums_verdict_kernel and init_kernel<true> under the same cap: 512 partials each, every workgroup on its ninth trip"""
    c, arrays, A, f = capped
    n = f["n"]
    rng = np.random.default_rng(41)
    pers, start = rng.uniform(0.0, 1.0, n), rng.uniform(0.1, 1.0, n)
    pers[::3] = 0.0
    _twice("capped_epilogue, personalised and warm", A, arrays, c.iters, ic.sum_depth(n), pers=pers, start=start)
    r8, _ = A.pagerank(tol=0.0, max_iterations=c.iters, personalization=_dev(pers * 8.0), start=_dev(start * 0.25))
    r1, _ = A.pagerank(tol=0.0, max_iterations=c.iters, personalization=_dev(pers), start=_dev(start))
    assert torch.equal(r1, r8)                                         # powers of two normalise exactly: the two sums of 512 partials scale with them


def test_bad_values_are_refused_wherever_they_hide():
    """One defect per array (iteration_cases.bad_values): in the last thread's share of a long row, in the last lane of a short row's group, in the
    last row, and two rows of finite entries whose sum alone overflows. Each is refused, and the handle is right again after the repair."""
    capi, _ = _host()
    cus = _cus()
    c = ic.build(ic.BAD_BASE, cus)
    arrays = _arrays(c)
    n = len(arrays[0]) - 1
    depth, ref = ic.sum_depth(n), _ref(ic.BAD_BASE, cus)
    A = _from_arrays(arrays, spmv_flags=capi.SPMV_STREAM | capi.SPMV_UPDATABLE)
    _run_fixed("before the defects", A, arrays, iters=c.iters, ref=ref, depth=depth)
    for b in ic.bad_values(cus):
        A.update_values(_dev(b.values.copy()))                         # (read-only, as the case's arrays are)
        with pytest.raises(capi.G4SError) as e:
            A.pagerank()
        assert e.value.status == capi.ERR_INVALID and "value" in str(e.value), b.tag
        A.update_values(_dev(arrays[2]))
        _run_fixed(f"after {b.tag}", A, arrays, iters=c.iters, ref=ref, depth=depth)   # a stale verdict or a stale 1 / s fails here
