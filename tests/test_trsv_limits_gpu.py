"""g4s_sptrsv_* on the cases of tests/level_cases.py, which sit on the edges of the shared level frame (level_schedule.hpp, level_tile.hpp, frontier.hpp):
every stride of a level launch of several workgroups, tiles that hold lane, wave and hub rows at once, every chain stride, every main-loop/tail split
of the strided sums, the sort-pass boundaries of the layout, hub columns in the analysis peel and a peel that resumes. tests/test_level_cases_cpu.py
proves that each case stands on its edge; this file runs them, each as a lower triangle and mirrored as an upper one. Every comparison is == on bits
against tests/trsv_ref.py, through the checks of test_trsv_gpu.py and test_trsv_multi_gpu.py; every output is pre-filled with their sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import level_cases as lc
from tests import test_trsv_multi_gpu as tm
from tests import trsv_ref as ref
from tests.test_trsv_gpu import XFILL, Plan, _dev, _exact, _same_bits

pytestmark = pytest.mark.gpu

BOTH = [(name, lower) for name in sorted(lc.SOLVE) for lower in (True, False)]
PEEL = [(name, lower) for name, lower in BOTH if lc.SOLVE[name].peel]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name,lower", BOTH)
def test_case_equals_reference(name, lower):
    """device and host pointers, chains and one launch per level, x aliasing b: the reference's levels, info and bits; and the launch counts of the model"""
    mat, b, x = lc.solved(name, lower)
    with_chains, without = _exact(mat, lower, False, b, (name, lower))
    f = lc.facts(name, _cus(), lower)
    assert with_chains["launches_per_solve"] == len(f["launches"]) and with_chains["chains"] == sum(l[0] == "chain" for l in f["launches"])
    assert without["launches_per_solve"] == len(f["launches_no_chains"]) == f["levels"] == with_chains["levels"] and without["chains"] == 0
    p = Plan(mat, lower)
    _same_bits(p.solve(b), x, (name, lower, "the shared reference"))
    p.close()


@pytest.mark.parametrize("name,lower", BOTH)
def test_block_solve_equals_single_solves_and_reference(name, lower):
    """k = G4S_TRSV_RHS_TILE + 1 columns — a full tile and a masked one —, row-major and column-major with a padded leading dimension, out of place and in
    place, chains and one launch per level: every column is the device's own single solve of it by bits; the first column and the one of the tail tile
    are the reference's as well (the Python reference of every column would dominate the run time)"""
    k = tm._kt() + 1
    mat, b, x = lc.solved(name, lower)
    B = np.random.default_rng(50 + len(name)).uniform(-1.0, 1.0, (mat[0], k))
    B[:, 0] = b
    for no_chains in (False, True):
        plan = tm._plan(mat, lower, no_chains=no_chains)
        one = tm.singles(plan.solve, B)
        _same_bits(one[:, 0], x, (name, lower, no_chains, "column 0 against the reference"))
        if not no_chains:
            _same_bits(one[:, k - 1], ref.solve(*mat, B[:, k - 1], lower), (name, lower, "the tail tile against the reference"))
        tm.solve_checked(lambda b_, x_: plan.solve(b_, out=x_), B, one, (name, lower, no_chains), layouts=(("row", 3), ("col", 5)))
        plan.close()


@pytest.mark.parametrize("lower", (True, False))
def test_unroll_edges_block_equals_reference_in_every_column(lower):
    """The block solve is the same template as the single solve, so "every column is the device's single solve" compares two instantiations of one sum.
    On unroll_edges — every main-loop/tail split of all six (class, stride, unroll) instantiations in one matrix — all G4S_TRSV_RHS_TILE + 1 columns, the
    full tile and the masked one, are therefore the Python reference's own solve of that column by bits, row-major and column-major, with chains, out
    of place and in place, the padding still the sentinel. The single solve is pinned to the same reference by test_case_equals_reference."""
    k = tm._kt() + 1
    mat, b, x = lc.solved("unroll_edges", lower)
    B = np.random.default_rng(61).uniform(-1.0, 1.0, (mat[0], k))
    B[:, 0] = b
    want = np.stack([x] + [ref.solve(*mat, B[:, j], lower) for j in range(1, k)], axis=1)
    plan = tm._plan(mat, lower)
    assert plan.info["chains"] == 1
    tm.solve_checked(lambda b_, x_: plan.solve(b_, out=x_), B, want, ("unroll_edges", lower), layouts=(("row", 3), ("col", 5)))
    plan.close()


@pytest.mark.parametrize("name,lower", PEEL)
def test_analysis_counts_equal_the_model(name, lower):
    """resumes, launches and host_waits of the analysis are what the host loop of peel() gives on this device's CU count (level_cases.peel); a
    disagreement is settled by reading trsv.hip, never by copying the device's number"""
    mat, b, x = lc.solved(name, lower)
    f = lc.facts(name, _cus(), lower)
    print(f"{name} lower={lower} cus={_cus()}: resumes {f['resumes']}, launches {f['launches_analysis']}, host_waits {f['host_waits']}, grids {f['grids']}")
    for device in (True, False):
        p = Plan(mat, lower, device=device)
        print("  device" if device else "  host", p.info)
        assert (p.info["resumes"], p.info["launches"], p.info["host_waits"]) == (f["resumes"], f["launches_analysis"], f["host_waits"]), (name, device, p.info)
        assert p.info["levels"] == f["levels"] and p.info["widest_level"] == max(f["widths"])
        _same_bits(p.solve(b), x, (name, lower, device))
        p.close()
    q = Plan(mat, lower, with_level=False)                                  # no level array asked for: one wait fewer
    assert (q.info["resumes"], q.info["launches"], q.info["host_waits"]) == (f["resumes"], f["launches_analysis"], f["host_waits"] - 1)
    q.close()


def test_fan_resumes_on_this_device():
    """the frontier of 64 · 2049 entries outgrows the first grid of 8 workgroups wherever a larger one exists; 64 · 2048 is exactly its cap"""
    cus = _cus()
    for name, want in (("fan_2048", 0), ("fan_2049", 1 if 2 * cus > lc.MIN_GRID else 0)):
        p = Plan(lc.matrix(name))
        assert p.info["resumes"] == want == lc.facts(name, cus)["resumes"], (name, p.info)
        p.close()


@pytest.mark.parametrize("name", ["hub_cols", "hub_in_tile_s16"])
def test_update_values_equals_a_fresh_analysis(name):
    from g4s_amd import host
    for lower in (True, False):
        mat, b, _ = lc.solved(name, lower)
        n, rp, ci, va = mat
        new = np.random.default_rng(11).uniform(1.0, 2.0, va.size) * np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 8.0, 0.125 / 8.0)
        want = ref.solve(n, rp, ci, new, b, lower)
        assert not np.array_equal(want, lc.solved(name, lower)[2]) and np.all(np.isfinite(want))
        for device in (True, False):
            p = Plan(mat, lower, device=device)
            if device:
                p.capi.check(p.lib.g4s_sptrsv_update_values(p.handle, host._ptr_nn(_dev(new, np.float64)), p.capi.DEVICE_POINTERS, host._stream()))
            else:
                p.capi.check(p.lib.g4s_sptrsv_update_values(p.handle, C.c_void_p(new.ctypes.data), p.capi.HOST_POINTERS, host._stream()))
            _same_bits(p.solve(b), want, (name, lower, device))
            _same_bits(p.solve(b, alias=True), want, (name, lower, device, "x is b"))
            fresh = Plan((n, rp, ci, new), lower)
            _same_bits(fresh.solve(b), want)
            got, again = C.create_string_buffer(48), C.create_string_buffer(48)
            p.capi.check(p.lib.g4s_sptrsv_get_info(p.handle, C.cast(got, C.POINTER(p.capi.TRSVInfo))))
            p.capi.check(p.lib.g4s_sptrsv_get_info(fresh.handle, C.cast(again, C.POINTER(p.capi.TRSVInfo))))
            assert got.raw[:32] == again.raw[:32]                          # everything but the analysis's own launch counts
            p.close()
            fresh.close()


def test_chain_mixed_in_a_captured_graph():
    """the chain of three levels with every row class, captured: two replays on changed b equal the eager solves and the reference"""
    from g4s_amd import host
    for lower in (True, False):
        mat, b0, _ = lc.solved("chain_mixed", lower)
        n, rp, ci, va = mat
        plan = host.sptrsv_analyse((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)), lower)
        assert plan.info["chains"] == 1 and plan.info["launches_per_solve"] == 2
        b, x = _dev(b0, np.float64), torch.full((n,), XFILL, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                plan.solve(b, out=x)
        torch.cuda.current_stream().wait_stream(side)
        for k in range(2):
            bk = np.random.default_rng(20 + k).uniform(-1, 1, n)
            b.copy_(torch.from_numpy(bk))
            x.fill_(XFILL)
            g.replay()
            torch.cuda.synchronize()
            got = x.cpu().numpy()
            _same_bits(got, plan.solve(b).cpu().numpy(), (lower, k))
            _same_bits(got, ref.solve(*mat, bk, lower), (lower, k, "reference"))
        plan.close()
