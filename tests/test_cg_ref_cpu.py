"""tests/cg_ref.py pinned to the oracle's conj_grad (oracle_conj_grad_elem), and the preconditions of tests/test_cg_loop_gpu.py — no GPU.

The oracle adds left to right, cg_ref in float64 adds pairwise, cg_ref in longdouble is the reference: the oracle stands where the device stands in
the GPU tests and must meet the same bound rule, err <= 16·max(gap, 2⁻⁵⁰) with gap = |cg_ref float64 − cg_ref longdouble| (relative, max norm)."""
import numpy as np
import pytest

from tests import cg_cases, cg_ref
from tests.helpers import assemble_csr


def _elem(oracle, ex, ey, ez, seed):
    from tests.test_cg_gpu import _setup
    ien, idmap, nno, neq, K, bc, F = _setup(ex, ey, ez, seed)
    BI = oracle.element_inverse_diagonal(ien, idmap, K, neq)
    matvec = lambda u: oracle.element_matvec(ien, idmap, K, u, neq)
    return ien, idmap, neq, K, bc, F, BI, matvec, cg_ref.csr_matvec(*assemble_csr(ien, idmap, K, neq), np.longdouble)


@pytest.mark.parametrize("ex,ey,ez,rel_acc,seed", [(3, 3, 2, 1e-8, 0), (8, 8, 4, 1e-6, 1)])
def test_cg_ref_matches_oracle(oracle, ex, ey, ez, rel_acc, seed):
    ien, idmap, neq, K, bc, F, BI, matvec, matvec_ld = _elem(oracle, ex, ey, ez, seed)
    acc = rel_acc * np.linalg.norm(F)
    d_or, cyc_or, res_or, hist_or = oracle.conj_grad_elem(ien, idmap, K, neq, BI, bc, F, acc, 250)
    d64, cyc64, res64, hist64, it64 = cg_ref.conj_grad(matvec, BI, bc, F, acc, 250, np.float64, keep_iterates=True)
    dld, cycld, resld, histld, itld = cg_ref.conj_grad(matvec_ld, BI, bc, F, acc, 250, np.longdouble, keep_iterates=True)
    assert cyc64 == cyc_or == cycld and len(hist64) == cyc_or
    assert np.all(d64[bc] == 0.0) and np.array_equal(it64[-1], d64)
    gap = cg_ref.rel_gap(d64, dld)
    assert gap <= cg_ref.GAP_MAX
    assert cg_ref.rel_gap(d_or, dld) <= cg_ref.bound(gap), (cg_ref.rel_gap(d_or, dld), gap)
    for k in range(cyc_or):
        gap = cg_ref.rel_gap(hist64[k], histld[k])
        assert gap <= cg_ref.GAP_MAX
        assert cg_ref.rel_gap(hist_or[k], histld[k]) <= cg_ref.bound(gap), (k, hist_or[k], histld[k], gap)
    assert res64 == hist64[-1] and cg_ref.rel_gap(res_or, resld) <= cg_ref.bound(cg_ref.rel_gap(res64, resld))


@pytest.mark.parametrize("ex,ey,ez,seed", [(3, 3, 2, 0), (8, 8, 4, 1)])
def test_cg_ref_degenerate_cases_match_oracle(oracle, ex, ey, ez, seed):
    ien, idmap, neq, K, bc, F, BI, matvec, matvec_ld = _elem(oracle, ex, ey, ez, seed)
    # zero right-hand side: the count == 0 clause runs one iteration, alpha = 1e-3 on a zero direction
    d_or, cyc_or, res_or, _ = oracle.conj_grad_elem(ien, idmap, K, neq, BI, bc, np.zeros(neq), 1e-8, 250)
    d, cyc, res, hist, _ = cg_ref.conj_grad(matvec, BI, bc, np.zeros(neq), 1e-8, 250, np.float64)
    assert cyc == cyc_or == 1 and res == res_or == 0.0 and np.array_equal(d, d_or) and not d.any() and list(hist) == [0.0]
    # steps = 0: still one iteration
    d_or, cyc_or, res_or, _ = oracle.conj_grad_elem(ien, idmap, K, neq, BI, bc, F, 0.0, 0)
    d, cyc, res, _, _ = cg_ref.conj_grad(matvec, BI, bc, F, 0.0, 0, np.float64)
    dld, _, resld, _, _ = cg_ref.conj_grad(matvec_ld, BI, bc, F, 0.0, 0, np.longdouble)
    assert cyc == cyc_or == 1
    assert cg_ref.rel_gap(d_or, dld) <= cg_ref.bound(cg_ref.rel_gap(d, dld)) and cg_ref.rel_gap(res_or, resld) <= cg_ref.bound(cg_ref.rel_gap(res, resld))
    # every equation on the boundary list: Ap is zero, so alpha = 1e-3, r never changes and the loop runs into its cap
    every = np.arange(neq, dtype=np.int32)
    d_or, cyc_or, res_or, hist_or = oracle.conj_grad_elem(ien, idmap, K, neq, BI, every, F, 0.0, 3)
    d, cyc, res, hist, _ = cg_ref.conj_grad(matvec, BI, every, F, 0.0, 3, np.float64)
    normF = float(np.sqrt(np.sum(np.asarray(F, np.longdouble) ** 2)))
    assert cyc == cyc_or == 3 and not d.any() and not d_or.any()
    assert abs(res - normF) <= 4 * np.spacing(normF) and abs(res_or - normF) <= 4 * np.spacing(normF)
    assert np.all(hist == hist[0]) and np.all(hist_or == hist_or[0])


def _gpu_problems(oracle):
    return [cg_cases.elem_problem(1, 1, 1, 0, oracle), cg_cases.elem_problem(8, 8, 4, 1, oracle), cg_cases.node_problem(oracle), cg_cases.dist_problem(oracle)] + \
           [cg_cases.band_problem(n) for n in cg_cases.CSR_SIZES + (1025,)]


def test_gpu_problems_meet_their_preconditions(oracle):
    """What tests/test_cg_loop_gpu.py asserts before it compares: round-off alone moves no compared iterate or residual by more than 1e-10, every
    capped solve really reaches its cap, and the residuals around each stopping iteration differ by more than a factor 1.5."""
    for p in _gpu_problems(oracle):
        R = cg_cases.reference(p)
        assert not p["F"][p["bc"]].any()
        for k in range(1, cg_cases.MAX_IT + 1):
            if not cg_cases.comparable(p, k):
                continue
            assert R.count >= k and R.f64[1] >= k, (p["name"], k)
            assert R.gap_d0(k) <= cg_ref.GAP_MAX, (p["name"], k, R.gap_d0(k))
            if cg_cases.comparable_residual(p, k):
                assert R.gap_res(k) <= cg_ref.GAP_MAX, (p["name"], k, R.gap_res(k))
        if p["n"] > max(cg_cases.STOP_AT):
            for k in cg_cases.STOP_AT:
                assert R.residual(k - 1) > 1.5 * R.residual(k), (p["name"], k)
