"""A plain restatement of CitcomS's Jacobi-preconditioned conj_grad (citcoms/lib/General_matrix_functions.c:307-424) in numpy, in a number
format of the caller's choice — TEST INFRASTRUCTURE ONLY. The update order is the one written above oracle_conj_grad_elem (oracle/g4s_oracle.c):

    r1 = F, d0 = 0; residual = sqrt(r1·r1)
    while (residual > acc and count < steps) or count == 0:
        z1 = BI∘r1; dotr1z1 = r1·z1; p2 = z1 (first) | z1 + (dotr1z1/dotr0z0)·p1; dotr0z0 = dotr1z1
        Ap = matvec(p2) with the boundary rows zeroed
        dotprod = p2·Ap; alpha = 1e-3 if dotprod == 0 else dotr1z1/dotprod
        d0 += alpha·p2; r2 = r1 − alpha·Ap; residual = sqrt(r2·r2); rotate (r, p); count++
    d0[zero_resid] = 0

With dtype = np.longdouble (64-bit significand on x86) it is the reference of tests/test_cg_loop_gpu.py; with np.float64 it is a second legitimate
summation order (numpy's pairwise sums) whose distance from the longdouble run measures how far round-off alone moves an iterate: the bound rule."""
import numpy as np


def csr_matvec(rowptr, colids, values, dtype):
    """x ↦ A·x for a CSR matrix without empty rows, every product and sum in `dtype` (np.add.reduceat over the rows)."""
    rp = np.asarray(rowptr, np.int64)
    assert np.all(rp[1:] > rp[:-1]), "csr_matvec: np.add.reduceat needs every row to hold an entry"
    ci, va, starts = np.asarray(colids, np.int64), np.asarray(values, dtype), rp[:-1]
    return lambda x: np.add.reduceat(va * x[ci], starts)


def conj_grad(matvec, BI, zero_resid, F, acc, steps, dtype, keep_iterates=False):
    """Returns (d0, count, residual, hist, iterates): hist[k] is the residual after k+1 iterations, iterates[k] the stripped d0 after k+1
    iterations (kept only with keep_iterates=True, else an empty list). Everything — vectors, dot products, alpha, beta — is in `dtype`."""
    dot = lambda a, b: np.sum(a * b, dtype=dtype)
    BI, F = np.asarray(BI, dtype), np.asarray(F, dtype)
    zr = np.asarray(zero_resid if zero_resid is not None else [], np.int64)
    acc = dtype(acc)
    r1, d0, p1 = F.copy(), np.zeros(len(F), dtype), np.zeros(len(F), dtype)
    residual = np.sqrt(dot(r1, r1))
    dotr0z0, count, hist, iterates = dtype(0), 0, [], []
    with np.errstate(all="ignore"):                                # past exact convergence the source divides 0 by 0 too
        while (residual > acc and count < steps) or count == 0:
            z1 = BI * r1
            dotr1z1 = dot(r1, z1)
            p2 = z1.copy() if count == 0 else z1 + (dotr1z1 / dotr0z0) * p1
            dotr0z0 = dotr1z1
            Ap = np.array(matvec(p2), dtype)
            Ap[zr] = 0
            dotprod = dot(p2, Ap)
            alpha = dtype(1.0e-3) if dotprod == 0 else dotr1z1 / dotprod
            d0 = d0 + alpha * p2
            r1 = r1 - alpha * Ap
            residual = np.sqrt(dot(r1, r1))
            hist.append(residual)
            p1 = p2
            count += 1
            if keep_iterates:
                it = d0.copy()
                it[zr] = 0
                iterates.append(it)
    d0[zr] = 0
    return d0, count, residual, np.array(hist, dtype), iterates


def rel_gap(a, b):
    """max|a − b| / max|b| with b the longdouble side (the `gap` and the `err` of the bound rule); 0 where both vanish."""
    a, b = np.atleast_1d(np.asarray(a, np.longdouble)), np.atleast_1d(np.asarray(b, np.longdouble))
    den = np.max(np.abs(b))
    num = np.max(np.abs(a - b))
    return 0.0 if num == 0 else float(num / den)


BOUND_FACTOR, GAP_FLOOR, GAP_MAX = 16.0, 2.0 ** -50, 1e-10


def bound(gap):
    """The bound rule: a device result may be 16·max(gap, 2⁻⁵⁰) from the longdouble reference, gap = the float64 restatement's own distance."""
    return BOUND_FACTOR * max(gap, GAP_FLOOR)
