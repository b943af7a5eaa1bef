"""numpy reference of g4s_pagerank's iteration (include/g4s.h), with the floating-point type as a parameter: np.longdouble is the yardstick of the GPU
tests, np.float64 the CPU self-test. Also the graph builders the PageRank tests share and the accuracy bound they assert."""
import math
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "rank residuals dangling max_in_degree max_out_degree kept")


def csr_of_edges(n, src, dst, w):
    """CSR by out-edges of an edge list, in the given order inside a row (duplicates kept)."""
    src, dst, w = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.float64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    return np.cumsum(rp).astype(np.int32), dst[order].astype(np.int32), w[order]


def rmat_edges(scale, edge_factor, seed, probs=(0.57, 0.19, 0.19, 0.05)):
    """A seeded R-MAT edge list on 2^scale vertices, duplicates and self-loops kept: (src, dst)."""
    rng = np.random.default_rng(seed)
    m = edge_factor << scale
    src, dst = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for _ in range(scale):
        q = rng.choice(4, size=m, p=probs)
        src = (src << 1) | (q >> 1)
        dst = (dst << 1) | (q & 1)
    return src, dst


def rmat_csr(scale, edge_factor, seed, weighted=True):
    src, dst = rmat_edges(scale, edge_factor, seed)
    w = np.random.default_rng(seed + 1).uniform(0.25, 4.0, src.size) if weighted else np.ones(src.size)
    return csr_of_edges(1 << scale, src, dst, w)


def gamma(n, max_in_degree, max_out_degree, sum_depth=None):
    """γ of the accuracy bound: a float64 run and the exact iteration differ by at most γ / (1 − damping) in L1 (tests/test_pagerank_gpu.py).
    sum_depth: the additions a term of the dangling-mass (and residual) sum passes through; None: ⌈log₂ n⌉ + 8, which holds while the epilogue's grid
    is far below its cap (n <= 2¹⁴). Under the capped grid the caller passes the depth read off the code (tests/iteration_cases.py, sum_depth)."""
    if sum_depth is None:
        sum_depth = math.ceil(math.log2(max(n, 1))) + 8
    return (max_in_degree + max_out_degree + sum_depth + 8) * 2.0 ** -53


def _segment_sums(v, starts, n_segments, dtype):
    """Σ of v over the segments [starts[i], starts[i + 1]) — zero for an empty one (np.add.reduceat alone returns v[starts[i]] there)."""
    out = np.zeros(n_segments, dtype)
    lens = np.diff(starts)
    nonempty = lens > 0
    if v.size and nonempty.any():
        out[nonempty] = np.add.reduceat(v, starts[:-1][nonempty])
    return out


def pagerank(rowptr, colids, values, n, damping=0.85, tol=0.0, max_iterations=0, personalization=None, start=None, dtype=np.longdouble, keep=()):
    """The iteration of include/g4s.h in `dtype`, in its order of operations: x = r · (1 / s) (0 where s == 0), y = Aᵀ x, m = Σ_{dangling} r,
    r' = damping · (y + m · p) + (1 − damping) · p, residual = Σ |r' − r|; stops after the first iteration with residual < tol or at the cap
    (0: 100). Returns Result(rank, residuals of every iteration, dangling count, max in-degree, max out-degree, {k: iterate k for k in keep})."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    a = np.asarray(values, np.float64).astype(dtype)
    assert np.all(np.isfinite(np.asarray(values, np.float64))) and np.all(np.asarray(values) >= 0)
    d = dtype(damping)
    one = dtype(1)
    cap = max_iterations if max_iterations > 0 else 100
    s = _segment_sums(a, rowptr, n, dtype)
    dangling = ~(s > 0)
    inv_s = np.zeros(n, dtype)
    inv_s[~dangling] = one / s[~dangling]
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    by_col = np.argsort(colids, kind="stable")
    col_starts = np.concatenate([[0], np.cumsum(np.bincount(colids, minlength=n))]).astype(np.int64)
    a_t, row_t = a[by_col], row_of[by_col]
    if personalization is None:
        p = np.full(n, one / dtype(n), dtype)
    else:
        pers = np.asarray(personalization, np.float64).astype(dtype)
        p = pers / pers.sum()
    if start is None:
        r = p.copy()
    else:
        st = np.asarray(start, np.float64).astype(dtype)
        r = st / st.sum()
    residuals, kept = [], {}
    if 0 in keep:
        kept[0] = r.copy()
    for k in range(1, cap + 1):
        x = r * inv_s
        y = _segment_sums(a_t * x[row_t], col_starts, n, dtype)
        m = r[dangling].sum() if dangling.any() else dtype(0)
        rn = d * (y + m * p) + (one - d) * p
        res = np.abs(rn - r).sum()
        r = rn
        residuals.append(res)
        if k in keep:
            kept[k] = r.copy()
        if res < tol:
            break
    max_in = int(np.bincount(colids, minlength=max(n, 1)).max()) if colids.size else 0
    max_out = int(np.diff(rowptr).max()) if n else 0
    return Result(r, residuals, int(dangling.sum()), max_in, max_out, kept)
