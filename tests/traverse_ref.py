"""Reference for g4s_sssp / g4s_bfs (include/g4s.h), numpy only. The graph is a CSR stored by out-edges (row i: the edges i → j, weight a_ij).
SSSP is the min-plus fixed point of d := d ⊕ (Aᵀ ⊗ d), iterated synchronously with spmv_semiring_ref.spmv from d[sources] = 0; BFS is the or-and loop
of INTEGRATION.md. Both are exact, so the device must match bit for bit (semiring_ref.same_values)."""
import numpy as np

from tests import spmv_semiring_ref
from tests.semiring_ref import same_values  # noqa: F401  (re-exported for the tests)


def transpose(rp, ci, va, n):
    """Aᵀ of an n × n CSR, stable, duplicates kept (what g4s_csr_transpose builds)."""
    rp, ci, va = np.asarray(rp), np.asarray(ci), np.asarray(va, np.float64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp).astype(np.int64))
    perm = np.argsort(ci, kind="stable")
    trp = np.zeros(n + 1, np.int64)
    np.add.at(trp, ci.astype(np.int64) + 1, 1)
    return np.cumsum(trp).astype(np.int32), row[perm].astype(np.int32), va[perm]


def sssp(rp, ci, va, n, sources, max_rounds=0, keep=()):
    """(dist, rounds, converged, {k: the vector after k rounds for k in keep}). rounds counts the products run, the last of which changed nothing when
    converged (so a chain of L edges takes L + 1). max_rounds = 0 means n."""
    trp, tci, tva = transpose(rp, ci, va, n)
    d = np.full(n, np.inf)
    d[np.asarray(sources, np.int64)] = 0.0
    after, cap = {}, (max_rounds or n)
    if 0 in keep:
        after[0] = d.copy()
    for k in range(1, cap + 1):
        new = spmv_semiring_ref.spmv(trp, tci, tva, d, "min_plus", y=d)
        same = np.array_equal(new, d)
        d = new
        if k in keep:
            after[k] = d.copy()
        if same:
            return d, k, True, after
    return d, cap, False, after


def bfs(rp, ci, va, n, sources, max_depth=0):
    """(level int32 with −1 where unreached, depth of the deepest level). An entry is an edge when its value is != 0 (or-and)."""
    trp, tci, tva = transpose(rp, ci, va, n)
    frontier = np.zeros(n)
    frontier[np.asarray(sources, np.int64)] = 1.0
    visited = frontier.copy()
    level = np.full(n, -1, np.int32)
    level[frontier != 0] = 0
    depth = 0
    while frontier.any() and (max_depth == 0 or depth < max_depth):
        depth += 1
        frontier = spmv_semiring_ref.spmv(trp, tci, tva, frontier, "or_and") * (1.0 - visited)
        level[frontier != 0] = depth
        visited = np.maximum(visited, frontier)
    return level, int(level.max())
