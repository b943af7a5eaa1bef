"""Level-synchronous numpy reference of g4s_betweenness (include/g4s.h) in np.longdouble: the same recurrence, the same edge rule (a stored entry is
an edge when it is != 0, NaN included) and parallel edges for repeated columns. Also the graph builders the betweenness tests share and the parity
bar they assert."""
from collections import namedtuple

import numpy as np

from tests.pagerank_ref import csr_of_edges, rmat_edges

Result = namedtuple("Result", "bc max_depth sigma_max levels reached")

PARITY = 1e-10                                                        # the project's fp64 parity bar: |got − ref| <= 1e-10 · ref


def _rows_edges(rowptr, frontier):
    """The entry indices of the rows in `frontier`, row after row, and the row each one belongs to."""
    starts, lens = rowptr[frontier], rowptr[frontier + 1] - rowptr[frontier]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    owner = np.repeat(np.arange(frontier.size), lens)
    k = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens) + starts[owner]
    return k, frontier[owner]


def betweenness(rowptr, colids, values, n, sources, scale=1.0, dtype=np.longdouble):
    """bc[v] = scale · Σ_s δ_s(v) over the listed sources (a repeated one counts twice), in `dtype`: level = BFS depth, σ[s] = 1,
    σ[v] = Σ σ[u] over edges u → v one level up, δ[u] = Σ (σ[u] / σ[v]) · (1 + δ[v]) over edges u → v one level down, δ[s] = 0.
    Returns Result(bc, deepest level over all sources, largest σ, Σ_s (depth_s + 1), Σ_s vertices reached)."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    is_edge = np.asarray(values, np.float64) != 0                     # NaN != 0 is True
    one = dtype(1)
    total = np.zeros(n, dtype)
    max_depth, sigma_max, levels, reached = 0, dtype(0), 0, 0
    for s in np.atleast_1d(np.asarray(sources)).tolist():
        level = np.full(n, -1, np.int64)
        sigma = np.zeros(n, dtype)
        level[s], sigma[s] = 0, one
        frontier, d, tree_edges = np.array([s], np.int64), 0, []
        reached += 1
        while True:
            k, u = _rows_edges(rowptr, frontier)
            keep = is_edge[k]
            u, v = u[keep], colids[k][keep]
            new = np.unique(v[level[v] == -1])
            if new.size == 0:
                break
            level[new] = d + 1
            down = level[v] == d + 1
            u, v = u[down], v[down]
            np.add.at(sigma, v, sigma[u])
            tree_edges.append((u, v))
            frontier, d = new, d + 1
            reached += new.size
        levels += d + 1
        max_depth = max(max_depth, d)
        sigma_max = max(sigma_max, sigma.max())
        delta = np.zeros(n, dtype)
        for u, v in reversed(tree_edges):
            np.add.at(delta, u, sigma[u] / sigma[v] * (one + delta[v]))
        delta[s] = 0
        total += delta
    return Result(dtype(scale) * total, max_depth, sigma_max, levels, reached)


def check_parity(label, got, ref):
    """|got − ref| <= 1e-10 · ref, and got == 0 exactly where ref is 0 (every term is non-negative, so Σ|terms| is the value itself).
    Prints and returns the largest err / ref."""
    got, ref = np.asarray(got, np.float64).astype(np.longdouble), np.asarray(ref, np.longdouble)
    zero = ref == 0
    err = np.abs(got - ref)
    worst = float((err[~zero] / ref[~zero]).max()) if (~zero).any() else 0.0
    print(f"betweenness {label}: n {ref.size}, nonzero {int((~zero).sum())}, max value {float(ref.max()):.4e}, max err / ref {worst:.3e}")
    assert np.all(got[zero] == 0), label
    assert np.all(err <= PARITY * ref), (label, worst)
    return worst


# ---------------------------------------------------------------------------------------------- graphs (rowptr, colids, values)
def symmetrise(n, src, dst):
    """Both directions of every edge, self-loops and duplicates dropped."""
    a, b = np.concatenate([src, dst]), np.concatenate([dst, src])
    key = np.unique(a[a != b] * n + b[a != b])
    return csr_of_edges(n, key // n, key % n, np.ones(key.size))


def rmat_directed(scale, edge_factor, seed):
    """R-MAT with deduplicated entries (self-loops kept: they lie on no shortest path)."""
    n = 1 << scale
    src, dst = rmat_edges(scale, edge_factor, seed)
    key = np.unique(src * n + dst)
    return csr_of_edges(n, key // n, key % n, np.ones(key.size))


def rmat_symmetric(scale, edge_factor, seed):
    src, dst = rmat_edges(scale, edge_factor, seed)
    return symmetrise(1 << scale, src, dst)


def grid(nx_, ny_):
    """The undirected nx_ × ny_ 4-neighbour grid, vertex i · ny_ + j."""
    idx = np.arange(nx_ * ny_).reshape(nx_, ny_)
    src = np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()])
    dst = np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()])
    return symmetrise(nx_ * ny_, src, dst)


def path(n):
    return csr_of_edges(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1))


def star(leaves):
    return symmetrise(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))


def binary_tree(n):
    child = np.arange(1, n)
    return symmetrise(n, (child - 1) // 2, child)


def diamonds(k):
    """a_0 → {b_0, c_0} → a_1 → … → a_k, directed: 3k + 1 vertices, σ[a_i] = 2^i from a_0. a_i = 3i, b_i = 3i + 1, c_i = 3i + 2."""
    a = 3 * np.arange(k)
    src = np.concatenate([a, a, a + 1, a + 2])
    dst = np.concatenate([a + 1, a + 2, a + 3, a + 3])
    return csr_of_edges(3 * k + 1, src, dst, np.ones(4 * k))


def with_hub(arrays, hub, fan, seed):
    """`arrays` (symmetric, deduplicated) with vertex `hub` joined both ways to `fan` other vertices."""
    rp, ci, _ = arrays
    n = len(rp) - 1
    src = np.repeat(np.arange(n), np.diff(rp))
    others = np.random.default_rng(seed).permutation(np.delete(np.arange(n), hub))[:fan]
    return symmetrise(n, np.concatenate([src, np.full(fan, hub)]), np.concatenate([ci.astype(np.int64), others]))
