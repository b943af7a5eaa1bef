"""numpy reference for g4s_kcore: the synchronous peeling that include/g4s.h defines, restated on the host, and the graphs the tests share.

Peeling: k = the smallest remaining degree (never decreasing); a frontier is ALL remaining vertices of degree <= k, removed at once; the next frontier
is the vertices that this removal brought to <= k; when a level runs dry k rises to the smallest remaining degree. core[v] = the k at which v left,
round[v] = the 0-based index of the frontier that took it. tests/test_kcore_cpu.py pins core against networkx.core_number and (round, id) as a degeneracy
ordering on every case, so the yardstick of the GPU tests rests on something this project did not write.

The R-MAT cases come from a numpy generator (rmat_edges: the quadrant probabilities 0.57 / 0.19 / 0.19 / 0.05 of the library's own generator) because
the library's generator runs on the device and the CPU tests have to see the same graph; tests/test_kcore_gpu.py also runs one graph of the library's
generator against this reference."""
import functools

import numpy as np


def _row_ids(rp, n):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))


def _entries_of(rp, rows):
    """indices of the stored entries of `rows`, row after row"""
    start, length = rp[rows], rp[rows + 1] - rp[rows]
    total = int(length.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(length) - length
    return np.repeat(start - first, length) + np.arange(total, dtype=np.int64)


def degrees(rp, ci, n):
    """row length minus a stored diagonal entry"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    return np.diff(rp) - np.bincount(_row_ids(rp, n)[ci == _row_ids(rp, n)], minlength=n)


def kcore(rp, ci, n, max_k=None):
    """(core, round, levels, rounds, capped) of the symmetric pattern (rp, ci); max_k=None: the full decomposition"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    deg = degrees(rp, ci, n).astype(np.int64)
    core, rnd = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    alive = np.ones(n, bool)
    levels = rounds = k = 0
    capped = 0
    while alive.any():
        k = max(k, int(deg[alive].min()))
        if max_k is not None and k >= max_k:
            capped = 1
            break
        levels += 1
        front = np.flatnonzero(alive & (deg <= k))
        while front.size:
            core[front], rnd[front] = k, rounds
            rounds += 1
            alive[front] = False
            nb = ci[_entries_of(rp, front)]
            nb = nb[alive[nb]]                                        # the frontier's own members (a diagonal entry among them) are gone
            touched, count = np.unique(nb, return_counts=True)
            deg[touched] -= count
            front = touched[deg[touched] <= k]                        # alive and outside the frontier: they were above k
    if capped:
        core[alive] = max_k
    return core, rnd, levels, rounds, capped


def top_core(core):
    """(degeneracy, vertices with that core number)"""
    d = int(core.max()) if core.size else 0
    return d, int(np.count_nonzero(core == d))


def degeneracy_order(rnd):
    """the vertices sorted by (round, id): round −1 (left by max_k) last"""
    key = np.where(rnd < 0, np.iinfo(np.int32).max, rnd)
    return np.lexsort((np.arange(rnd.size), key)).astype(np.int32)


def later_neighbours(rp, ci, n, order):
    """per vertex: its neighbours (itself excluded) at or after its own position in `order`"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    rows = _row_ids(rp, n)
    keep = (ci != rows) & (pos[ci] >= pos[rows])
    return np.bincount(rows[keep], minlength=n)


def networkx_core(rp, ci, n):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    rows = _row_ids(np.asarray(rp, np.int64), n)
    off = np.asarray(ci) != rows
    G.add_edges_from(zip(rows[off].tolist(), np.asarray(ci)[off].tolist()))
    c = nx.core_number(G)
    return np.array([c[v] for v in range(n)], np.int32)


# ------------------------------------------------------------------------------------------------ graphs
def from_edges(n, edges, loops=()):
    """the symmetric pattern of the undirected edges (m × 2), repeats merged, rows ascending; `loops`: vertices with a stored diagonal entry"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    l = np.asarray(list(loops), np.int64)
    r = np.concatenate([e[:, 0], e[:, 1], l])
    c = np.concatenate([e[:, 1], e[:, 0], l])
    key = np.unique(r * n + c)
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=rp[1:])
    return rp.astype(np.int32), (key % n).astype(np.int32)


def clique_edges(ids):
    ids = np.asarray(ids, np.int64)
    a, b = np.triu_indices(ids.size, 1)
    return np.stack([ids[a], ids[b]], 1)


def tiny():
    return 8, from_edges(8, [(1, 2), (2, 3), (3, 1), (5, 6)], loops=(0, 3))


def star(leaves=5000):
    return leaves + 1, from_edges(leaves + 1, np.stack([np.zeros(leaves, np.int64), np.arange(1, leaves + 1)], 1))


def hub_leaves_clique(leaves=4990, clique=20, tied=10):
    n = 1 + leaves + clique
    cl = np.arange(1 + leaves, n)
    spokes = np.concatenate([np.arange(1, 1 + leaves), cl[:tied]])
    return n, from_edges(n, np.concatenate([np.stack([np.zeros(spokes.size, np.int64), spokes], 1), clique_edges(cl)]))


def path(n=4001):
    return n, from_edges(n, np.stack([np.arange(n - 1), np.arange(1, n)], 1))


def grid(nx=64, ny=64):
    v = np.arange(nx * ny).reshape(ny, nx)
    e = np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1), np.stack([v[:-1].ravel(), v[1:].ravel()], 1)])
    return nx * ny, from_edges(nx * ny, e)


def doubling_tree(depth=14, clique=40):
    """a complete binary tree (root 0, children of v: 2v + 1 and 2v + 2); leaf j is tied to clique vertices 2j and 2j + 1 (mod the clique)"""
    tree = (1 << (depth + 1)) - 1
    n = tree + clique
    child = np.arange(1, tree)
    leaves = np.arange((1 << depth) - 1, tree)
    j = np.arange(leaves.size)
    ties = np.concatenate([np.stack([leaves, tree + (2 * j) % clique], 1), np.stack([leaves, tree + (2 * j + 1) % clique], 1)])
    return n, from_edges(n, np.concatenate([np.stack([(child - 1) // 2, child], 1), ties, clique_edges(np.arange(tree, n))]))


def rmat_edges(scale, edge_factor, seed):
    rng = np.random.default_rng(seed)
    m = edge_factor << scale
    r, c = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for _ in range(scale):
        u = rng.random(m)
        r = 2 * r + (u >= 0.76)                                       # quadrants: 0.57 | 0.19 / 0.19 | 0.05
        c = 2 * c + (((u >= 0.57) & (u < 0.76)) | (u >= 0.95))
    return np.stack([r, c], 1)


def rmat(scale=13, edge_factor=16, seed=20240613):
    """symmetrised R-MAT; the self-loops the generator draws stay stored as diagonal entries"""
    e = rmat_edges(scale, edge_factor, seed)
    loop = e[:, 0] == e[:, 1]
    return 1 << scale, from_edges(1 << scale, e[~loop], loops=np.unique(e[loop, 0]))


CASES = {"tiny": tiny, "star": star, "hub_leaves_clique": hub_leaves_clique, "path": path, "grid": grid, "doubling_tree": doubling_tree, "rmat13": rmat}


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, rowptr, colids, core, round, levels, rounds) of a named case: built and peeled once per process, arrays read-only"""
    n, (rp, ci) = CASES[name]()
    core, rnd, levels, rounds, _ = kcore(rp, ci, n)
    for a in (rp, ci, core, rnd):
        a.setflags(write=False)
    return n, rp, ci, core, rnd, levels, rounds
