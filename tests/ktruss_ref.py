"""numpy reference for g4s_ktruss: the synchronous edge peeling that include/g4s.h defines, restated on the host, and the graphs the tests share.

Peeling: the support of an edge is the number of triangles through it; j = the smallest remaining support (never decreasing); a frontier is ALL
remaining edges of support <= j, removed at once with truss = j + 2 and round = the 0-based index of that frontier. A triangle all of whose edges were
present before the removal and which holds at least one frontier edge dies ONCE: each of its edges outside the frontier loses exactly 1. The next
frontier is the edges that this brought to <= j; when a level runs dry j rises to the smallest remaining support. tests/test_ktruss_cpu.py pins the
truss numbers against networkx.k_truss for every k, so the yardstick of the GPU tests rests on something this project did not write.

All results are per STORED ENTRY of the symmetric CSR pattern, as the library returns them: both copies of an edge carry the same values, a diagonal
entry gets truss 0, round −1, support 0. The graphs are built with tests/kcore_ref.py's from_edges / clique_edges / rmat."""
import functools

import numpy as np

from tests import kcore_ref as kref

HUB_CUT = 4096                         # frontier.hpp: kHubCut


def edge_ids(rp, ci, n):
    """(eid per stored entry, eu, ev): the compact id of an undirected off-diagonal edge is the rank of its entry right of the diagonal; −1 on the diagonal"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    up = ci > rows
    eu, ev = rows[up], ci[up]
    keys = eu * n + ev                                                # ascending: rows ascend, and the ids inside a row
    eid = np.full(ci.size, -1, np.int64)
    eid[up] = np.arange(keys.size)
    low = ci < rows
    pos = np.searchsorted(keys, ci[low] * n + rows[low])
    assert np.array_equal(keys[pos], ci[low] * n + rows[low]), "the pattern is not symmetric"
    eid[low] = pos
    return eid, eu, ev


def walk_len(rp, eu, ev):
    """the entries the library walks for an edge: the shorter of its endpoints' stored rows"""
    d = np.diff(np.asarray(rp, np.int64))
    return np.minimum(d[eu], d[ev])


def triangles(eu, ev, n):
    """(T, 3) edge ids of every triangle, each once: vertices relabelled by (degree, id), every edge directed upwards, pairs of out-neighbours looked up"""
    m = eu.size
    if m == 0:
        return np.zeros((0, 3), np.int64)
    deg = np.bincount(np.concatenate([eu, ev]), minlength=n)
    rank = np.empty(n, np.int64)
    rank[np.lexsort((np.arange(n), deg))] = np.arange(n)
    a, b = np.minimum(rank[eu], rank[ev]), np.maximum(rank[eu], rank[ev])
    order = np.argsort(a * n + b, kind="stable")                      # position in the directed list → edge id
    a, b = a[order], b[order]
    keys = a * n + b
    last = np.searchsorted(a, a, side="right")
    later = last - np.arange(m) - 1                                   # out-neighbours of a behind b
    i = np.repeat(np.arange(m), later)
    k = np.arange(i.size) - np.repeat(np.cumsum(later) - later, later) + i + 1
    want = b[i] * n + b[k]
    pos = np.minimum(np.searchsorted(keys, want), m - 1)
    hit = keys[pos] == want
    return np.stack([order[i[hit]], order[k[hit]], order[pos[hit]]], 1)


def ktruss(rp, ci, n, max_k=None):
    """(support, truss, round, levels, rounds, capped): the first three per stored entry of the symmetric pattern (rp, ci); max_k=None: the full decomposition"""
    eid, eu, ev = edge_ids(rp, ci, n)
    m = eu.size
    T = triangles(eu, ev, n)
    sup0 = np.bincount(T.ravel(), minlength=m).astype(np.int64)
    sup = sup0.copy()
    by_edge = np.argsort(T.ravel(), kind="stable") // 3               # the triangles of edge c: by_edge[start[c]:start[c + 1]]
    start = np.zeros(m + 1, np.int64)
    np.cumsum(sup0, out=start[1:])
    tri_alive = np.ones(T.shape[0], bool)
    alive, in_front = np.ones(m, bool), np.zeros(m, bool)
    truss, rnd = np.zeros(m, np.int32), np.full(m, -1, np.int32)
    levels = rounds = j = capped = 0
    while alive.any():
        j = max(j, int(sup[alive].min()))
        if max_k is not None and j + 2 >= max_k:
            capped = 1
            break
        levels += 1
        front = np.flatnonzero(alive & (sup <= j))
        while front.size:
            truss[front], rnd[front] = j + 2, rounds
            rounds += 1
            alive[front] = False
            in_front[front] = True
            t = np.unique(by_edge[kref._entries_of(start, front)])
            t = t[tri_alive[t]]                                       # every edge of these was present before this removal
            tri_alive[t] = False                                      # the triangle dies once, however many of its edges are in the frontier
            e = T[t].ravel()
            e = e[~in_front[e]]
            in_front[front] = False
            touched, count = np.unique(e, return_counts=True)
            sup[touched] -= count
            front = touched[sup[touched] <= j]                        # alive and outside the frontier: they were above j
    if capped:
        truss[alive] = max_k
    on = eid >= 0
    spread = lambda x, dflt: np.where(on, x[np.maximum(eid, 0)] if m else dflt, dflt).astype(np.int32)
    return spread(sup0, 0), spread(truss, 0), spread(rnd, -1), levels, rounds, capped


def facts(rp, ci, n, support, truss):
    """(undirected edges, triangles, max truss, undirected edges at the max truss) from the per-entry results"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    up = np.asarray(ci) > rows
    top = int(truss[up].max()) if up.any() else 0
    return int(up.sum()), int(support[up].sum()) // 3, top, int(np.count_nonzero(truss[up] == top)) if up.any() else 0


def networkx_graph(rp, ci, n):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = np.asarray(ci) != rows
    G.add_edges_from(zip(rows[off].tolist(), np.asarray(ci)[off].tolist()))
    return G


def truss_edges(rp, ci, n, truss, k):
    """the undirected edges (u < v) with truss >= k"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = (np.asarray(ci) > rows) & (truss >= k)
    return set(zip(rows[keep].tolist(), np.asarray(ci)[keep].tolist()))


# ------------------------------------------------------------------------------------------------ graphs
def k4_ear():
    """K4 on 0 … 3 plus vertex 4 tied to 0 and 1: the triangle (0, 1, 4) has two frontier edges and must take one, not two, off (0, 1)"""
    return 5, kref.from_edges(5, np.concatenate([kref.clique_edges(np.arange(4)), [(0, 4), (1, 4)]]))


def tri_grid(nx=64, ny=64):
    """the grid plus one diagonal per cell: everything is truss 3, peeled from the two corners without a diagonal inwards, one anti-diagonal per round"""
    v = np.arange(nx * ny).reshape(ny, nx)
    e = np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1), np.stack([v[:-1].ravel(), v[1:].ravel()], 1),
                        np.stack([v[:-1, :-1].ravel(), v[1:, 1:].ravel()], 1)])
    return nx * ny, kref.from_edges(nx * ny, e)


def hub_bridge(leaves=4100):
    """u = 0 and v = 1 joined, K9 on {0, 2, 3, 4, 5 … 9} and on {1, 2, 3, 4, 10 … 14}, `leaves` private leaves on each of u and v: (0, 1) has support 3
    and is peeled alone, its shorter row has leaves + 9 entries, and its three triangles are alive when it goes"""
    n = 15 + 2 * leaves
    l0, l1 = np.arange(15, 15 + leaves), np.arange(15 + leaves, n)
    e = np.concatenate([[(0, 1)], kref.clique_edges([0, 2, 3, 4, 5, 6, 7, 8, 9]), kref.clique_edges([1, 2, 3, 4, 10, 11, 12, 13, 14]),
                        np.stack([np.zeros(leaves, np.int64), l0], 1), np.stack([np.ones(leaves, np.int64), l1], 1)])
    return n, kref.from_edges(n, e)


def hub_pair(leaves=4100):
    """0 and 1 joined and sharing `leaves` leaves, K6 on {0, 1, leaves + 2 … leaves + 5}: the support pass meets a hub edge with leaves + 4 hits"""
    n = leaves + 6
    l = np.arange(2, 2 + leaves)
    e = np.concatenate([[(0, 1)], np.stack([np.zeros(leaves, np.int64), l], 1), np.stack([np.ones(leaves, np.int64), l], 1),
                        kref.clique_edges([0, 1] + list(range(leaves + 2, n)))])
    return n, kref.from_edges(n, e)


def tri_tree(depth=16):
    """A binary tree of triangles grown from the weak edge (0, 1): every edge of generation g (2^g of them) carries one triangle whose two other edges
    are generation g + 1; every edge of the last generation sits in a K4 with two vertices of its own. The root has support 1, the inner edges 2, the
    last generation 3 and the K4s' other edges 2, so level j = 1 peels the generations root-outward, one per round, the frontier doubling."""
    a, b = np.array([0], np.int64), np.array([1], np.int64)
    edges, nv = [np.stack([a, b], 1)], 2
    for _ in range(depth):
        c = nv + np.arange(a.size)
        nv += a.size
        a, b = np.concatenate([a, b]), np.concatenate([c, c])
        edges.append(np.stack([a, b], 1))
    p, q = nv + np.arange(a.size), nv + a.size + np.arange(a.size)
    nv += 2 * a.size
    edges += [np.stack([x, y], 1) for x, y in ((a, p), (a, q), (b, p), (b, q), (p, q))]
    return nv, kref.from_edges(nv, np.concatenate(edges))


CASES = {"tiny": kref.tiny, "star": kref.star, "path": kref.path, "grid": kref.grid, "k4_ear": k4_ear, "hub_leaves_clique": kref.hub_leaves_clique,
         "tri_grid": tri_grid, "rmat10": lambda: kref.rmat(10, 16, 20240613), "rmat11": lambda: kref.rmat(11, 16, 20240613), "hub_bridge": hub_bridge,
         "hub_pair": hub_pair, "tri_tree": tri_tree}


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, rowptr, colids, support, truss, round, levels, rounds) of a named case: built and peeled once per process, arrays read-only"""
    n, (rp, ci) = CASES[name]()
    support, truss, rnd, levels, rounds, _ = ktruss(rp, ci, n)
    for a in (rp, ci, support, truss, rnd):
        a.setflags(write=False)
    return n, rp, ci, support, truss, rnd, levels, rounds
