"""numpy / scipy reference for g4s_strongly_connected_components, and the graphs its tests share.

Labels: scipy.sparse.csgraph.connected_components(connection="strong"), made canonical (the smallest vertex id of each component); networkx in
tests/test_scc_cpu.py. The counts of g4s_scc_info that are functions of the graph — trimmed, pivot, pivot_size, color_rounds — come from `route`, a
plain restatement of the route include/g4s.h fixes: trim to the fixpoint, one pivot (largest din·dout, smallest id at ties) by forward and backward
reach, colouring rounds (colour = the smallest id that reaches a vertex; the vertices that keep their own id are roots; backward reach inside a
colour), every removal followed by trimming. The simulation labels on its own, and tests/test_scc_cpu.py holds it against scipy on every case."""
import functools

import numpy as np

from tests.kcore_ref import _entries_of, rmat_edges


def csr_of_edges(n, edges):
    """(rowptr, colids) of the directed edges (m × 2: start, end) in the order given inside each row: repeats and self-loops stay, nothing is sorted"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.argsort(e[:, 0], kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=rp[1:])
    return rp.astype(np.int32), e[order, 1].astype(np.int32)


def transpose(rp, ci, n):
    """(trowptr, tcolids) as g4s_csr_transpose gives them: stable, so repeats stay"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    return csr_of_edges(n, np.stack([np.asarray(ci, np.int64), rows], 1))


def canonical(comp):
    """labels[v] = the smallest vertex id among the vertices that share comp[v]"""
    comp = np.asarray(comp)
    first = np.full(int(comp.max()) + 1 if comp.size else 0, comp.size, np.int64)
    np.minimum.at(first, comp, np.arange(comp.size))
    return first[comp].astype(np.int32)


def scipy_labels(rp, ci, n):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(len(ci), np.int8), np.asarray(ci), np.asarray(rp)), shape=(n, n))
    return canonical(connected_components(A, directed=True, connection="strong")[1])


def networkx_labels(rp, ci, n):
    import networkx as nx
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.repeat(np.arange(n), np.diff(rp)).tolist(), np.asarray(ci).tolist()))
    lab = np.empty(n, np.int32)
    for comp in nx.strongly_connected_components(G):
        lab[list(comp)] = min(comp)
    return lab


def stats(labels):
    """(components, largest, largest_label) as g4s_scc_info counts them: ties go to the smaller label"""
    roots, size = np.unique(labels, return_counts=True)
    if roots.size == 0:
        return 0, 0, 0
    k = int(np.argmax(size))                                          # the first maximum: the smallest label
    return int(roots.size), int(size[k]), int(roots[k])


def _reach(rp, ci, start, allowed):
    """(mask of the vertices reached from `start` through `allowed` vertices, steps that walked a non-empty frontier)"""
    seen = np.zeros(allowed.size, bool)
    seen[start] = True
    front, steps = np.asarray(start, np.int64), 0
    while front.size:
        steps += 1
        nb = np.unique(ci[_entries_of(rp, front)])
        front = nb[allowed[nb] & ~seen[nb]]
        seen[front] = True
    return seen, steps


def route(rp, ci, n):
    """dict: labels, trimmed, pivot, pivot_size, color_rounds of the fixed route, and what the tests assert of a case's shape: trim_frontiers (sizes
    of the frontiers of the first trimming), reach_steps (forward, backward), roots (per colouring round)"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    trp, tci = (np.asarray(a, np.int64) for a in transpose(rp, ci, n))
    rows, trows = np.repeat(np.arange(n), np.diff(rp)), np.repeat(np.arange(n), np.diff(trp))
    dout = np.bincount(rows[ci != rows], minlength=n).astype(np.int64)    # stored off-diagonal entries, repeats counted
    din = np.bincount(trows[tci != trows], minlength=n).astype(np.int64)
    labels = np.full(n, -1, np.int32)
    live = np.ones(n, bool)
    out = {"trimmed": 0, "pivot": -1, "pivot_size": 0, "color_rounds": 0, "trim_frontiers": [], "reach_steps": (0, 0), "roots": []}

    def remove(front, sizes=None):
        """`front` is labelled: take it out and trim to the fixpoint"""
        while front.size:
            live[front] = False
            for ptr, ids, counter in ((rp, ci, din), (trp, tci, dout)):
                k = _entries_of(ptr, front)
                other = ids[k]
                other = other[other != np.repeat(front, ptr[front + 1] - ptr[front])]
                np.subtract.at(counter, other, 1)
            front = np.flatnonzero(live & ((din <= 0) | (dout <= 0)))
            labels[front] = front
            out["trimmed"] += int(front.size)
            if sizes is not None and front.size:
                sizes.append(int(front.size))

    first = np.flatnonzero((din == 0) | (dout == 0))
    labels[first] = first
    out["trimmed"] += int(first.size)
    if first.size:
        out["trim_frontiers"].append(int(first.size))
    remove(first, out["trim_frontiers"])
    if live.any():
        prod = np.where(live, din * dout, -1)
        p = int(np.flatnonzero(prod == prod.max())[0])
        fwd, fs = _reach(rp, ci, [p], live)
        bwd, bs = _reach(trp, tci, [p], live & fwd)
        comp = np.flatnonzero(fwd & bwd)
        labels[comp] = comp[0]
        out.update(pivot=p, pivot_size=int(comp.size), reach_steps=(fs, bs))
        remove(comp)
    while live.any():
        out["color_rounds"] += 1
        colour = np.arange(n)
        keep = live[rows] & live[ci]
        u, w = rows[keep], ci[keep]
        while True:
            before = colour.copy()
            np.minimum.at(colour, w, colour[u])
            if np.array_equal(before, colour):
                break
        roots = np.flatnonzero(live & (colour == np.arange(n)))
        out["roots"].append(int(roots.size))
        labels[roots] = roots
        front, claimed = roots, [roots]
        while front.size:
            k = _entries_of(trp, front)
            src, c = tci[k], np.repeat(colour[front], trp[front + 1] - trp[front])
            ok = live[src] & (labels[src] == -1) & (colour[src] == c)
            front = np.unique(src[ok])
            labels[front] = colour[front]
            claimed.append(front)
        remove(np.concatenate(claimed))
    out["labels"] = labels
    return out


# ------------------------------------------------------------------------------------------------ graphs
def _ring(ids):
    ids = np.asarray(ids, np.int64)
    return np.stack([ids, np.roll(ids, -1)], 1)


def _spokes(hub, leaves, out=True, back=True):
    leaves = np.asarray(leaves, np.int64)
    h = np.full(leaves.size, hub, np.int64)
    return np.concatenate(([np.stack([h, leaves], 1)] if out else []) + ([np.stack([leaves, h], 1)] if back else []))


def tiny():
    """0: alone with a self-loop; 1 ⇄ 2 with 1 → 2 stored twice; 2 → 3 the bridge; 3 → 4 → 5 → 3 with row 5 unsorted (a chord 5 → 4); 6: an empty
    row; 7: its only out-edge is a self-loop; 8 → 9"""
    rows = [[0], [2, 2, 7], [1, 3], [4], [5, 6], [4, 3], [], [7], [9], []]
    return 10, csr_of_edges(10, [(u, v) for u, r in enumerate(rows) for v in r])


TINY_LABELS = [0, 1, 1, 3, 3, 3, 6, 7, 8, 9]


def cycle(n=2049):
    return n, csr_of_edges(n, _ring(np.arange(n)))


def path(n=1500):
    return n, csr_of_edges(n, np.stack([np.arange(n - 1), np.arange(1, n)], 1))


def hub_cycle(leaves=5000):
    return leaves + 1, csr_of_edges(leaves + 1, _spokes(0, np.arange(1, leaves + 1)))


def hub_out(leaves=5000):
    return leaves + 1, csr_of_edges(leaves + 1, _spokes(0, np.arange(1, leaves + 1), back=False))


def funnel(closed, leaves=5000):
    mid = np.arange(2, leaves + 2)
    e = [_spokes(0, mid, back=False), _spokes(1, mid, out=False)] + ([np.array([[1, 0]])] if closed else [])
    return leaves + 2, csr_of_edges(leaves + 2, np.concatenate(e))


def two_hubs(leaves=5000):
    m = leaves + 1
    return 2 * m, csr_of_edges(2 * m, np.concatenate([_spokes(0, np.arange(1, m)), _spokes(m, np.arange(m + 1, 2 * m))]))


def two_cycles(length=1000):
    n = 2 * length
    return n, csr_of_edges(n, np.concatenate([_ring(np.arange(0, n, 2)), _ring(np.arange(1, n, 2)), np.array([[0, 1]])]))


def chain(count=40, upstream=False):
    """`count` three-cycles {3i, 3i + 1, 3i + 2} in a line; a bridge 3i + 2 → 3(i + 1), or with upstream 3(i + 1) + 2 → 3i"""
    e = [_ring(np.arange(3 * i, 3 * i + 3)) for i in range(count)]
    i = np.arange(count - 1)
    e.append(np.stack([3 * (i + 1) + 2, 3 * i], 1) if upstream else np.stack([3 * i + 2, 3 * (i + 1)], 1))
    return 3 * count, csr_of_edges(3 * count, np.concatenate(e))


def cycles_dag(cycles=300, extra=600, tails=200, seed=20240614):
    """cycles of length 2 … 40 with a chord each (where there is room), `extra` edges from a lower-numbered cycle to a higher one, `tails` vertices with
    one edge into a cycle and `tails` with one edge out of one; every id under one random permutation"""
    rng = np.random.default_rng(seed)
    length = rng.integers(2, 41, cycles)
    start = np.concatenate([[0], np.cumsum(length)])
    n = int(start[-1]) + 2 * tails
    e = []
    for c in range(cycles):
        ids = np.arange(start[c], start[c + 1])
        e.append(_ring(ids))
        if ids.size >= 4:
            a, b = rng.choice(ids.size, 2, replace=False)
            e.append(np.array([[ids[a], ids[b]]]))
    member = lambda c: start[c] + rng.integers(0, length[c])
    for _ in range(extra):
        a, b = np.sort(rng.choice(cycles, 2, replace=False))
        e.append(np.array([[member(a), member(b)]]))
    for t in range(tails):
        e.append(np.array([[start[-1] + t, member(rng.integers(cycles))]]))
        e.append(np.array([[member(rng.integers(cycles)), start[-1] + tails + t]]))
    e = rng.permutation(n)[np.concatenate(e)]
    return n, csr_of_edges(n, e[rng.permutation(len(e))])


def rmat13():
    """R-MAT of scale 13, edge factor 4, as drawn: directed, self-loops and repeats stored, rows unsorted"""
    return 1 << 13, csr_of_edges(1 << 13, rmat_edges(13, 4, 20240613))


def er(n=4096, m=6144, seed=20240615):
    rng = np.random.default_rng(seed)
    return n, csr_of_edges(n, rng.integers(0, n, (m, 2)))


def doubling_out_tree(depth=17):
    """root 0, v → 2v + 1 and 2v + 2 down to `depth`, every leaf → 0: one component whose forward reach doubles each step"""
    n = (1 << (depth + 1)) - 1
    v = np.arange((1 << depth) - 1)
    leaves = np.arange((1 << depth) - 1, n)
    return n, csr_of_edges(n, np.concatenate([np.stack([v, 2 * v + 1], 1), np.stack([v, 2 * v + 2], 1), np.stack([leaves, np.zeros(leaves.size, np.int64)], 1)]))


CASES = {"tiny": tiny, "cycle": cycle, "path": path, "hub_cycle": hub_cycle, "hub_out": hub_out, "funnel_closed": lambda: funnel(True),
         "funnel_open": lambda: funnel(False), "two_hubs": two_hubs, "two_cycles": two_cycles, "chain40": chain, "chain40rev": lambda: chain(upstream=True),
         "cycles_dag": cycles_dag, "rmat13": rmat13, "er": er}

PINNED = ("components", "largest", "largest_label", "trimmed", "pivot", "pivot_size", "color_rounds")   # the fields of g4s_scc_info that the graph fixes


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, rowptr, colids, trowptr, tcolids, route dict with the PINNED fields filled in) of a named case (or "doubling_out_tree"): built once per
    process, arrays read-only"""
    n, (rp, ci) = (doubling_out_tree if name == "doubling_out_tree" else CASES[name])()
    trp, tci = transpose(rp, ci, n)
    r = route(rp, ci, n)
    r["components"], r["largest"], r["largest_label"] = stats(r["labels"])
    for a in (rp, ci, trp, tci, r["labels"]):
        a.setflags(write=False)
    return n, rp, ci, trp, tci, r
