"""numpy reference for g4s_color: the first-fit colouring in decreasing priority that include/g4s.h defines, restated on the host level by level, and
the graphs the tests share.

Priority: the pair (key[v], fmix32(v ^ seed)) compared lexicographically, larger first; fmix32 is the murmur3 finaliser, a bijection on 32 bits, so
the order is strict. color[v] = the smallest colour not held by a neighbour above v; round[v] = 0 when no neighbour is above v, else 1 + the largest
round among those neighbours; overflow = the vertices whose neighbours above them hold all of the colours 0 … 63. tests/test_color_cpu.py pins the
colours against networkx.greedy_color with the explicit order on every case, so the yardstick of the GPU tests rests on something this project did not
write.

The graphs are those of tests/kcore_ref.py plus three named for what they hit in the overflow path (clique64_hub, clique65_hub, clique_window)."""
import functools

import numpy as np

from tests import kcore_ref

MASK_COLORS = 64
ORDERS = ("hash", "largest_first", "smallest_last", "reverse_id")


def fmix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def priority(n, key=None, seed=0):
    """one uint64 per vertex that compares as the pair (key, hash) does: the key moved to [0, 2^32) in the high half"""
    h = fmix32(np.arange(n, dtype=np.uint64) ^ np.uint64(seed & 0xFFFFFFFF)).astype(np.uint64)
    k = np.zeros(n, np.int64) if key is None else np.asarray(key, np.int64)
    return ((k + 2**31).astype(np.uint64) << np.uint64(32)) | h


def order(n, key=None, seed=0):
    """the vertices in decreasing priority: the sequence a sequential greedy colouring visits"""
    return np.argsort(priority(n, key, seed), kind="stable")[::-1]


def color(rp, ci, n, key=None, seed=0):
    """(color, round, overflow) of the symmetric pattern (rp, ci) under the priority (key, seed)"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    prio = priority(n, key, seed)
    rows = kcore_ref._row_ids(rp, n)
    down = (ci != rows) & (prio[rows] > prio[ci])                     # the entries u → w from a vertex to a neighbour below it, in row order
    src, dst = rows[down], ci[down]
    dp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=dp[1:])
    pred = np.bincount(dst, minlength=n)
    col, rnd = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    used = np.zeros((n, 8), bool)                                     # used[v, c]: a neighbour above v holds colour c; the last column stays clear
    front = np.flatnonzero(pred == 0)
    overflow = r = 0
    while front.size:
        c = np.argmin(used[front], axis=1)                            # the first clear column
        col[front], rnd[front] = c, r
        overflow += int(np.count_nonzero(c >= MASK_COLORS))
        if c.max() + 2 > used.shape[1]:
            used = np.concatenate([used, np.zeros((n, max(used.shape[1], int(c.max()) + 2 - used.shape[1])), bool)], axis=1)
        e = kcore_ref._entries_of(dp, front)
        w = dst[e]
        used[w, col[src[e]]] = True
        touched, count = np.unique(w, return_counts=True)
        pred[touched] -= count
        front = touched[pred[touched] == 0]
        r += 1
    return col, rnd, overflow


def networkx_color(rp, ci, n, key=None, seed=0):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    rows = kcore_ref._row_ids(np.asarray(rp, np.int64), n)
    off = np.asarray(ci) != rows
    G.add_edges_from(zip(rows[off].tolist(), np.asarray(ci)[off].tolist()))
    seq = order(n, key, seed).tolist()
    c = nx.greedy_color(G, strategy=lambda g, colors: seq)
    return np.array([c[v] for v in range(n)], np.int32)


def higher_neighbours(rp, ci, n, key=None, seed=0):
    """per vertex: how many neighbours (itself excluded) are above it"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    prio = priority(n, key, seed)
    rows = kcore_ref._row_ids(rp, n)
    return np.bincount(rows[(ci != rows) & (prio[ci] > prio[rows])], minlength=n)


def is_proper(rp, ci, n, col):
    rows = kcore_ref._row_ids(np.asarray(rp, np.int64), n)
    off = np.asarray(ci) != rows
    return bool(np.all(col[rows[off]] != col[np.asarray(ci)[off]]))


def class0_is_maximal_independent(rp, ci, n, col):
    rows = kcore_ref._row_ids(np.asarray(rp, np.int64), n)
    ci = np.asarray(ci)
    off = ci != rows
    zero = col == 0
    inside = np.bincount(rows[off & zero[ci]], minlength=n)          # neighbours in class 0
    return bool(np.all(inside[zero] == 0) and np.all(inside[~zero] > 0))


def classes(col):
    """(perm, offsets): the vertices sorted by (colour, id), and where each class starts"""
    perm = np.argsort(col, kind="stable").astype(np.int32)
    offsets = np.zeros(int(col.max()) + 2 if col.size else 1, np.int64)
    if col.size:
        np.cumsum(np.bincount(col), out=offsets[1:])
    return perm, offsets


# ------------------------------------------------------------------------------------------------ graphs
def clique_hub(clique, leaves=5000):
    """K_clique on the vertices 0 … clique − 1, then a hub adjacent to all of them and to `leaves` leaves. The hub has key 0 and the rest key 1, so the hub
    is coloured last, behind a mask that the clique has filled; its row is above the hub cut of the walk."""
    hub = clique
    n = clique + 1 + leaves
    spokes = np.concatenate([np.arange(clique), np.arange(hub + 1, n)])
    e = np.concatenate([kcore_ref.clique_edges(np.arange(clique)), np.stack([np.full(spokes.size, hub, np.int64), spokes], 1)])
    key = np.ones(n, np.int32)
    key[hub] = 0
    return n, kcore_ref.from_edges(n, e), key


def clique64_hub():
    return clique_hub(64)


def clique65_hub():
    return clique_hub(65)


def clique_window(window):
    """K_m with m = 64 + window + 1: the vertex coloured last needs the second window of the row scan; the colours are the ranks in priority order"""
    m = MASK_COLORS + window + 1
    return m, kcore_ref.from_edges(m, kcore_ref.clique_edges(np.arange(m))), None


HUB_CASES = {"clique64_hub": clique64_hub, "clique65_hub": clique65_hub}
CASES = tuple(sorted(kcore_ref.CASES)) + tuple(sorted(HUB_CASES))


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, rowptr, colids, own key or None) of a named case, arrays read-only"""
    if name in HUB_CASES:
        n, (rp, ci), key = HUB_CASES[name]()
        key.setflags(write=False)
    else:
        n, rp, ci = kcore_ref.case(name)[:3]
        key = None
    for a in (rp, ci):
        a.setflags(write=False)
    return n, rp, ci, key


@functools.lru_cache(maxsize=None)
def keys(name, how):
    """the key array of an order on a named case (None for the hash order), and whether the call computes it itself (largest-first)"""
    n, rp, ci, own = graph(name)
    if how == "hash":
        return None
    if how == "own":
        return own
    if how == "largest_first":
        key = kcore_ref.degrees(rp, ci, n).astype(np.int32)
    elif how == "smallest_last":
        key = kcore_ref.kcore(rp, ci, n)[1].astype(np.int32)
    elif how == "reverse_id":
        key = (n - 1 - np.arange(n)).astype(np.int32)
    else:
        raise KeyError(how)
    key.setflags(write=False)
    return key


@functools.lru_cache(maxsize=None)
def case(name, how, seed=0):
    """(n, rowptr, colids, key, color, round, overflow) of a named case under a named order: coloured once per process, arrays read-only"""
    n, rp, ci, _ = graph(name)
    key = keys(name, how)
    col, rnd, over = color(rp, ci, n, key, seed)
    for a in (col, rnd):
        a.setflags(write=False)
    return n, rp, ci, key, col, rnd, over


def orders_of(name):
    return ORDERS + (("own",) if name in HUB_CASES else ())
