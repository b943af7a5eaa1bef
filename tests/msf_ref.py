"""The reference of g4s_minimum_spanning_forest (include/g4s.h): Kruskal over the stored entries in the strict order (w, min(i,j), max(i,j), k) — −w under
`maximum`, −0.0 == +0.0 — with a plain union-find, in numpy and Python. It returns the ascending positions, the canonical labels and the weight, and it
holds the named graphs that tests/test_msf_cpu.py pins to scipy and networkx and that the GPU tests compare with ==. All weights of the named graphs are
integer-valued (or ±inf), so every sum is exact whatever its shape."""
import functools
import math

import numpy as np

PINNED = ("edges", "components", "weight")


def forest(n, rowptr, colids, values=None, maximum=False):
    """dict(positions int32, labels int32[n], edges, components, weight) of the forest; ValueError for a NaN."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    nnz = int(rowptr[n]) if n else 0
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    lo, hi = np.minimum(rows, colids[:nnz]), np.maximum(rows, colids[:nnz])
    if values is None:
        w = np.zeros(nnz)
    else:
        w = np.asarray(values, np.float64)[:nnz]
        if np.isnan(w).any():
            raise ValueError("a value is NaN")
        w = (-w if maximum else w) + 0.0                                 # −0.0 + 0.0 == +0.0
    order = np.lexsort((np.arange(nnz), hi, lo, w))                      # the last key is the first to decide
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    chosen = []
    lo_l, hi_l = lo.tolist(), hi.tolist()
    for k in order.tolist():
        a, b = find(lo_l[k]), find(hi_l[k])
        if a != b:
            parent[max(a, b)] = min(a, b)                                # the smaller id stays the root: the canonical label
            chosen.append(k)
    positions = np.array(sorted(chosen), np.int32)
    labels = np.array([find(v) for v in range(n)], np.int32)
    weight = 0.0
    if values is not None:
        for x in np.asarray(values, np.float64)[positions].tolist():     # ascending position order; exact for integer-valued weights
            weight += x
    return {"positions": positions, "labels": labels, "edges": int(positions.size), "components": n - int(positions.size), "weight": weight}


def same_weight(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))                   # +inf and −inf in one forest sum to NaN on both sides


def pairs(rowptr, colids, positions, n):
    """the forest as a set of (lo, hi) vertex pairs"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))
    p = np.asarray(positions, np.int64)
    c = np.asarray(colids, np.int64)
    return set(zip(np.minimum(rows[p], c[p]).tolist(), np.maximum(rows[p], c[p]).tolist()))


# ------------------------------------------------------------------------------------------------ graphs
def from_edges(n, src, dst, w=None, symmetric=True):
    """(n, rowptr, colids, values-or-None): a CSR of the edge list in the order given inside each row (rows need not be sorted, repeats stay);
    symmetric=True stores every edge in both directions."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    if symmetric:
        off = src != dst
        src, dst = np.concatenate([src, dst[off]]), np.concatenate([dst, src[off]])
        if w is not None:
            w = np.concatenate([np.asarray(w, np.float64), np.asarray(w, np.float64)[off]])
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    return n, rowptr, dst[order].astype(np.int32), None if w is None else np.asarray(w, np.float64)[order]


def _grid(side, w):
    idx = np.arange(side * side).reshape(side, side)
    src = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    dst = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return from_edges(side * side, src, dst, None if w is None else np.full(src.size, w))


def _clique(m, w, base=0):
    s, d = np.triu_indices(m, 1)
    return s + base, d + base, np.full(s.size, float(w))


def _path(n, kind):
    i = np.arange(n - 1)
    w = {"inc": i + 1.0, "dec": (n - i) * 1.0, "alt": (i % 2) * 1.0}[kind]
    return from_edges(n, i, i + 1, w)


def _star(m, tied):
    rng = np.random.default_rng(m)
    w = rng.permutation(m).astype(np.float64)
    if tied:
        w = np.floor(w / 2.0) % (m // 4)                                 # heavy ties
    return from_edges(m + 1, np.zeros(m, np.int64), np.arange(1, m + 1), w)


def _two_k6():
    s1, d1, w1 = _clique(6, 2.0)
    s2, d2, w2 = _clique(6, 2.0, 6)
    src = np.concatenate([s1, s2, [0, 5]])                               # two bridges: (0, 6) heavy, (5, 11) light
    dst = np.concatenate([d1, d2, [6, 11]])
    w = np.concatenate([w1 + np.arange(15), w2 + np.arange(15) % 3, [100.0, 1.0]])
    return from_edges(12, src, dst, w)


def _random(n, deg, kind, seed):
    from tests import helpers
    rp, ci, _ = helpers.random_csr(n, n, deg / n, seed)
    rng = np.random.default_rng(seed + 1)
    w = rng.integers(0, 8, ci.size) if kind == "ties" else rng.integers(0, 1 << 30, ci.size)
    return n, rp, ci, w.astype(np.float64)


def _triangle_parts(part):
    n, rp, ci, w = _random(300, 6.0, "distinct", 77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    up = rows < ci                                                       # the strict upper triangle of a random pattern is the graph
    s, d, x = rows[up], ci[up], w[up]
    if part == "upper":
        return from_edges(n, s, d, x, symmetric=False)
    if part == "lower":
        return from_edges(n, d, s, x, symmetric=False)
    return from_edges(n, s, d, x)


CASES = {
    "grid64_null": lambda: _grid(64, None),
    "grid64_ones": lambda: _grid(64, 1.0),
    "clique5_null": lambda: from_edges(5, *_clique(5, 1.0)[:2]),
    "clique5_ones": lambda: from_edges(5, *_clique(5, 1.0)),
    "path_inc": lambda: _path(5000, "inc"),
    "path_dec": lambda: _path(5000, "dec"),
    "path_alt": lambda: _path(5000, "alt"),
    **{f"star{m}": (lambda m=m: _star(m, False)) for m in (4095, 4096, 4097, 10000)},
    **{f"star{m}_tied": (lambda m=m: _star(m, True)) for m in (4095, 4096, 4097, 10000)},
    "two_k6": _two_k6,
    # the pair (0, 1) three times with different weights (the lightest, the last one stored, wins), beside a path
    "repeats_differ": lambda: from_edges(4, [0, 0, 0, 1, 2], [1, 1, 1, 2, 3], [5.0, 3.0, 2.0, 4.0, 4.0], symmetric=False),
    # with equal weights the smallest position wins
    "repeats_equal": lambda: from_edges(4, [0, 0, 0, 1, 2], [1, 1, 1, 2, 3], [3.0, 3.0, 3.0, 3.0, 3.0], symmetric=False),
    # self-loops lighter than everything else are never chosen
    "self_loops": lambda: from_edges(5, [0, 0, 1, 1, 2, 3, 3, 4], [0, 1, 1, 2, 2, 3, 4, 4], [-9.0, 2.0, -9.0, 3.0, -9.0, -9.0, 1.0, -9.0]),
    # vertices 0, 3, 7, 8, 9 have empty rows; 0, 7 and 9 are isolated
    "isolated": lambda: from_edges(10, [1, 2, 4, 5, 6], [2, 3, 5, 6, 8], [2.0, 1.0, 4.0, 3.0, 7.0], symmetric=False),
    "negative": lambda: from_edges(6, [0, 1, 2, 3, 4, 0, 1], [1, 2, 3, 4, 5, 5, 4], [-1.0, -5.0, 2.0, -3.0, 0.0, -2.0, -4.0]),
    "tri_upper": lambda: _triangle_parts("upper"),
    "tri_lower": lambda: _triangle_parts("lower"),
    "tri_full": lambda: _triangle_parts("full"),
}

# the named graphs whose weights are all distinct per vertex pair: the forest is unique as a set of pairs whatever the tie-break
DISTINCT = ("path_inc", "path_dec", "star4095", "star4097", "tri_upper", "tri_lower", "tri_full")

RANDOM = tuple((deg, kind) for deg in (0.5, 1.0, 2.0, 4.0) for kind in ("ties", "distinct"))


@functools.lru_cache(maxsize=None)
def case(name, maximum=False):
    """(n, rowptr, colids, values-or-None, reference dict) of a named graph; computed once and shared: treat the arrays as read-only."""
    n, rp, ci, w = CASES[name]()
    return n, rp, ci, w, forest(n, rp, ci, w, maximum)


@functools.lru_cache(maxsize=None)
def random_case(deg, kind):
    n, rp, ci, w = _random(50000, deg, kind, int(deg * 10) + (0 if kind == "ties" else 100))
    return n, rp, ci, w, forest(n, rp, ci, w)
