"""numpy reference for g4s_connected_components: canonical labels (the smallest vertex id of each weakly connected component) by iterating
l := min(l, l[neighbours both ways], l[l]) to its fixed point, and the map from scipy's discovery-order labels to canonical ones."""
import numpy as np


def labels(rowptr, colids, n):
    """(labels int32[n], rounds): every stored entry (i, j) is an undirected edge, whatever its value."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    l = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        new = l.copy()
        if colids.size:
            np.minimum.at(new, src, l[colids])
            np.minimum.at(new, colids, l[src])
        new = np.minimum(new, new[new])                              # shortcut: labels are vertex ids
        rounds += 1
        if np.array_equal(new, l):
            return l.astype(np.int32), rounds
        l = new


def canonical(scipy_labels, n):
    """scipy's 0 … k−1 labels in discovery order → the smallest member of each component."""
    lab = np.asarray(scipy_labels, np.int64)
    if n == 0:
        return np.empty(0, np.int32)
    smallest = np.full(int(lab.max()) + 1, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n, dtype=np.int64))
    return smallest[lab].astype(np.int32)


def scipy_labels(rowptr, colids, n):
    """Canonicalised scipy.sparse.csgraph.connected_components(directed=True, connection="weak") of the pattern (all values 1.0)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    G = sp.csr_matrix((np.ones(len(colids)), np.asarray(colids), np.asarray(rowptr)), shape=(n, n))
    k, lab = connected_components(G, directed=True, connection="weak")
    return canonical(lab, n), k


def stats(lab):
    """(components, largest, largest_label) the way g4s_cc_info defines them."""
    lab = np.asarray(lab)
    if lab.size == 0:
        return 0, 0, 0
    cnt = np.bincount(lab)
    return int(np.unique(lab).size), int(cnt.max()), int(np.argmax(cnt))   # argmax: the first, i.e. smallest, label of that size
