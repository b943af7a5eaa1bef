"""numpy oracle of g4s_csr_ewise_* and g4s_csr_select_* (include/g4s.h). A stored position is an entry whatever its value, so the pattern comes from set
operations on the keys row·cols + col (int64) and the values from searchsorted — never from scipy's A + B, which drops results equal to zero.
test_ewise_cpu.py pins it to scipy on inputs where no result is zero. Rows of the inputs of ewise() are strictly ascending; select() takes any order."""
import numpy as np

OPS = ("union", "intersect", "difference")
COMBINERS = ("plus", "times", "min", "max", "first", "second")
PREDICATES = ("tril", "triu", "offdiag", "diag", "nonzero", "gt", "ge", "lt", "le")


def row_of_entry(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def keys(rowptr, colids, cols):
    return row_of_entry(rowptr) * np.int64(max(cols, 1)) + np.asarray(colids, np.int64)


def combine_values(name, x, y):
    if name == "plus":
        return x + y
    if name == "times":
        return x * y
    if name == "min":
        return np.where(y < x, y, x)
    if name == "max":
        return np.where(x < y, y, x)
    if name == "first":
        return x.copy()
    if name == "second":
        return y.copy()
    raise ValueError(name)


def _find(k, kc):
    """(found, index): where every key of kc sits in the ascending keys k."""
    i = np.minimum(np.searchsorted(k, kc), max(len(k) - 1, 0))
    found = (k[i] == kc) if len(k) else np.zeros(len(kc), bool)
    return found, i


def ewise(a, b, rows, cols, op="union", combine="plus"):
    """(rowptr int32, colids int32, values float64) of A op B; a and b are (rowptr, colids, values) triples with strictly ascending rows."""
    ka, kb = keys(a[0], a[1], cols), keys(b[0], b[1], cols)
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0), "the oracle needs strictly ascending rows"
    va, vb = np.asarray(a[2], np.float64), np.asarray(b[2], np.float64)
    if op == "union":
        kc = np.union1d(ka, kb)
    elif op == "intersect":
        kc = np.intersect1d(ka, kb, assume_unique=True)
    elif op == "difference":
        kc = np.setdiff1d(ka, kb, assume_unique=True)
    else:
        raise ValueError(op)
    in_a, ia = _find(ka, kc)
    in_b, ib = _find(kb, kc)
    out = np.empty(len(kc), np.float64)
    both = in_a & in_b
    out[both] = combine_values(combine, va[ia[both]], vb[ib[both]])
    out[in_a & ~in_b] = va[ia[in_a & ~in_b]]
    out[in_b & ~in_a] = vb[ib[in_b & ~in_a]]
    w = np.int64(max(cols, 1))
    rowptr = np.zeros(rows + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(kc // w, minlength=rows)[:rows]) if rows else 0
    return rowptr.astype(np.int32), (kc % w).astype(np.int32), out


def select_mask(rowptr, colids, values, pred, k=0, thr=0.0):
    d = np.asarray(colids, np.int64) - row_of_entry(rowptr)
    if pred == "tril":
        return d <= k
    if pred == "triu":
        return d >= k
    if pred == "offdiag":
        return d != 0
    if pred == "diag":
        return d == 0
    v = np.asarray(values, np.float64)
    with np.errstate(invalid="ignore"):
        if pred == "nonzero":
            return v != 0
        if pred == "gt":
            return v > thr
        if pred == "ge":
            return v >= thr
        if pred == "lt":
            return v < thr
        if pred == "le":
            return v <= thr
    raise ValueError(pred)


def select(a, rows, pred, k=0, thr=0.0):
    """(rowptr, colids, values) of the entries of a = (rowptr, colids, values-or-None) that satisfy pred, in stored order."""
    rp, ci, va = a
    m = select_mask(rp, ci, va, pred, k, thr)
    rowptr = np.zeros(rows + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row_of_entry(rp)[m], minlength=rows)[:rows]) if rows else 0
    return rowptr.astype(np.int32), np.asarray(ci, np.int32)[m], None if va is None else np.asarray(va, np.float64)[m]


def transpose(a, rows, cols):
    """Aᵀ with ascending rows (stable), as a triple."""
    rp, ci, va = a
    order = np.argsort(np.asarray(ci, np.int64), kind="stable")
    trp = np.zeros(cols + 1, np.int64)
    trp[1:] = np.cumsum(np.bincount(np.asarray(ci, np.int64), minlength=cols))
    return trp.astype(np.int32), row_of_entry(rp)[order].astype(np.int32), np.asarray(va, np.float64)[order]
