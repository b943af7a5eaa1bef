"""numpy reference of g4s_csr_from_coo_* (include/g4s.h): the stable (row, col, input index) order as one lexsort, head flags where the key changes, and
the duplicate policy as an explicit left-to-right loop over every run — not np.add.reduceat, whose order of summation is not promised."""
import numpy as np

DUPLICATES = ("keep", "plus", "times", "min", "max", "first", "second")

_FOLD = {
    "plus": lambda x, y: x + y,
    "times": lambda x, y: x * y,
    "min": lambda x, y: y if y < x else x,
    "max": lambda x, y: y if x < y else x,
    "first": lambda x, y: x,
    "second": lambda x, y: y,
}


def perm_of(row, col):
    """perm[p] = the input index of the p-th triple in (row, col, input index) order."""
    n = len(row)
    return np.lexsort((np.arange(n), np.asarray(col, np.int64), np.asarray(row, np.int64))).astype(np.int32)


def fold(dup, values):
    """acc = combine(acc, next) over `values` from left to right, in Python floats (IEEE doubles)."""
    f = _FOLD[dup]
    it = iter(values)
    acc = next(it)
    for x in it:
        acc = f(acc, x)
    return acc


def from_coo(row, col, val, rows, cols, dup="plus"):
    """(rowptr, colids, values-or-None, perm, longest_run) of the rows × cols CSR of the triples under the duplicate policy `dup`."""
    assert dup in DUPLICATES
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    n = len(row)
    assert n == 0 or (row.min() >= 0 and row.max() < rows and col.min() >= 0 and col.max() < cols)
    perm = perm_of(row, col)
    r, c = row[perm], col[perm]
    key = r * max(cols, 1) + c
    change = np.ones(n, bool)
    change[1:] = key[1:] != key[:-1]
    run_starts = np.flatnonzero(change)
    longest = int(np.diff(np.append(run_starts, n)).max()) if n else 0
    starts = np.arange(n) if dup == "keep" else run_starts
    ends = np.append(starts[1:], n)
    rowptr = np.zeros(rows + 1, np.int64)
    np.add.at(rowptr, r[starts] + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.int32)
    colids = c[starts].astype(np.int32)
    values = None
    if val is not None:
        v = np.asarray(val, np.float64)[perm].tolist()
        f = "first" if dup == "keep" else dup
        values = np.array([fold(f, v[s:e]) for s, e in zip(starts.tolist(), ends.tolist())], np.float64).reshape(-1)
    return rowptr, colids, values, perm, longest


def row_indices(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).astype(np.int32)
