"""Value reference for the SpGEMM semirings (include/g4s.h, G4S_SEMIRING_*), numpy only: every product expanded, sorted by (row, column),
then reduced per output entry. min, max and or do not depend on the order of the products, so the device must match this bit for bit."""
import numpy as np

NAMES = ("plus_times", "min_plus", "max_plus", "or_and")


def _mul(name, a, b):
    if name == "plus_times":
        return a * b
    if name in ("min_plus", "max_plus"):
        return a + b
    return ((a != 0) & (b != 0)).astype(np.float64)          # std::logical_and as 1.0 / 0.0; NaN counts as nonzero


def _reduce(name, v, starts):
    if name == "min_plus":
        return np.minimum.reduceat(v, starts)
    if name in ("max_plus", "or_and"):
        return np.maximum.reduceat(v, starts)
    return np.add.reduceat(v, starts)


def products(A, B):
    """(row, column, a, b) of every product of A·B in CSR (repeated columns inside a row included)."""
    arp, aci, ava = (np.asarray(x) for x in A)
    brp, bci, bva = (np.asarray(x) for x in B)
    M = len(arp) - 1
    arow = np.repeat(np.arange(M, dtype=np.int64), np.diff(arp))
    blen = (brp[1:] - brp[:-1]).astype(np.int64)[aci]
    total = int(blen.sum())
    first = np.repeat(brp[aci].astype(np.int64), blen)
    off = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(blen) - blen, blen)
    k = first + off
    return np.repeat(arow, blen), bci[k].astype(np.int64), np.repeat(ava, blen), bva[k]


def spgemm(A, B, M, semiring):
    """C = A·B over the semiring: (crpt int32, ccol int32, cval float64), rows sorted by column."""
    row, col, a, b = products(A, B)
    v = _mul(semiring, a, b)
    order = np.lexsort((col, row))
    row, col, v = row[order], col[order], v[order]
    if row.size == 0:
        return np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    head = np.ones(row.size, bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    starts = np.flatnonzero(head)
    crow, ccol = row[starts], col[starts]
    cval = _reduce(semiring, v, starts)
    crpt = np.zeros(M + 1, np.int64)
    np.add.at(crpt, crow + 1, 1)
    return np.cumsum(crpt).astype(np.int32), ccol.astype(np.int32), cval


def same_values(c, ref):
    """Exact equality with −0 and +0 taken as equal (the sign of a zero min/max-plus result is outside the contract)."""
    return np.array_equal(np.asarray(c) + 0.0, np.asarray(ref) + 0.0, equal_nan=False)
