"""numpy reference of g4s_csr_extract_* (include/g4s.h): C = A[I, J] as a direct loop — per output row, collect (q, e) over the inverse lists of J for
every stored entry e of the source row, then sort. The order inside an output row is (q, stored position of the source entry)."""
import numpy as np


def extract(rowptr, colids, values, rows, cols, I=None, J=None):
    """(crpt, ccol, cval-or-None, src) of A[I, J]; I / J None: every row / every column in order. src[x]: the index into colids / values behind entry x."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    I = np.arange(rows) if I is None else np.asarray(I, np.int64)
    J = np.arange(cols) if J is None else np.asarray(J, np.int64)
    assert len(rowptr) == rows + 1
    assert len(I) == 0 or (I.min() >= 0 and I.max() < rows)
    assert len(J) == 0 or (J.min() >= 0 and J.max() < cols)
    inverse = [[] for _ in range(cols)]                                 # inverse[c]: the q with J[q] == c
    for q, c in enumerate(J.tolist()):
        inverse[c].append(q)
    crpt, ccol, src = [0], [], []
    for r in I.tolist():
        pairs = []
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            pairs += [(q, e) for q in inverse[int(colids[e])]]
        pairs.sort()                                                    # (q, e): e ascends with the stored position inside the row
        ccol += [q for q, _ in pairs]
        src += [e for _, e in pairs]
        crpt.append(len(ccol))
    src = np.array(src, np.int32).reshape(-1)
    cval = None if values is None else np.asarray(values, np.float64)[src]
    return np.array(crpt, np.int32), np.array(ccol, np.int32).reshape(-1), cval, src
