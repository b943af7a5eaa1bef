"""Value reference for the masked SpGEMM C⟨M⟩ = A ⊗ B (include/g4s.h, g4s_spgemm_masked) and for triangle counting, numpy / scipy only.
The masked product is the full semiring product of tests/semiring_ref.py, looked up at every mask entry by a search over its sorted (row, column)
keys; a mask entry the full product does not have gets the semiring's identity. Triangles: trace(G³) / 6 and Σ (L·L) ∘ L with scipy."""
import numpy as np
import scipy.sparse as sp

from tests import semiring_ref

IDENTITY = {"plus_times": 0.0, "min_plus": np.inf, "max_plus": -np.inf, "or_and": 0.0}


def _ones(A):
    return A[0], A[1], np.ones(len(A[1]), np.float64)


def mask_rows(mrpt):
    mrpt = np.asarray(mrpt)
    return np.repeat(np.arange(len(mrpt) - 1, dtype=np.int64), np.diff(mrpt))


def spgemm_masked(A, B, M, N, mask, semiring, pattern_only=False):
    """(cval, hit): the value of every mask entry and whether the full product has an entry there. A, B = (rowptr, colids, values);
    mask = (mrpt, mcol). pattern_only: every stored value of A and B counts as 1.0."""
    if pattern_only:
        A, B = _ones(A), _ones(B)
    crpt, ccol, cval = semiring_ref.spgemm(A, B, M, semiring)
    ckey = mask_rows(crpt) * np.int64(N) + ccol.astype(np.int64)                 # ascending: rows of the reference are sorted by column
    mrpt, mcol = (np.asarray(x) for x in mask)
    mkey = mask_rows(mrpt) * np.int64(N) + mcol.astype(np.int64)
    pos = np.searchsorted(ckey, mkey)
    hit = pos < ckey.size
    hit[hit] = ckey[pos[hit]] == mkey[hit]
    out = np.full(mkey.size, IDENTITY[semiring], np.float64)
    out[hit] = cval[pos[hit]]
    return out, hit


def abs_sums(A, B, M, N, mask):
    """Σ |a·b| per mask entry: the scale of the plus-times bound 1e-10·Σ|a·b|."""
    absA, absB = (A[0], A[1], np.abs(A[2])), (B[0], B[1], np.abs(B[2]))
    return spgemm_masked(absA, absB, M, N, mask, "plus_times")[0]


def symmetric_simple_graph(rowptr, colids, n):
    """The simple undirected graph of a square pattern: G = pattern(A + Aᵀ) without the diagonal, as a scipy CSR of ones with sorted rows."""
    A = sp.csr_matrix((np.ones(len(colids)), np.asarray(colids), np.asarray(rowptr)), shape=(n, n))
    G = (A + A.T).tocsr()
    G.setdiag(0)
    G.eliminate_zeros()
    G.data[:] = 1.0
    G.sort_indices()
    return G


def triangles_trace(G):
    """trace(G³) / 6 for a symmetric 0/1 matrix without a diagonal."""
    G2 = (G @ G).tocsr()
    return int(round(G2.multiply(G.T).sum())) // 6


def triangles_lower(G):
    """Σ (L·L) ∘ L, L the strictly lower triangle of the pattern of G."""
    L = sp.tril(G, k=-1).tocsr()
    L.data[:] = 1.0
    return int(round((L @ L).multiply(L).sum()))
