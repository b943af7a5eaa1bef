"""The fixed, seeded problems of the concurrency tests (test_concurrency_cpu.py, concurrency_worker.py) and their expected results, numpy / scipy only.

Every value is a small integer, so every plus-times sum is exact in any order while Σ|a·b| per output entry stays below 2^53 (abs_sum_bound,
asserted by test_concurrency_cpu.py); min-plus, max-plus and or-and are exact anyway. Every comparison made with these cases is therefore ==.
The expected results come from the references of this directory: semiring_ref (products, _mul, _reduce — the products of a problem are expanded and
sorted once and reduced per semiring), masked_ref, components_ref, traverse_ref, spmv_semiring_ref and the oracle's SpMV."""
import functools

import numpy as np

from tests import components_ref, masked_ref, oracle_lib, semiring_ref, spmv_semiring_ref, traverse_ref
from tests.helpers import assemble_csr, hex_mesh, power_law_csr, spd_blocks

SEMIRINGS = semiring_ref.NAMES
ROUNDS = 8                    # rounds of every scenario: fixed, no loop until failure
THREADS = 6                   # host threads of the widest scenario
BARRIER_TIMEOUT = 30.0        # seconds a thread waits at a threading.Barrier for the others (a single call takes milliseconds); below every child's time
                              # limit in test_concurrency_gpu.py (asserted there), so a thread that never arrives ends the scenario with a difference


def ints(pattern, seed, lo=-4, hi=4, nonzero=False):
    """integer values in lo … hi for a (rowptr, colids[, values]) pattern, as test_spgemm_masked_gpu._ints"""
    v = np.random.default_rng(seed).integers(lo, hi + 1, len(pattern[1])).astype(np.float64)
    if nonzero:
        v[v == 0] = 1.0
    return np.ascontiguousarray(pattern[0], np.int32), np.ascontiguousarray(pattern[1], np.int32), v


def int_vector(seed, n, k=None):
    return np.random.default_rng(seed).integers(-4, 5, n if k is None else (n, k)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ SpGEMM-shaped problems: C = A·A on a power-law square
class Product:
    """One square problem A (n × n, integer values) with everything the scenarios compare against."""

    def __init__(self, name, n, seed, max_len):
        self.name, self.n = name, n
        self.A = ints(power_law_csr(n, n, seed, max_len), seed + 1000)
        self.A2 = (self.A[0], self.A[1], ints(self.A, seed + 2000)[2])            # the same pattern with other values (the time-stepping case)
        self.nnz = len(self.A[1])

    @functools.cached_property
    def _sorted_products(self):
        row, col, a, b = semiring_ref.products(self.A, self.A)
        order = np.lexsort((col, row))
        row, col = row[order], col[order]
        head = np.ones(row.size, bool)
        head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
        starts = np.flatnonzero(head)
        crpt = np.zeros(self.n + 1, np.int64)
        np.add.at(crpt, row[starts] + 1, 1)
        return order, starts, np.cumsum(crpt).astype(np.int32), col[starts].astype(np.int32)

    def _values(self, A, semiring, pattern_only=False):
        order, starts, _, _ = self._sorted_products
        if pattern_only:
            A = masked_ref._ones(A)
        _, _, a, b = semiring_ref.products(A, A)
        return semiring_ref._reduce(semiring, semiring_ref._mul(semiring, a, b)[order], starts)

    @property
    def crpt(self):
        return self._sorted_products[2]

    @property
    def ccol(self):
        return self._sorted_products[3]

    @property
    def cnnz(self):
        return int(self.crpt[-1])

    @functools.lru_cache(maxsize=None)
    def cval(self, semiring, second_values=False):
        return self._values(self.A2 if second_values else self.A, semiring)

    @functools.cached_property
    def abs_sum_bound(self):
        """max over the output entries of Σ|a·b| (both value sets): below 2^53 every plus-times sum is exact in any order"""
        absA = lambda A: (A[0], A[1], np.abs(A[2]))
        return float(max(self._values(absA(self.A), "plus_times").max(initial=0.0), self._values(absA(self.A2), "plus_times").max(initial=0.0)))

    @functools.cached_property
    def row_flop(self):
        lens = np.diff(self.A[0].astype(np.int64))
        flop = np.zeros(self.n, np.int64)
        np.add.at(flop, np.repeat(np.arange(self.n), lens), lens[self.A[1]])
        return flop

    # -- masked product on the mask A (C⟨A⟩ = A·A) and the triangle count
    @functools.lru_cache(maxsize=None)
    def masked(self, semiring, pattern_only=False):
        cval = self._values(self.A, semiring, pattern_only)
        n = np.int64(self.n)
        ckey = masked_ref.mask_rows(self.crpt) * n + self.ccol.astype(np.int64)
        mkey = masked_ref.mask_rows(self.A[0]) * n + self.A[1].astype(np.int64)
        pos = np.searchsorted(ckey, mkey)
        hit = pos < ckey.size
        hit[hit] = ckey[pos[hit]] == mkey[hit]
        out = np.full(mkey.size, masked_ref.IDENTITY[semiring], np.float64)
        out[hit] = cval[pos[hit]]
        return out

    @property
    def masked_products(self):
        """g4s_masked_info.products for the mask A: the products of the rows whose mask row is not empty (every non-empty row of A)"""
        return int(self.row_flop.sum())

    @functools.cached_property
    def graph(self):
        """the simple undirected graph of the pattern (sorted rows, no diagonal): the input of g4s_triangle_count"""
        G = masked_ref.symmetric_simple_graph(self.A[0], self.A[1], self.n)
        return G.indptr.astype(np.int32), G.indices.astype(np.int32)

    @functools.cached_property
    def triangles(self):
        rp, ci = self.graph
        import scipy.sparse as sp
        return masked_ref.triangles_lower(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(self.n, self.n)))

    # -- components, transpose, SpMV, traversal
    @functools.cached_property
    def labels(self):
        return components_ref.labels(self.A[0], self.A[1], self.n)[0]

    @functools.cached_property
    def cc_stats(self):
        return components_ref.stats(self.labels)

    @functools.cached_property
    def transpose(self):
        trp, tci, tva = traverse_ref.transpose(*self.A, self.n)
        return trp, tci, tva, np.argsort(self.A[1], kind="stable").astype(np.int32)

    @functools.cached_property
    def x(self):
        return int_vector(self.n + 7, self.n)

    @functools.cached_property
    def y0(self):
        return int_vector(self.n + 8, self.n)

    @functools.cached_property
    def spmv(self):
        """y = 2·A·x − 3·y0 (integers throughout)"""
        return oracle_lib.load().spmv(*self.A, self.x, self.y0, 2.0, -3.0)

    @functools.cached_property
    def weights(self):
        """the graph of the traversals: the same pattern with weights 1 … 5 (no negative cycle), and the source: the longest row"""
        return (self.A[0], self.A[1], np.abs(self.A[2]) + 1.0), int(np.argmax(np.diff(self.A[0])))

    @functools.cached_property
    def sssp(self):
        W, src = self.weights
        return traverse_ref.sssp(*W, self.n, [src])[0]

    @functools.cached_property
    def bfs(self):
        """levels over the edges with a value != 0 (A's own values: about one entry in nine is a stored zero)"""
        return traverse_ref.bfs(*self.A, self.n, [self.weights[1]])[0]


@functools.lru_cache(maxsize=None)
def products():
    """Three power-law squares; every operation of threads_synchronous_calls runs on all three (schedule). The first two have the same shape (the
    in-place scenario rewrites one into the other) and outputs within 25 % of each other (a cached output block freed by one fits the other); the
    third is also the 'large enough' product two threads run behind a barrier."""
    return (Product("pl13a", 1 << 13, 23, 600), Product("pl13b", 1 << 13, 31, 600), Product("pl14", 1 << 14, 47, 1500))


# ------------------------------------------------------------------------------------------------ the mixes of scenario threads_synchronous_calls
# the calls a thread's mix is drawn from, in the order of concurrency_worker.OPS (sssp and bfs run on the handle the thread owns: problem t % 3)
OP_NAMES = ("onecall_dev plus_times", "masked min_plus", "components device", "two_call plus_times", "sssp", "onecall_host min_plus", "masked plus_times",
            "transpose", "triangles", "onecall_dev min_plus", "masked or_and", "spmv_host", "two_call max_plus", "components host",
            "masked plus_times pattern", "bfs", "masked max_plus", "create_destroy_blocked", "onecall_host plus_times")
OPS_PER_ROUND = 5
STRIDES = (1, 5, 7, 11, 13, 17)                                      # one per thread, all coprime to len(OP_NAMES) = 19


def schedule(t):
    """thread t's mix: ROUNDS lists of (index into OP_NAMES, index into products()). Its own stride through the calls, phase-shifted, so that a problem
    is in different threads at different times; over the six threads every call meets every one of the three problems
    (test_concurrency_cpu.test_every_call_runs_on_every_problem)."""
    return [[((t * 3 + q * STRIDES[t]) % len(OP_NAMES), (q + t) % 3) for q in range(r * OPS_PER_ROUND, (r + 1) * OPS_PER_ROUND)] for r in range(ROUNDS)]


# ------------------------------------------------------------------------------------------------ the four SpMV paths (scenario handles_on_streams)
def _rmat_pattern(scale, edge_factor, seed):
    n = 1 << scale
    keys = np.unique(oracle_lib.load().rmat_keys(seed, scale, n, 0, edge_factor * n))
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, keys // n + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), (keys % n).astype(np.int32)


class Handle:
    """A square matrix for one SpMV path, with per-round inputs and the expected result of the four enqueued calls."""
    K = 8

    def __init__(self, path, pattern, seed):
        self.path, self.seed = path, seed
        self.A = pattern if len(pattern) == 3 else ints(pattern, seed, nonzero=True)
        self.n = len(self.A[0]) - 1

    @functools.cached_property
    def AT(self):
        return traverse_ref.transpose(*self.A, self.n)

    def inputs(self, r):
        s = self.seed * 100 + r
        return {"x": int_vector(s, self.n), "X": int_vector(s + 1, self.n, self.K), "y_acc": int_vector(s + 2, self.n), "xt": int_vector(s + 3, self.n)}

    def expected(self, r):
        o, i = oracle_lib.load(), self.inputs(r)
        return {"spmv": o.spmv(*self.A, i["x"]),
                "spmm": np.stack([o.spmv(*self.A, np.ascontiguousarray(i["X"][:, j])) for j in range(self.K)], axis=1),
                "min_plus_acc": spmv_semiring_ref.spmv(*self.A, i["x"], "min_plus", y=i["y_acc"]),
                "transpose": o.spmv(*self.AT, i["xt"])}

    @functools.cached_property
    def abs_sum_bound(self):
        o = oracle_lib.load()
        absA = (self.A[0], self.A[1], np.abs(self.A[2]))
        return float(max(o.spmv(*absA, np.full(self.n, 4.0)).max(), o.spmv(self.AT[0], self.AT[1], np.abs(self.AT[2]), np.full(self.n, 4.0)).max()))


SPMV_PATHS = {"stream": 0, "blocked": 1, "diagonal": 3, "block_row": 4}


@functools.lru_cache(maxsize=None)
def handles():
    """stream and blocked: R-MAT 2^16 (forced by flag); diagonal: the 7-point Laplacian on 32 × 32 × 16; block-row: an assembled hexahedral FE matrix"""
    ien, idmap, _, neq = hex_mesh(16, 14, 12)
    fe = assemble_csr(ien, idmap, spd_blocks(len(ien), 24, 3), neq)
    return (Handle("stream", _rmat_pattern(16, 12, 5), 11), Handle("blocked", _rmat_pattern(16, 12, 6), 12),
            Handle("diagonal", oracle_lib.load().laplacian7(32, 32, 16), 13), Handle("block_row", (fe[0], fe[1]), 14))


# ------------------------------------------------------------------------------------------------ invalid inputs (scenario errors_stay_with_their_thread)
def invalid_inputs():
    """(bad colids for g4s_connected_components, an unsorted mask for g4s_spgemm_masked) built from the first problem"""
    P = products()[0]
    bad_ci = P.A[1].copy()
    bad_ci[len(bad_ci) // 2] = P.n                                   # one column id outside [0, n)
    r = int(np.argmax(np.diff(P.A[0])))                              # the longest row: swap its first two ids
    bad_mask = P.A[1].copy()
    k = P.A[0][r]
    bad_mask[[k, k + 1]] = bad_mask[[k + 1, k]]
    return bad_ci, bad_mask
