"""The problems of tests/test_cg_loop_gpu.py and their references (numpy only; tests/test_cg_ref_cpu.py asserts the preconditions without a GPU).

Every problem is a dict: n, BI, bc (sorted int32 boundary equations, a random ninth), F (zero on bc), csr = (rowptr, colids, values) of the operator the
references multiply with, plus what the device operator is created from. reference(p) runs tests/cg_ref.conj_grad once per number format with
acc = 0 and MAX_IT iterations and keeps every iterate: with acc = 0 a solve capped at k is the first k iterations of that run."""
import numpy as np

from tests import cg_ref
from tests.helpers import assemble_csr, hex_mesh, spd_blocks

CAPS = (0, 1, 2, 3, 4, 7, 12)
MAX_IT = 12
STOP_AT = (2, 5, 9)
CSR_SIZES = (1, 255, 256, 257, 65536, 65537, 150001)              # 1 … 257: the zero-fill of unused partial-sum slots; the last three: the grid-stride loops wrap
BAND_NX = 31

_cache = {}


def band_problem(n):
    """SPD band with offsets {−nx, −1, 0, 1, nx}: symmetric off-diagonals in [−1, 0), diagonal = 1.5·Σ|off| + U(0, 1) (strictly diagonally dominant,
    so Jacobi-CG contracts by a factor ≈ 0.3 per iteration)."""
    key = ("band", n)
    if key in _cache:
        return _cache[key]
    import scipy.sparse as sp
    rng = np.random.default_rng(7000 + n)
    rows, cols, vals = [], [], []
    for off in (1, BAND_NX):
        if n > off:
            w = -rng.uniform(0.0, 1.0, n - off) - 2.0 ** -60           # [−1, 0): never zero
            i = np.arange(n - off)
            rows += [i, i + off]; cols += [i + off, i]; vals += [w, w]
    offsum = np.zeros(n)
    for r, v in zip(rows, vals):
        np.add.at(offsum, r, np.abs(v))
    diag = 1.5 * offsum + rng.uniform(0.0, 1.0, n)
    rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(diag)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sort_indices()
    bc = np.sort(rng.choice(n, n // 9, replace=False)).astype(np.int32)
    F = rng.uniform(-1, 1, n)
    F[bc] = 0.0
    p = {"name": f"band{n}", "n": n, "BI": 1.0 / diag, "bc": bc, "F": F,
         "csr": (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64))}
    _cache[key] = p
    return p


def elem_problem(ex, ey, ez, seed, oracle):
    """The element-operator problem of tests/test_cg_gpu.py (_setup) with the oracle's inverse diagonal."""
    key = ("elem", ex, ey, ez, seed)
    if key in _cache:
        return _cache[key]
    ien, idmap, nno, neq = hex_mesh(ex, ey, ez)
    K = spd_blocks(len(ien), 24, seed)
    rng = np.random.default_rng(seed)
    bc = np.array(sorted(set(idmap[rng.choice(nno, max(1, nno // 9), replace=False)].ravel().tolist())), np.int32)
    F = rng.uniform(-1, 1, neq)
    F[bc] = 0.0
    p = {"name": f"elem{neq}", "n": neq, "BI": oracle.element_inverse_diagonal(ien, idmap, K, neq), "bc": bc, "F": F, "csr": assemble_csr(ien, idmap, K, neq),
         "ien": ien, "idmap": idmap, "nno": nno, "K": K}
    _cache[key] = p
    return p


def node_problem(oracle):
    """The node-assembled operator on hex_mesh(8, 8, 4) (_problem of tests/test_nodeop_gpu.py). The direction vectors of CG vanish on the boundary
    equations (F does, and the boundary rows of Ap are zeroed), so K·p is the same product with or without the boundary columns the node form drops:
    the references multiply with the assembled K."""
    key = ("node",)
    if key in _cache:
        return _cache[key]
    from tests.test_nodeop_gpu import _problem
    ien, idmap, nno, neq, K, nm, max_eqn, bc, ks, rng = _problem(oracle, 8, 8, 4, 2)
    F = rng.uniform(-1, 1, neq)
    F[bc] = 0.0
    p = {"name": f"node{neq}", "n": neq, "BI": oracle.element_inverse_diagonal(ien, idmap, K, neq), "bc": bc, "F": F, "csr": assemble_csr(ien, idmap, K, neq),
         "idmap": idmap, "nno": nno, "nm": nm, "max_eqn": max_eqn, "ks": ks}
    _cache[key] = p
    return p


def dist_problem(oracle):
    """The 12×10×6 problem of tests/test_dist_cg_gpu.py (_problem) with BI = 1/diag of the assembled matrix, as that test passes it."""
    key = ("dist",)
    if key in _cache:
        return _cache[key]
    ien, idmap, nno, neq = hex_mesh(12, 10, 6)
    K = spd_blocks(len(ien), 24, 11)
    rng = np.random.default_rng(11)
    bc = np.array(sorted(set(idmap[rng.choice(nno, nno // 9, replace=False)].ravel().tolist())), np.int32)
    F = rng.uniform(-1, 1, neq)
    F[bc] = 0.0
    rp, ci, va = assemble_csr(ien, idmap, K, neq)
    diag = np.array([va[rp[r] + np.searchsorted(ci[rp[r]:rp[r + 1]], r)] for r in range(neq)])
    p = {"name": f"dist{neq}", "n": neq, "BI": 1.0 / diag, "bc": bc, "F": F, "csr": (rp, ci, va)}
    _cache[key] = p
    return p


class Reference:
    """Two runs of cg_ref.conj_grad on one problem: ld (np.longdouble, the reference) and f64 (np.float64, the second summation order)."""

    def __init__(self, p, acc=0.0, steps=MAX_IT, bc=None, F=None):
        bc = p["bc"] if bc is None else bc
        F = p["F"] if F is None else F
        run = lambda dt: cg_ref.conj_grad(cg_ref.csr_matvec(*p["csr"], dt), p["BI"], bc, F, acc, steps, dt, keep_iterates=True)
        self.ld, self.f64 = run(np.longdouble), run(np.float64)
        self.count = self.ld[1]

    def gap_d0(self, k):
        """gap of the stripped iterate after k iterations (k >= 1)"""
        return cg_ref.rel_gap(self.f64[4][k - 1], self.ld[4][k - 1])

    def gap_res(self, k):
        return cg_ref.rel_gap(self.f64[3][k - 1], self.ld[3][k - 1])

    def iterate(self, k):
        return self.ld[4][k - 1]

    def residual(self, k):
        return self.ld[3][k - 1]


def reference(p):
    """The acc = 0, MAX_IT-iteration reference of a problem, computed once."""
    key = ("ref", p["name"])
    if key not in _cache:
        _cache[key] = Reference(p)
    return _cache[key]


def comparable(p, k):
    """An iterate can be compared only while the Krylov space is not exhausted: after n iterations the exact residual is zero and what a further
    iteration does is decided by round-off alone (n = 1 reaches that at k = 2)."""
    return max(k, 1) <= p["n"]


def comparable_residual(p, k):
    """The residual after n iterations is zero in exact arithmetic: what a run computes there is its own round-off, |r| <= a few ulp of |F|."""
    return max(k, 1) < p["n"]
