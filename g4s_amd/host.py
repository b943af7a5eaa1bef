"""Host-side mirror of the reference's interface for the hot path, over device-resident buffers.

Names and argument meaning follow the reference so that tests read like tests of the reference would:
  CSR            — mm/inc/CSR.h:22-100 (rows, cols, nnz, rowptr, colids, values, zerobased)
  HashSpGEMM     — mm/inc/hash_mult.h:1028-1057 (sortOutput flag; multiply/add: plus-times, min-plus, max-plus or or-and)
  spmv           — the CSR mat-vec the build defines for mv/ (DESIGN.md §SpMV), y = alpha·A·x + beta·y
  spmv_semiring  — the same over min-plus, max-plus or or-and (SEMIRINGS): y = A ⊗ x, or y ⊕ (A ⊗ x)
  spmm           — the same with a dense block of k vectors, Y = alpha·A·X + beta·Y (the sparse form of mm/src/cblas_dxxmm.c)
  csr_transpose  — Aᵀ as a CSR (the CSC form of A; mm/inc/CSR.h:171-230, mm/inc/convert.h), stable: entries of a column keep their order
  csr_from_coo   — a CSR from an edge list in any order, repeats merged by a duplicate policy (CSR(graph&), mm/inc/CSR.h:255-329); csr_row_indices /
                   CSR.to_coo the way back, csr_canonical a CSR with sorted rows and merged repeats
  csr_extract    — C = A[I, J] for id lists in any order, with repeats (g4s_csr_extract_*; the block constructor mm/inc/CSR.h:691-733 and CSC::SpRef,
                   mm/inc/CSC.h:513-690); csr_permute, csr_induced_subgraph and csr_submatrix are compositions of it
  spgemm_masked  — C⟨M⟩ = A ⊗ B at the positions of a given pattern M only (g4s_spgemm_masked); triangle_count: Σ (L·L⟨L⟩) of the lower triangle
  connected_components — canonical labels (smallest member id) of the weakly connected components of a pattern (g4s_connected_components)
  strongly_connected_components — canonical labels of the strongly connected components of a directed pattern (g4s_strongly_connected_components);
                   compact_labels (labels → 0 … k−1) and condensation (the DAG of the components) are compositions of existing device calls
  minimum_spanning_forest — the positions of the entries of the minimum / maximum spanning forest of a weighted undirected graph
                   (g4s_minimum_spanning_forest); spanning_forest_csr (the forest as a CSR) is a composition of existing device calls
  ktruss         — truss numbers, peel rounds and supports of the edges of a symmetric pattern (g4s_ktruss); ktruss_subgraph is a composition of it
  sptrsv_analyse — the plan of a level-scheduled triangular solve on the lower or upper triangle of a square CSR (g4s_sptrsv_*): solve, update_values;
                   spsolve_triangular is the one-shot form with scipy's meaning, gauss_seidel a sweep built from two plans and g4s_spmv
  ilu0           — the ILU(0) factorisation of a square CSR with canonical rows and its apply z = U⁻¹ L⁻¹ r (g4s_ilu0_*): apply, factor, factors;
                   pcg is a preconditioned CG wired from g4s_spmv, that apply and torch
  kcore          — core numbers and the peel order of a symmetric pattern (g4s_kcore); degeneracy_order and kcore_subgraph are compositions of it
  color          — greedy colouring in a priority order (g4s_color); color_smallest_last, maximal_independent_set and color_classes go with it
  sssp / bfs     — shortest paths / BFS levels from a set of sources on a graph stored by out-edges (g4s_sssp, g4s_bfs): one call, the loop on the device
  pagerank       — PageRank of a graph stored by out-edges (g4s_pagerank): one call, the loop, the dangling mass and the stop test on the device
  betweenness    — betweenness centrality from a list of sources (g4s_betweenness): Brandes' two sweeps per source, both on the device
  spmv_transpose — y = alpha·Aᵀ·x + beta·y on a handle of A (spmv_semiring_transpose: the semiring form), through the handle's own transpose
Everything here calls the C-ABI (libg4s_hip.so); torch tensors only hold device memory. No CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else C.c_void_p(0)


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("g4s_amd.host needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")


class CSR:
    """Device-resident CSR<int32, fp64> with the reference's field names (mm/inc/CSR.h:92-99)."""

    def __init__(self, rowptr, colids, values, rows, cols, spmv_flags=0):
        _require_gpu()
        assert rowptr.dtype == torch.int32 and colids.dtype == torch.int32 and values.dtype == torch.float64
        assert rowptr.is_cuda and colids.is_cuda and values.is_cuda
        assert rowptr.numel() == rows + 1 and colids.numel() == values.numel()
        self.rows, self.cols, self.nnz = int(rows), int(cols), int(colids.numel())
        self.rowptr, self.colids, self.values = rowptr.contiguous(), colids.contiguous(), values.contiguous()
        self.zerobased = True
        self._spmv_flags = spmv_flags
        self._handle = None

    @classmethod
    def from_host(cls, rowptr, colids, values, rows, cols, device="cuda", **kw):
        _require_gpu()
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        return cls(t(rowptr, np.int32), t(colids, np.int32), t(values, np.float64), rows, cols, **kw)

    def to_host(self):
        return self.rowptr.cpu().numpy(), self.colids.cpu().numpy(), self.values.cpu().numpy()

    # -- SpMV plan handle (g4s_csr_create with borrowed device arrays)
    @property
    def handle(self):
        if self._handle is None:
            lib = capi.load()
            h = C.c_void_p()
            # g4s_csr_create reads the borrowed arrays on the NULL stream: whatever torch stream filled them must be complete first
            torch.cuda.current_stream().synchronize()
            capi.check(lib.g4s_csr_create(C.byref(h), self.rows, self.cols, self.nnz, _ptr(self.rowptr), _ptr(self.colids),
                                          _ptr(self.values), capi.DEVICE_POINTERS | self._spmv_flags))
            self._handle = h
        return self._handle

    def info(self):
        inf = capi.CsrInfo()
        capi.check(capi.load().g4s_csr_get_info(self.handle, C.byref(inf)))
        return {n: getattr(inf, n) for n, _ in capi.CsrInfo._fields_}

    def spmv(self, x, y=None, alpha=1.0, beta=0.0):
        """y = alpha·A·x + beta·y on the current torch stream (asynchronous)."""
        assert x.dtype == torch.float64 and x.is_cuda and x.numel() == self.cols
        if y is None:
            assert beta == 0.0
            y = torch.empty(self.rows, dtype=torch.float64, device=x.device)
        assert y.dtype == torch.float64 and y.numel() == self.rows
        capi.check(capi.load().g4s_spmv(self.handle, _ptr(x), _ptr(y), float(alpha), float(beta), _stream()))
        return y

    def spmv_semiring(self, x, y=None, semiring="min_plus", accumulate=False):
        """y := A ⊗ x, or y := y ⊕ (A ⊗ x) with accumulate=True, over `semiring` (a name of SEMIRINGS; include/g4s.h, g4s_spmv_semiring), on the current
        torch stream (asynchronous). min_plus: min(a + x), max_plus: max(a + x), or_and: 1.0 where any a != 0 and x != 0, else 0.0; an empty row gets the
        identity (+inf, −inf, 0.0), or leaves y unchanged when accumulating. plus_times is spmv(x, y, 1, accumulate ? 1 : 0)."""
        flags = _spmv_semiring_flags(semiring, accumulate, y)
        assert x.dtype == torch.float64 and x.is_cuda and x.numel() == self.cols
        if y is None:
            y = torch.empty(self.rows, dtype=torch.float64, device=x.device)
        assert y.dtype == torch.float64 and y.is_cuda and y.numel() == self.rows
        capi.check(capi.load().g4s_spmv_semiring(self.handle, _ptr(x), _ptr(y), flags, _stream()))
        return y

    def transpose(self):
        """Aᵀ as a new CSR (cols × rows) with the same spmv_flags, built on the device by g4s_csr_transpose (stable: see csr_transpose)."""
        trp, tci, tva = csr_transpose(self.rowptr, self.colids, self.values, self.rows, self.cols)
        return CSR(trp, tci, tva, self.cols, self.rows, spmv_flags=self._spmv_flags)

    def transpose_reserve(self):
        """Build the handle's transpose now (g4s_csr_transpose_reserve; synchronous), so that transposed products only enqueue kernels — before a capture."""
        torch.cuda.current_stream().synchronize()
        capi.check(capi.load().g4s_csr_transpose_reserve(self.handle))

    def transpose_info(self):
        """g4s_csr_transpose_info: the info of the handle's Aᵀ (its spmv_path, plan_bytes with the transpose's arrays, …); an error before a reserve."""
        inf = capi.CsrInfo()
        capi.check(capi.load().g4s_csr_transpose_info(self.handle, C.byref(inf)))
        return {n: getattr(inf, n) for n, _ in capi.CsrInfo._fields_}

    def spmv_transpose(self, x, y=None, alpha=1.0, beta=0.0):
        """y = alpha·Aᵀ·x + beta·y (x: rows, y: cols) on the current torch stream (asynchronous once the transpose exists; the first call reserves it)."""
        assert x.dtype == torch.float64 and x.is_cuda and x.numel() == self.rows
        if y is None:
            assert beta == 0.0
            y = torch.empty(self.cols, dtype=torch.float64, device=x.device)
        assert y.dtype == torch.float64 and y.is_cuda and y.numel() == self.cols
        capi.check(capi.load().g4s_spmv_transpose(self.handle, _ptr(x), _ptr(y), float(alpha), float(beta), _stream()))
        return y

    def spmv_semiring_transpose(self, x, y=None, semiring="min_plus", accumulate=False):
        """y := Aᵀ ⊗ x, or y ⊕ (Aᵀ ⊗ x) with accumulate=True (x: rows, y: cols) — spmv_semiring with Aᵀ: pull-style relaxation on a graph stored by
        out-edges, without a second matrix."""
        flags = _spmv_semiring_flags(semiring, accumulate, y)
        assert x.dtype == torch.float64 and x.is_cuda and x.numel() == self.rows
        if y is None:
            y = torch.empty(self.cols, dtype=torch.float64, device=x.device)
        assert y.dtype == torch.float64 and y.is_cuda and y.numel() == self.cols
        capi.check(capi.load().g4s_spmv_semiring_transpose(self.handle, _ptr(x), _ptr(y), flags, _stream()))
        return y

    def traverse_reserve(self, symmetric=False, direction="auto"):
        """Build now what sssp / bfs need (g4s_csr_traverse_reserve; synchronous): the workspace and — unless symmetric or direction="push" — Aᵀ."""
        flags = _traverse_flags(direction, symmetric)
        torch.cuda.current_stream().synchronize()
        capi.check(capi.load().g4s_csr_traverse_reserve(self.handle, flags))

    def _traverse(self, fn, sources, out, cap, direction, symmetric):
        flags = _traverse_flags(direction, symmetric)
        src = np.ascontiguousarray(np.atleast_1d(np.asarray(sources)), dtype=np.int32)
        info = capi.TraverseInfo()
        capi.check(getattr(capi.load(), fn)(self.handle, C.c_void_p(src.ctypes.data), int(src.size), _ptr(out), int(cap), flags, C.byref(info), _stream()))
        return out, {n: getattr(info, n) for n, _ in capi.TraverseInfo._fields_ if n != "reserved"}

    def sssp(self, sources, max_iterations=0, direction="auto", symmetric=False):
        """Shortest-path distances from the nearest of `sources` (vertex ids; an int or a sequence) over the edges i → j of row i, weight a_ij
        (g4s_sssp): (float64 tensor of rows, +inf where unreached; info dict). Exact: the min-plus fixed point, the same bits for every direction
        ("auto", "push", "pull"). max_iterations=0: rows. symmetric=True declares A == Aᵀ, so no transpose is built. Synchronous."""
        _traverse_flags(direction, symmetric)
        return self._traverse("g4s_sssp", sources, torch.empty(self.rows, dtype=torch.float64, device=self.rowptr.device), max_iterations, direction, symmetric)

    def bfs(self, sources, max_depth=0, direction="auto", symmetric=False):
        """BFS levels from `sources` (g4s_bfs): (int32 tensor of rows, −1 where unreached; info dict). A stored entry is an edge when it is != 0.
        max_depth=0: no cap. Synchronous."""
        _traverse_flags(direction, symmetric)
        return self._traverse("g4s_bfs", sources, torch.empty(self.rows, dtype=torch.int32, device=self.rowptr.device), max_depth, direction, symmetric)

    def pagerank_reserve(self, symmetric=False):
        """Build now what pagerank needs (g4s_csr_pagerank_reserve; synchronous): the workspace, the out-strengths and — unless symmetric — Aᵀ."""
        flags = _pagerank_args(0.85, 1e-10, 0, None, None, symmetric, self)
        torch.cuda.current_stream().synchronize()
        capi.check(capi.load().g4s_csr_pagerank_reserve(self.handle, flags & capi.PAGERANK_SYMMETRIC))

    def pagerank(self, damping=0.85, tol=1e-10, max_iterations=0, personalization=None, start=None, symmetric=False):
        """PageRank of the graph this matrix stores by out-edges (row u: the edges u → v, weight a_uv >= 0; g4s_pagerank): (float64 tensor of rows
        that sums to 1; info dict). networkx's pagerank with dangling = personalization: r' = damping·(Aᵀ(r / s) + m·p) + (1 − damping)·p with s the
        out-strengths, m the rank of the dangling vertices and p = personalization / Σ (float64 device tensor of rows, >= 0; None: uniform). Stops
        after the first iteration with Σ|r' − r| < tol, or at max_iterations (0: 100). start: a float64 device tensor to iterate from (normalised
        inside; it is not modified); None: p. symmetric=True declares A == Aᵀ, so no transpose is built. Synchronous. ValueError before any GPU
        call for bad arguments."""
        flags = _pagerank_args(damping, tol, max_iterations, personalization, start, symmetric, self)
        rank = torch.empty(self.rows, dtype=torch.float64, device=self.rowptr.device) if start is None else start.clone()
        pers = None if personalization is None else personalization.contiguous()
        info = capi.PagerankInfo()
        capi.check(capi.load().g4s_pagerank(self.handle, float(damping), float(tol), int(max_iterations), _ptr(pers), _ptr_nn(rank), flags, C.byref(info),
                                            _stream()))
        return rank, {n: getattr(info, n) for n, _ in capi.PagerankInfo._fields_}

    def betweenness_reserve(self):
        """Build now what betweenness needs (g4s_csr_betweenness_reserve; synchronous): the workspace and the verdict on stored zeros. No transpose."""
        if self.rows != self.cols:
            raise ValueError(f"betweenness needs a square matrix, not {self.rows} x {self.cols}")
        torch.cuda.current_stream().synchronize()
        capi.check(capi.load().g4s_csr_betweenness_reserve(self.handle, 0))

    def betweenness(self, sources, scale=1.0, out=None, accumulate=False):
        """Betweenness centrality of the graph this matrix stores by out-edges, from `sources` (vertex ids; an int or a sequence — each one is a
        traversal, a repeated one counts twice; g4s_betweenness): (float64 tensor of rows; info dict). bc[v] = scale · Σ_s δ_s(v) with Brandes'
        dependencies δ_s: the sum over s of networkx's betweenness_centrality_subset(G, [s], G, normalized=False). An entry is an edge when it is
        != 0, repeated columns are parallel edges. accumulate=True adds to `out` (a float64 device tensor of rows, required then) instead of
        overwriting it. Bit-for-bit reproducible while info["sigma_exact"] == 1. Synchronous. ValueError before any GPU call for bad arguments; a
        path count beyond the range of a double raises G4SError with status ERR_OVERFLOW."""
        src, flags = _betweenness_args(sources, scale, out, accumulate, self)
        bc = torch.empty(self.rows, dtype=torch.float64, device=self.rowptr.device) if out is None else out
        info = capi.BcInfo()
        capi.check(capi.load().g4s_betweenness(self.handle, C.c_void_p(src.ctypes.data), int(src.size), float(scale), _ptr_nn(bc), flags, C.byref(info), _stream()))
        return bc, {n: getattr(info, n) for n, _ in capi.BcInfo._fields_}

    def triangle_count(self, return_info=False):
        """The triangles of the graph whose symmetric pattern (or lower triangle) this matrix stores — triangle_count(self)."""
        return triangle_count(self, return_info)

    def connected_components(self, symmetric=False, return_info=False):
        """Canonical labels of the weakly connected components of this square pattern — connected_components(self). Needs no plan: the handle
        is not touched."""
        return connected_components(self, symmetric, return_info)

    def strongly_connected_components(self, transpose=None, return_info=False):
        """Canonical labels of the strongly connected components of the directed graph this matrix stores by out-edges —
        strongly_connected_components(self, …). Needs no plan."""
        return strongly_connected_components(self, transpose, return_info)

    def minimum_spanning_forest(self, maximum=False, return_labels=False):
        """The positions of the entries of the minimum (maximum) spanning forest of the undirected graph this matrix stores, weights = values —
        minimum_spanning_forest(self, …). Needs no plan."""
        return minimum_spanning_forest(self, maximum, return_labels)

    def triangular_plan(self, lower=True, unit_diagonal=False, return_level=False):
        """The plan of a triangular solve on this matrix's lower or upper triangle — sptrsv_analyse(self, …). It keeps its own copy of the triangle."""
        return sptrsv_analyse(self, lower, unit_diagonal, return_level)

    def ilu0(self):
        """The ILU(0) factorisation of this matrix (canonical rows, every diagonal entry stored) — ilu0(self). It keeps its own copy."""
        return ilu0(self)

    def kcore(self, max_k=None, return_round=False, return_info=False):
        """Core numbers (and the peel rounds) of the graph whose symmetric pattern this matrix stores — kcore(self, …). Needs no plan."""
        return kcore(self, max_k, return_round, return_info)

    def ktruss(self, max_k=None, return_round=False, return_support=False, return_info=False):
        """Truss numbers (and the peel rounds and supports) of the edges of the graph whose symmetric pattern this matrix stores, one per stored entry —
        ktruss(self, …). Needs no plan."""
        return ktruss(self, max_k, return_round, return_support, return_info)

    def color(self, key=None, seed=0, largest_first=False, return_round=False, return_info=False):
        """The first-fit colouring in decreasing priority (key, hash) of the graph whose symmetric pattern this matrix stores — color(self, …)."""
        return color(self, key, seed, largest_first, return_round, return_info)

    def ewise(self, other, op="union", combine="plus", pattern_only=False, return_info=False):
        """self ∪ other, self ∩ other or self ∖ other as a new device CSR — csr_ewise(self, other, …)."""
        return csr_ewise(self, other, op, combine, pattern_only, return_info)

    def select(self, pred, k=0, thr=0.0):
        """The entries of this matrix that satisfy `pred`, in their stored order, as a new device CSR — csr_select(self, …)."""
        return csr_select(self, pred, k, thr)

    def symmetrise(self, combine="max", drop_diagonal=False):
        """A ∪ Aᵀ of this square matrix as a new device CSR — csr_symmetrise(self, …)."""
        return csr_symmetrise(self, combine, drop_diagonal)

    @classmethod
    def from_coo(cls, row, col, val=None, rows=None, cols=None, dup="plus", symmetric=False, **kw):
        """A device CSR from the triples (row, col, val) — csr_from_coo(…); val=None stores 1.0 everywhere. kw: as for the constructor."""
        _require_gpu()
        rows, cols = _coo_shape(row, col, rows, cols, symmetric)
        rp, ci, va = csr_from_coo(row, col, val, rows, cols, dup, symmetric)
        if va is None:
            va = torch.ones(ci.numel(), dtype=torch.float64, device=ci.device)
        return cls(rp, ci, va, rows, cols, **kw)

    def to_coo(self):
        """(row, col, val) of the stored entries in stored order: csr_row_indices(self.rowptr, self.nnz) beside colids and values (borrowed)."""
        return csr_row_indices(self.rowptr, self.nnz), self.colids, self.values

    def canonical(self, dup="plus"):
        """This matrix with sorted rows and merged repeats as a new device CSR — csr_canonical(self, dup)."""
        return csr_canonical(self, dup)

    def extract(self, I=None, J=None, pattern_only=False, return_src=False, return_info=False):
        """self[I, J] as a new device CSR — csr_extract(self, …)."""
        return csr_extract(self, I, J, pattern_only, return_src, return_info)

    def permute(self, perm):
        """self[perm, perm] of this square matrix — csr_permute(self, perm)."""
        return csr_permute(self, perm)

    def induced_subgraph(self, vertices):
        """(self[ids, ids], ids) for an id tensor or a bool mask — csr_induced_subgraph(self, vertices)."""
        return csr_induced_subgraph(self, vertices)

    def submatrix(self, M, N, M_start=0, N_start=0):
        """The M × N block at (M_start, N_start) — csr_submatrix(self, …)."""
        return csr_submatrix(self, M, N, M_start, N_start)

    def spmm(self, X, Y=None, alpha=1.0, beta=0.0):
        """Y = alpha·A·X + beta·Y for a 2-D float64 device tensor X of cols × k, on the current torch stream (asynchronous). Row-major when
        X.stride(1) == 1, column-major when X.stride(0) == 1 (k > 1); the leading dimension is the other stride, Y has X's layout. A new Y
        (beta == 0) is allocated in X's layout."""
        assert X.dtype == torch.float64 and X.is_cuda and X.dim() == 2 and X.shape[0] == self.cols
        k = X.shape[1]
        if Y is None:
            assert beta == 0.0
            Y = torch.empty(k, self.rows, dtype=torch.float64, device=X.device).t() if X.stride(0) == 1 and k > 1 and X.stride(1) != 1 else \
                torch.empty(self.rows, k, dtype=torch.float64, device=X.device)
        assert Y.dtype == torch.float64 and Y.is_cuda and Y.dim() == 2 and tuple(Y.shape) == (self.rows, k)
        if k == 0 or self.rows == 0:
            return Y
        cm = False                                                  # row-major when both blocks are, else column-major when both are
        ldx, ldy = _spmm_ld(X, False), _spmm_ld(Y, False)
        if ldx is None or ldy is None:
            cm = True
            ldx, ldy = _spmm_ld(X, True), _spmm_ld(Y, True)
        if ldx is None or ldy is None:
            raise ValueError(f"X and Y must both be row-major (stride(1) == 1) or both column-major (stride(0) == 1); strides {tuple(X.stride())}, {tuple(Y.stride())}")
        flags = capi.SPMM_COL_MAJOR if cm else 0
        capi.check(capi.load().g4s_spmm(self.handle, k, _ptr(X), ldx, _ptr(Y), ldy, float(alpha), float(beta), flags, _stream()))
        return Y

    def spmm_reserve(self, k_max):
        """Build now what spmm needs for up to k_max vectors (synchronous), so that later calls never allocate — before a stream capture."""
        capi.check(capi.load().g4s_csr_spmm_reserve(self.handle, int(k_max)))

    def update_values(self, values):
        """New values for the same pattern (g4s_csr_update_values), in place: `values` (device tensor, nnz doubles) replaces self.values — the handle borrows
        the tensor's memory from here on — and the plan's own copy is refreshed on the current torch stream."""
        assert values.dtype == torch.float64 and values.is_cuda and values.numel() == self.nnz
        self.values = values
        if self._handle is not None:
            capi.check(capi.load().g4s_csr_update_values(self._handle, _ptr(values), capi.DEVICE_POINTERS, _stream()))

    def close(self):
        if self._handle is not None:
            capi.load().g4s_csr_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spmv(A, x, y=None, alpha=1.0, beta=0.0):
    return A.spmv(x, y, alpha, beta)


def _spmv_semiring_flags(semiring, accumulate, y):
    """The flags of g4s_spmv_semiring; ValueError (before any GPU call) for an unknown name or for accumulating into no y."""
    if semiring not in SEMIRINGS:
        raise ValueError(f"unknown semiring {semiring!r}; expected one of {sorted(SEMIRINGS)}")
    if accumulate and y is None:
        raise ValueError("accumulate=True needs the y to combine with (y is None)")
    return SEMIRINGS[semiring] | (capi.SPMV_ACCUMULATE if accumulate else 0)


def spmv_semiring(A, x, y=None, semiring="min_plus", accumulate=False):
    """y := A ⊗ x or y ⊕ (A ⊗ x) over a semiring (g4s_spmv_semiring) — CSR.spmv_semiring as a function, like spmv."""
    _spmv_semiring_flags(semiring, accumulate, y)
    return A.spmv_semiring(x, y, semiring, accumulate)


def spmv_transpose(A, x, y=None, alpha=1.0, beta=0.0):
    """y = alpha·Aᵀ·x + beta·y (g4s_spmv_transpose) — CSR.spmv_transpose as a function, like spmv."""
    return A.spmv_transpose(x, y, alpha, beta)


def spmv_semiring_transpose(A, x, y=None, semiring="min_plus", accumulate=False):
    """y := Aᵀ ⊗ x or y ⊕ (Aᵀ ⊗ x) (g4s_spmv_semiring_transpose) — CSR.spmv_semiring_transpose as a function."""
    _spmv_semiring_flags(semiring, accumulate, y)
    return A.spmv_semiring_transpose(x, y, semiring, accumulate)


DIRECTIONS = {"auto": 0, "push": capi.TRAVERSE_PUSH, "pull": capi.TRAVERSE_PULL}


def _traverse_flags(direction, symmetric):
    """The flags of g4s_sssp / g4s_bfs; ValueError (before any GPU call) for an unknown direction."""
    if not isinstance(direction, str) or direction not in DIRECTIONS:
        raise ValueError(f"unknown direction {direction!r}; expected one of {sorted(DIRECTIONS)}")
    return DIRECTIONS[direction] | (capi.TRAVERSE_SYMMETRIC if symmetric else 0)


def sssp(A, sources, max_iterations=0, direction="auto", symmetric=False):
    """(dist, info) = shortest paths from `sources` on the graph A stores by out-edges (g4s_sssp) — CSR.sssp as a function."""
    _traverse_flags(direction, symmetric)
    return A.sssp(sources, max_iterations, direction, symmetric)


def bfs(A, sources, max_depth=0, direction="auto", symmetric=False):
    """(level, info) = BFS levels from `sources` (g4s_bfs) — CSR.bfs as a function."""
    _traverse_flags(direction, symmetric)
    return A.bfs(sources, max_depth, direction, symmetric)


def _pagerank_args(damping, tol, max_iterations, personalization, start, symmetric, A=None):
    """The flags of g4s_pagerank; ValueError (before any GPU call) for an argument the call would refuse."""
    if isinstance(damping, bool) or not isinstance(damping, (int, float, np.floating)) or not (0.0 <= damping < 1.0):
        raise ValueError(f"damping must be a number in [0, 1), not {damping!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating)) or not (tol >= 0.0):
        raise ValueError(f"tol must be a number >= 0, not {tol!r}")
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, (int, np.integer)) or not (0 <= max_iterations < 2 ** 31):
        raise ValueError(f"max_iterations must be an int >= 0 (0: 100), not {max_iterations!r}")
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError(f"symmetric must be a bool, not {symmetric!r}")
    for name, v in (("personalization", personalization), ("start", start)):
        if v is None:
            continue
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.dim() != 1:
            raise ValueError(f"{name} must be a 1-D float64 tensor or None")
        if A is not None and v.numel() != A.rows:
            raise ValueError(f"{name} has {v.numel()} entries, the graph has {A.rows} vertices")
        if not v.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
    if A is not None and A.rows != A.cols:
        raise ValueError(f"PageRank needs a square matrix, not {A.rows} x {A.cols}")
    return (capi.PAGERANK_SYMMETRIC if symmetric else 0) | (capi.PAGERANK_WARM_START if start is not None else 0)


def pagerank(A, damping=0.85, tol=1e-10, max_iterations=0, personalization=None, start=None, symmetric=False):
    """(rank, info) = PageRank of the graph A stores by out-edges (g4s_pagerank) — CSR.pagerank as a function."""
    _pagerank_args(damping, tol, max_iterations, personalization, start, symmetric)
    return A.pagerank(damping, tol, max_iterations, personalization, start, symmetric)


def _betweenness_args(sources, scale, out, accumulate, A=None):
    """(sources as a contiguous int32 array, the flags of g4s_betweenness); ValueError (before any GPU call) for an argument the call would refuse."""
    if isinstance(sources, (str, bytes)) or sources is None:
        raise ValueError(f"sources must be a vertex id or a sequence of vertex ids, not {sources!r}")
    try:
        arr = np.atleast_1d(np.asarray(sources))
    except Exception as e:
        raise ValueError(f"sources must be a vertex id or a sequence of vertex ids: {e}") from None
    if arr.ndim != 1 or arr.size < 1 or arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"sources must be a non-empty 1-D sequence of integers, not {sources!r}")
    if arr.min() < 0 or arr.max() >= (A.rows if A is not None else 2 ** 31):
        raise ValueError(f"sources holds a vertex id outside [0, {A.rows if A is not None else 2 ** 31})")
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating, np.integer)) or not np.isfinite(scale):
        raise ValueError(f"scale must be a finite number, not {scale!r}")
    if not isinstance(accumulate, (bool, np.bool_)):
        raise ValueError(f"accumulate must be a bool, not {accumulate!r}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs the out to add to (out is None)")
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.dim() != 1 or not out.is_contiguous():
            raise ValueError("out must be a contiguous 1-D float64 tensor or None")
        if A is not None and out.numel() != A.rows:
            raise ValueError(f"out has {out.numel()} entries, the graph has {A.rows} vertices")
        if not out.is_cuda:
            raise ValueError("out must be a device tensor")
    if A is not None and A.rows != A.cols:
        raise ValueError(f"betweenness needs a square matrix, not {A.rows} x {A.cols}")
    return np.ascontiguousarray(arr, dtype=np.int32), (capi.BC_ACCUMULATE if accumulate else 0)


def betweenness(A, sources, scale=1.0, out=None, accumulate=False):
    """(bc, info) = betweenness centrality of the graph A stores by out-edges, from `sources` (g4s_betweenness) — CSR.betweenness as a function."""
    _betweenness_args(sources, scale, out, accumulate)
    return A.betweenness(sources, scale, out, accumulate)


def csr_transpose(rowptr, colids, values, rows, cols, with_perm=False):
    """Aᵀ of a rows × cols CSR through g4s_csr_transpose: (trowptr, tcolids, tvalues) as CUDA tensors, plus perm with with_perm=True. numpy inputs go
    through host pointers, CUDA tensors through device pointers (on the current torch stream). values may be None: the pattern only (tvalues None).
    Stable: perm = argsort(colids, kind="stable"), tcolids = row_of_entry[perm], tvalues = values[perm]."""
    _require_gpu()
    rows, cols = int(rows), int(cols)
    lib = capi.load()
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and (values is None or values.is_cuda)
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        assert rowptr.dtype == torch.int32 and colids.dtype == torch.int32 and rowptr.numel() == rows + 1
        values = None if values is None else values.contiguous()
        assert values is None or (values.dtype == torch.float64 and values.numel() == colids.numel())
        nnz, dev = colids.numel(), rowptr.device
        trp = torch.empty(cols + 1, dtype=torch.int32, device=dev)
        tci = torch.empty(nnz, dtype=torch.int32, device=dev)
        tva = None if values is None else torch.empty(nnz, dtype=torch.float64, device=dev)
        perm = torch.empty(nnz, dtype=torch.int32, device=dev) if with_perm else None
        capi.check(lib.g4s_csr_transpose(rows, cols, nnz, _ptr(rowptr), _ptr(colids), _ptr(values), _ptr(trp), _ptr(tci), _ptr(tva), _ptr(perm),
                                         capi.DEVICE_POINTERS, _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        values = None if values is None else np.ascontiguousarray(values, np.float64)
        assert rowptr.size == rows + 1 and (values is None or values.size == colids.size)
        nnz = colids.size
        trp, tci = np.empty(cols + 1, np.int32), np.empty(nnz, np.int32)
        tva = None if values is None else np.empty(nnz, np.float64)
        perm = np.empty(nnz, np.int32) if with_perm else None
        P = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size > 0 else C.c_void_p(0)
        capi.check(lib.g4s_csr_transpose(rows, cols, nnz, P(rowptr), P(colids), P(values), P(trp), P(tci), P(tva), P(perm), capi.HOST_POINTERS,
                                         _stream()))
        cu = lambda a: None if a is None else torch.from_numpy(a).cuda()
        trp, tci, tva, perm = cu(trp), cu(tci), cu(tva), cu(perm)
    return (trp, tci, tva, perm) if with_perm else (trp, tci, tva)


def _spmm_ld(M, col_major):
    """The leading dimension of a 2-D block M read in the given layout (row-major: element (i, j) at [i·ld + j], column-major: [i + j·ld]), or None
    when M is not laid out that way. A stride along an axis of extent 1 is never used and does not count."""
    r, k = M.shape
    inner, outer, n_outer, n_inner = (0, 1, k, r) if col_major else (1, 0, r, k)
    if n_inner > 1 and M.stride(inner) != 1:
        return None
    if n_outer <= 1:
        return max(n_inner, 1)
    return M.stride(outer) if M.stride(outer) >= n_inner else None


def spmm(A, X, Y=None, alpha=1.0, beta=0.0):
    """Y = alpha·A·X + beta·Y (g4s_spmm) — CSR.spmm as a function, like spmv."""
    _require_gpu()
    return A.spmm(X, Y, alpha, beta)


def get_flop(A, B):
    """Σ_i Σ_{j∈A(i,:)} nnz(B(acol_j,:)) — get_flop, mm/inc/hash_mult.h:46-62; compute_flop, mkl_mult.h:8-38."""
    flop = C.c_int64(0)
    capi.check(capi.load().g4s_spgemm_flop(A.rows, _ptr(A.rowptr), _ptr(A.colids), _ptr(B.rowptr), C.byref(flop), C.c_void_p(0),
                                           capi.DEVICE_POINTERS))
    return flop.value


class _LibraryBuffer:
    """A device array the library allocated for a callee-allocated output (mkl_mult.h:90-92: outputs are allocated by the callee and
    freed by the caller). torch views it without a copy through __cuda_array_interface__ and keeps this object alive; the memory goes
    back through g4s_dev_free when the last view is gone."""

    def __init__(self, ptr, count, typestr):
        self._ptr, self._count, self._typestr = int(ptr or 0), int(count), typestr

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self._count,), "typestr": self._typestr, "data": (self._ptr, False), "version": 2}

    def __del__(self):
        try:
            if self._ptr:
                capi.load().g4s_dev_free(C.c_void_p(self._ptr))
        except Exception:
            pass


class _BorrowedBuffer:
    """A device array owned by a library object (e.g. the vectors of a g4s_cg_ws_t), viewed by torch without a copy."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def view_f64(ptr, count, device="cuda"):
    """torch view of `count` doubles at a device pointer the caller keeps alive."""
    return torch.as_tensor(_BorrowedBuffer(ptr.value if hasattr(ptr, "value") else ptr, count, "<f8"), device=device)


def view_i32(ptr, count, device="cuda"):
    """torch view of `count` int32 at a device pointer the caller keeps alive."""
    return torch.as_tensor(_BorrowedBuffer(ptr.value if hasattr(ptr, "value") else ptr, count, "<i4"), device=device)


def _view(ptr, count, typestr, dtype, device):
    if count == 0:
        if ptr:
            capi.load().g4s_dev_free(ptr)
        return torch.empty(0, dtype=dtype, device=device)
    return torch.as_tensor(_LibraryBuffer(ptr.value if hasattr(ptr, "value") else ptr, count, typestr), device=device)


SEMIRINGS = {"plus_times": capi.SEMIRING_PLUS_TIMES, "min_plus": capi.SEMIRING_MIN_PLUS, "max_plus": capi.SEMIRING_MAX_PLUS, "or_and": capi.SEMIRING_OR_AND}


def HashSpGEMM(a, b, sortOutput=True, two_phase=False, semiring="plus_times"):
    """C = A·B — HashSpGEMM, mm/inc/hash_mult.h:1028-1057. One call into the library (symbolic → crpt, numeric → ccol/cval, the sorted
    columns of the large rows carried from the first phase to the second); `two_phase=True` issues g4s_spgemm_symbolic and
    g4s_spgemm_numeric separately into torch-owned arrays. The result's `timings` holds the library's stage times (one-call form).
    `semiring` picks the multiply/add pair (include/g4s.h, G4S_SEMIRING_*): "plus_times" (Σ a·b), "min_plus" (min(a + b)), "max_plus"
    (max(a + b)) or "or_and" (1.0 where any a != 0 and b != 0, else 0.0); the pattern of C is the same for all four."""
    if semiring not in SEMIRINGS:
        raise ValueError(f"unknown semiring {semiring!r}; expected one of {sorted(SEMIRINGS)}")
    _require_gpu()
    assert a.cols == b.rows
    lib = capi.load()
    dev = a.rowptr.device
    if not two_phase:
        crpt_p, ccol_p, cval_p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        cnnz, tm = C.c_int64(0), capi.Timings()
        flags = capi.DEVICE_POINTERS | (capi.SORT_OUTPUT if sortOutput else 0) | SEMIRINGS[semiring]
        capi.check(lib.g4s_spgemm_csr_i32_f64(_ptr(a.rowptr), _ptr(a.colids), _ptr(a.values), _ptr(b.rowptr), _ptr(b.colids), _ptr(b.values),
                                              C.byref(crpt_p), C.byref(ccol_p), C.byref(cval_p), a.rows, a.cols, b.cols, C.byref(cnnz), C.byref(tm), flags))
        c = CSR(_view(crpt_p, a.rows + 1, "<i4", torch.int32, dev), _view(ccol_p, cnnz.value, "<i4", torch.int32, dev),
                _view(cval_p, cnnz.value, "<f8", torch.float64, dev), a.rows, b.cols)
        c.timings = {n: getattr(tm, n) for n, _ in capi.Timings._fields_}
        return c
    crpt = torch.empty(a.rows + 1, dtype=torch.int32, device=dev)
    cnnz = C.c_int64(0)
    capi.check(lib.g4s_spgemm_symbolic(a.rows, a.cols, b.cols, _ptr(a.rowptr), _ptr(a.colids), _ptr(b.rowptr), _ptr(b.colids),
                                       _ptr(crpt), C.byref(cnnz), _stream()))
    ccol = torch.empty(cnnz.value, dtype=torch.int32, device=dev)
    cval = torch.empty(cnnz.value, dtype=torch.float64, device=dev)
    flags = capi.DEVICE_POINTERS | (capi.SORT_OUTPUT if sortOutput else 0) | SEMIRINGS[semiring]
    capi.check(lib.g4s_spgemm_numeric(a.rows, a.cols, b.cols, _ptr(a.rowptr), _ptr(a.colids), _ptr(a.values),
                                      _ptr(b.rowptr), _ptr(b.colids), _ptr(b.values), _ptr(crpt), _ptr(ccol), _ptr(cval),
                                      flags, _stream()))
    return CSR(crpt, ccol, cval, a.rows, b.cols)


def _ptr_nn(t):
    """Like _ptr, but never NULL: an empty array is passed as a pointer that is not read (entry points that take NULL for 'absent')."""
    if t.numel() > 0:
        return C.c_void_p(t.data_ptr())
    if t.device not in _PLACEHOLDER:
        _PLACEHOLDER[t.device] = torch.zeros(2, dtype=torch.float64, device=t.device)
    return C.c_void_p(_PLACEHOLDER[t.device].data_ptr())


_PLACEHOLDER = {}


def _masked_info(info):
    return {n: getattr(info, n) for n, _ in capi.MaskedInfo._fields_}


def spgemm_masked(a, b, mask, semiring="plus_times", pattern_only=False, return_info=False):
    """C⟨M⟩ = A ⊗ B: the product over `semiring` computed only at the positions of the pattern `mask` (g4s_spgemm_masked) — a CSR, or a
    (rowptr, colids) pair of int32 device tensors, with strictly ascending rows. The result is a CSR that SHARES the mask's rowptr / colids tensors
    and owns the new values: the full product's value where it has an entry, the semiring's identity (0.0, +inf, −inf, 0.0) elsewhere.
    pattern_only=True counts every stored value of a and b as 1.0 and reads no values: plus_times then counts the products of each entry, or_and
    marks the entries that receive one. mask may be a or b itself (C⟨A⟩ = A·A). Synchronous. return_info=True adds the dict of g4s_masked_info."""
    if semiring not in SEMIRINGS:
        raise ValueError(f"unknown semiring {semiring!r}; expected one of {sorted(SEMIRINGS)}")
    _require_gpu()
    mrp, mci = (mask.rowptr, mask.colids) if isinstance(mask, CSR) else mask
    assert a.cols == b.rows
    assert mrp.dtype == torch.int32 and mci.dtype == torch.int32 and mrp.is_cuda and mci.is_cuda and mrp.numel() == a.rows + 1
    mrp, mci = mrp.contiguous(), mci.contiguous()
    cval = torch.empty(mci.numel(), dtype=torch.float64, device=mci.device)
    info = capi.MaskedInfo()
    null = C.c_void_p(0)
    capi.check(capi.load().g4s_spgemm_masked(a.rows, a.cols, b.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), null if pattern_only else _ptr_nn(a.values),
                                             _ptr_nn(b.rowptr), _ptr_nn(b.colids), null if pattern_only else _ptr_nn(b.values), _ptr_nn(mrp), _ptr_nn(mci),
                                             _ptr_nn(cval), capi.DEVICE_POINTERS | SEMIRINGS[semiring], C.byref(info), _stream()))
    c = CSR(mrp, mci, cval, a.rows, b.cols)
    return (c, _masked_info(info)) if return_info else c


def triangle_count(A, return_info=False):
    """The number of vertex triples i > j > k with (i, j), (i, k) and (j, k) all stored below the diagonal of the square pattern A
    (g4s_triangle_count): the triangles of a simple undirected graph given as its symmetric pattern or as its lower triangle; entries on and above
    the diagonal do not count. Rows must be strictly ascending. Synchronous. return_info=True adds the g4s_masked_info of the product L·L⟨L⟩."""
    _require_gpu()
    assert A.rows == A.cols
    count, info = C.c_int64(0), capi.MaskedInfo()
    capi.check(capi.load().g4s_triangle_count(A.rows, _ptr_nn(A.rowptr), _ptr_nn(A.colids), C.byref(count), capi.DEVICE_POINTERS, C.byref(info), _stream()))
    return (count.value, _masked_info(info)) if return_info else count.value


def connected_components(A, symmetric=False, return_info=False):
    """labels (int32 device tensor of n) = the smallest vertex id of each vertex's weakly connected component (g4s_connected_components): every
    stored entry of the square pattern is an undirected edge, whatever its value. A is a CSR, or a (rowptr, colids) pair of int32 device tensors or
    of numpy arrays (host pointers; the labels come back on the device all the same). symmetric=True declares the PATTERN symmetric, which lets the
    call skip the rows of the largest sampled component; on a pattern that is not, components may come out split. Synchronous; no plan is built.
    return_info=True adds the dict of g4s_cc_info. ValueError (before any GPU call) for a non-square CSR or a `symmetric` that is not a bool."""
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError(f"symmetric must be a bool, not {symmetric!r}")
    if isinstance(A, (tuple, list)):
        if len(A) != 2:
            raise ValueError("expected a CSR or a (rowptr, colids) pair")
        rowptr, colids = A
        n = int(rowptr.numel() if isinstance(rowptr, torch.Tensor) else np.asarray(rowptr).size) - 1
        if n < 0:
            raise ValueError("rowptr is empty: a pattern of n rows has n + 1 row pointers")
    else:
        if A.rows != A.cols:
            raise ValueError(f"connected components need a square pattern, not {A.rows} x {A.cols}")
        rowptr, colids, n = A.rowptr, A.colids, int(A.rows)
    _require_gpu()
    flags = capi.CC_SYMMETRIC if symmetric else 0
    info = capi.CCInfo()
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        labels = torch.empty(n, dtype=torch.int32, device=rowptr.device)
        capi.check(capi.load().g4s_connected_components(n, _ptr_nn(rowptr), _ptr_nn(colids), _ptr_nn(labels), flags | capi.DEVICE_POINTERS, C.byref(info),
                                                        _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        out = np.empty(max(n, 1), np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        capi.check(capi.load().g4s_connected_components(n, P(rowptr), P(colids if colids.size else out), P(out), flags | capi.HOST_POINTERS, C.byref(info),
                                                        _stream()))
        labels = torch.from_numpy(out[:n]).cuda()
    inf = {n_: getattr(info, n_) for n_, _ in capi.CCInfo._fields_}
    return (labels, inf) if return_info else labels


def _pattern_of(A, what):
    """(rowptr, colids, n) of a CSR or of a (rowptr, colids) pair; ValueError for a pair of the wrong length, an empty rowptr, a CSR that is not square"""
    if isinstance(A, (tuple, list)):
        if len(A) != 2:
            raise ValueError("expected a CSR or a (rowptr, colids) pair")
        rowptr, colids = A
        n = int(rowptr.numel() if isinstance(rowptr, torch.Tensor) else np.asarray(rowptr).size) - 1
        if n < 0:
            raise ValueError("rowptr is empty: a pattern of n rows has n + 1 row pointers")
        return rowptr, colids, n
    if A.rows != A.cols:
        raise ValueError(f"{what} needs a square pattern, not {A.rows} x {A.cols}")
    return A.rowptr, A.colids, int(A.rows)


def strongly_connected_components(A, transpose=None, return_info=False):
    """labels (int32 device tensor of n) = the smallest vertex id of each vertex's STRONGLY connected component (g4s_strongly_connected_components):
    every stored entry (u, v) of the square pattern is an edge u → v, whatever its value. A is a CSR, or a (rowptr, colids) pair of int32 device
    tensors or of numpy arrays (host pointers; the labels come back on the device all the same). transpose: the (trowptr, tcolids) pair of Aᵀ's
    pattern, of the same kind as A's arrays, for a caller who has it (csr_transpose gives one); None lets the call build it. Synchronous; no plan is
    built. return_info=True adds the dict of g4s_scc_info. ValueError (before any GPU call) for a CSR that is not square, a transpose that is not a
    pair, whose trowptr does not have n + 1 entries or whose arrays are not of A's kind, and a return_info that is not a bool."""
    if not isinstance(return_info, (bool, np.bool_)):
        raise ValueError(f"return_info must be a bool, not {return_info!r}")
    rowptr, colids, n = _pattern_of(A, "strongly connected components")
    on_device = isinstance(rowptr, torch.Tensor)
    trp = tci = None
    if transpose is not None:
        if not isinstance(transpose, (tuple, list)) or len(transpose) != 2:
            raise ValueError("transpose must be None or a (trowptr, tcolids) pair")
        trp, tci = transpose
        if isinstance(trp, torch.Tensor) != on_device or isinstance(tci, torch.Tensor) != on_device:
            raise ValueError("transpose must be of the same kind as the pattern: device tensors with device tensors, numpy arrays with numpy arrays")
        size = (lambda a: int(a.numel())) if on_device else (lambda a: int(np.asarray(a).size))
        if size(trp) != n + 1 or size(tci) != size(colids):
            raise ValueError(f"transpose has the wrong length: trowptr needs {n + 1} entries and tcolids {size(colids)}, not {size(trp)} and {size(tci)}")
    _require_gpu()
    info, null = capi.SCCInfo(), C.c_void_p(0)
    fn = capi.load().g4s_strongly_connected_components
    if on_device:
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        if trp is not None:
            assert trp.is_cuda and tci.is_cuda and trp.dtype == torch.int32 and tci.dtype == torch.int32
            trp, tci = trp.contiguous(), tci.contiguous()
        labels = torch.empty(n, dtype=torch.int32, device=rowptr.device)
        capi.check(fn(n, _ptr_nn(rowptr), _ptr_nn(colids), null if trp is None else _ptr_nn(trp), null if trp is None else _ptr_nn(tci), _ptr_nn(labels),
                      capi.DEVICE_POINTERS, C.byref(info), _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        out = np.empty(max(n, 1), np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        if trp is not None:
            trp, tci = np.ascontiguousarray(trp, np.int32), np.ascontiguousarray(tci, np.int32)
        spare = np.zeros(1, np.int32)                                   # an empty array is passed as a pointer that is not read
        capi.check(fn(n, P(rowptr), P(colids if colids.size else spare), null if trp is None else P(trp), null if trp is None else P(tci if tci.size else spare),
                      P(out), capi.HOST_POINTERS, C.byref(info), _stream()))
        labels = torch.from_numpy(out[:n]).cuda()
    inf = {n_: getattr(info, n_) for n_, _ in capi.SCCInfo._fields_ if n_ != "reserved"}
    return (labels, inf) if return_info else labels


def minimum_spanning_forest(A, maximum=False, return_labels=False):
    """(positions, info) of the minimum spanning forest of the undirected graph whose edges are the stored off-diagonal entries of the square matrix A
    (g4s_minimum_spanning_forest): positions (int32 device tensor of info["edges"]) = the ascending indices k into colids / values of the forest's
    entries, under the strict order (w, min(i,j), max(i,j), k) — the forest Kruskal builds scanning the entries in that order, the same on every run.
    A is a CSR (the weights are its values), or a (rowptr, colids) pair (all weights equal: a spanning forest) or a (rowptr, colids, values) triple of
    device tensors or of numpy arrays (host pointers; the results come back on the device all the same). maximum=True gives the maximum spanning forest
    (only the weight is reversed). return_labels=True returns (positions, labels, info), labels being those of connected_components. info is the dict
    of g4s_msf_info. Synchronous; no plan is built. ValueError (before any GPU call) for a CSR that is not square, a tuple of the wrong length, values
    that do not match colids, and flags that are not bools."""
    for name, v in (("maximum", maximum), ("return_labels", return_labels)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    if isinstance(A, (tuple, list)):
        if len(A) not in (2, 3):
            raise ValueError("expected a CSR, a (rowptr, colids) pair or a (rowptr, colids, values) triple")
        rowptr, colids, n = _pattern_of(tuple(A[:2]), "a spanning forest")
        values = A[2] if len(A) == 3 else None
    else:
        rowptr, colids, n = _pattern_of(A, "a spanning forest")
        values = A.values
    on_device = isinstance(rowptr, torch.Tensor)
    size = (lambda a: int(a.numel())) if on_device else (lambda a: int(np.asarray(a).size))
    if values is not None and (isinstance(values, torch.Tensor) != on_device or size(values) != size(colids)):
        raise ValueError("values must be of the same kind and length as colids")
    _require_gpu()
    info, null = capi.MSFInfo(), C.c_void_p(0)
    flags = capi.MSF_MAXIMUM if maximum else 0
    fn = capi.load().g4s_minimum_spanning_forest
    if on_device:
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        assert values is None or (values.is_cuda and values.dtype == torch.float64)
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        values = None if values is None else values.contiguous()
        edges = torch.empty(max(n - 1, 0), dtype=torch.int32, device=rowptr.device)
        labels = torch.empty(n, dtype=torch.int32, device=rowptr.device) if return_labels else None
        capi.check(fn(n, _ptr_nn(rowptr), _ptr_nn(colids), null if values is None else _ptr_nn(values), _ptr_nn(edges), null if labels is None else _ptr_nn(labels),
                      flags | capi.DEVICE_POINTERS, C.byref(info), _stream()))
        positions = edges[:info.edges]
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        values = None if values is None else np.ascontiguousarray(values, np.float64)
        out, lab = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        spare = np.zeros(1, np.float64)                                 # an empty array is passed as a pointer that is not read
        P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
        capi.check(fn(n, P(rowptr), P(colids), null if values is None else P(values), P(out), P(lab) if return_labels else null, flags | capi.HOST_POINTERS,
                      C.byref(info), _stream()))
        positions = torch.from_numpy(out[:info.edges]).cuda()
        labels = torch.from_numpy(lab[:n]).cuda() if return_labels else None
    inf = {n_: getattr(info, n_) for n_, _ in capi.MSFInfo._fields_}
    return (positions, labels, inf) if return_labels else (positions, inf)


def spanning_forest_csr(A, positions, symmetric=True):
    """The forest that minimum_spanning_forest(A) found, as a device CSR of A's shape: the entries of the CSR A at `positions` (an int32 device tensor
    of indices into A.colids), rows ascending; with symmetric=True (the default) every edge is stored in both directions — 2 · len(positions) entries
    — as connected_components(…, symmetric=True), bfs and sssp want an undirected graph. A composition of existing device calls: csr_row_indices, two
    gathers, csr_from_coo and, for symmetric=True, csr_symmetrise. No new kernel. ValueError (before any GPU call) for an A that is not a square CSR
    and a `symmetric` that is not a bool."""
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError(f"symmetric must be a bool, not {symmetric!r}")
    if not isinstance(A, CSR) or A.rows != A.cols:
        raise ValueError("spanning_forest_csr needs the square CSR the positions point into")
    _require_gpu()
    assert positions.is_cuda and positions.dtype == torch.int32 and positions.dim() == 1
    n, at = int(A.rows), positions.long()
    row = csr_row_indices(A.rowptr, A.nnz)[at]
    rp, ci, va = csr_from_coo(row, A.colids[at], A.values[at], n, n, dup="first")
    f = CSR(rp, ci, va, n, n)
    return csr_symmetrise(f, "first") if symmetric else f


def compact_labels(labels):
    """(index, roots) of canonical component labels — those of connected_components or of strongly_connected_components (an int32 device tensor with
    labels[labels[v]] == labels[v]): roots (int32, ascending) = the k distinct labels, index[v] (int32) = the rank of labels[v] among them, so
    roots[index] == labels and component a of the numbering 0 … k−1 is the one whose smallest vertex is roots[a]. A composition of device calls
    (a compare, a prefix sum, a gather): no new kernel."""
    _require_gpu()
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.dim() == 1
    n = labels.numel()
    is_root = labels == torch.arange(n, dtype=torch.int32, device=labels.device)
    rank = torch.cumsum(is_root, 0, dtype=torch.int32) - 1             # rank[r] of a root r: the roots below it
    roots = torch.nonzero(is_root).flatten().to(torch.int32)
    return rank[labels.long()], roots


def condensation(A, labels=None):
    """(C, index): the condensation of the directed graph A (a CSR) by its strongly connected components — C is the k × k device CSR (values 1.0)
    with an entry (a, b) where some stored edge of A runs from component a to a DIFFERENT component b, rows ascending, repeats merged; index[v] is
    v's component in the numbering of compact_labels. labels: the result of strongly_connected_components(A), computed when None. C is acyclic. A
    composition: csr_row_indices, a gather through index, csr_from_coo (repeats merged) and csr_select dropping the diagonal."""
    rowptr, colids, n = _pattern_of(A, "a condensation")
    if isinstance(A, (tuple, list)):
        raise ValueError("condensation needs a CSR, not a (rowptr, colids) pair")
    if labels is None:
        labels = strongly_connected_components(A)
    index, roots = compact_labels(labels)
    k = int(roots.numel())
    src = index[csr_row_indices(rowptr, int(colids.numel())).long()]
    dst = index[colids.long()]
    crp, cci, _ = csr_from_coo(src, dst, None, k, k, dup="first")
    c = CSR(crp, cci, torch.ones(cci.numel(), dtype=torch.float64, device=cci.device), k, k)
    return csr_select(c, "offdiag"), index


def _is_count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 0


def kcore(A, max_k=None, return_round=False, return_info=False):
    """core (int32 device tensor of n): core[v] = the largest k such that v belongs to a subgraph in which every vertex has at least k neighbours
    (g4s_kcore) — networkx.core_number of the graph without self-loops. A is a CSR, or a (rowptr, colids) pair of int32 device tensors or of numpy
    arrays (host pointers; the results come back on the device all the same), and holds the SYMMETRIC pattern of a simple undirected graph with
    strictly ascending rows (csr_symmetrise gives one); a stored diagonal entry is ignored. max_k: peel the levels below it only — the vertices of the
    max_k-core then get core = max_k and round = −1; None is the full decomposition. return_round=True adds round (int32 device tensor): the index of
    the peel frontier that removed each vertex, a function of the graph alone. return_info=True adds the dict of g4s_kcore_info. Synchronous; no plan
    is built. ValueError (before any GPU call) for a CSR that is not square, a max_k that is not a non-negative integer below 2^31, and return_round /
    return_info that are not bools."""
    if max_k is not None and not (_is_count(max_k) and max_k <= capi.KCORE_FULL):
        raise ValueError(f"max_k must be None or a non-negative integer below 2^31, not {max_k!r}")
    for name, v in (("return_round", return_round), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    rowptr, colids, n = _pattern_of(A, "a k-core decomposition")
    _require_gpu()
    cap = capi.KCORE_FULL if max_k is None else int(max_k)
    info, null = capi.KCoreInfo(), C.c_void_p(0)
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        core = torch.empty(n, dtype=torch.int32, device=rowptr.device)
        rnd = torch.empty(n, dtype=torch.int32, device=rowptr.device) if return_round else None
        capi.check(capi.load().g4s_kcore(n, _ptr_nn(rowptr), _ptr_nn(colids), cap, _ptr_nn(core), _ptr_nn(rnd) if return_round else null,
                                         capi.DEVICE_POINTERS, C.byref(info), _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        out, out_r = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        capi.check(capi.load().g4s_kcore(n, P(rowptr), P(colids if colids.size else out), cap, P(out), P(out_r) if return_round else null,
                                         capi.HOST_POINTERS, C.byref(info), _stream()))
        core = torch.from_numpy(out[:n]).cuda()
        rnd = torch.from_numpy(out_r[:n]).cuda() if return_round else None
    res = (core,) + ((rnd,) if return_round else ()) + (({n_: getattr(info, n_) for n_, _ in capi.KCoreInfo._fields_},) if return_info else ())
    return res[0] if len(res) == 1 else res


def _rhs_block(b, out, n, name):
    """What the block entry points (g4s_sptrsv_solve_multi, g4s_ilu0_apply_multi) need of a 2-D right-hand side b of n × k and its output: (out, k, ldb,
    ldo, flags). Row-major when stride(1) == 1, column-major when stride(0) == 1, read the way CSR.spmm reads its blocks (_spmm_ld); out has b's
    layout, and a new one is allocated in it. ValueError, before any GPU call, for a wrong shape or dtype, k above capi.TRSV_MAX_RHS, blocks that are
    neither row- nor column-major, and two blocks of different layouts."""
    if not (isinstance(b, torch.Tensor) and b.dtype == torch.float64 and b.dim() == 2 and b.shape[0] == n):
        raise ValueError(f"{name} must be a float64 tensor of {n} entries or of {n} x k")
    k = int(b.shape[1])
    if k > capi.TRSV_MAX_RHS:
        raise ValueError(f"{name} has {k} columns, more than the {capi.TRSV_MAX_RHS} one call takes")
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == (n, k) and out.device == b.device):
        raise ValueError(f"out must be a float64 tensor of {n} x {k} on {name}'s device")
    for cm in (False, True):                                        # row-major when both blocks are, else column-major when both are
        ldb = _spmm_ld(b, cm)
        ldo = ldb if out is None else _spmm_ld(out, cm)
        if ldb is not None and ldo is not None:
            break
    else:
        raise ValueError(f"{name} and out must both be row-major (stride(1) == 1) or both column-major (stride(0) == 1); strides {tuple(b.stride())}"
                         + ("" if out is None else f", {tuple(out.stride())}"))
    _require_gpu()
    assert b.is_cuda
    if out is None:
        out = torch.empty(k, n, dtype=torch.float64, device=b.device).t() if cm else torch.empty(n, k, dtype=torch.float64, device=b.device)
        ldo = _spmm_ld(out, cm)
    return out, k, ldb, ldo, (capi.TRSV_COL_MAJOR if cm else 0)


def _solve_rhs(handle, single, multi, b, out, n, name):
    """TriangularPlan.solve and ILU0.apply behind their open handle: a 2-D b goes as a block (_rhs_block) to the C function named multi, a vector of
    n doubles to the one named single; out is allocated where it is None, and returned. `name` is what the ValueErrors call b."""
    if isinstance(b, torch.Tensor) and b.dim() == 2:
        out, k, ldb, ldo, flags = _rhs_block(b, out, n, name)
        capi.check(getattr(capi.load(), multi)(handle, k, _ptr(b), ldb, _ptr(out), ldo, flags, _stream()))
        return out
    if not (isinstance(b, torch.Tensor) and b.dtype == torch.float64 and b.dim() == 1 and b.numel() == n and b.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float64 tensor of {n} entries")
    if out is None:
        out = torch.empty_like(b)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.dim() == 1 and out.numel() == n and out.is_contiguous()
              and out.device == b.device):
        raise ValueError(f"out must be a contiguous float64 tensor of {n} entries on {name}'s device")
    assert b.is_cuda
    capi.check(getattr(capi.load(), single)(handle, _ptr_nn(b), _ptr_nn(out), _stream()))
    return out


class TriangularPlan:
    """A g4s_trsv_t: the (level, row) copy of a triangle and its launch list. solve(b, out=None) enqueues on the current torch stream and waits for
    nothing (it can be captured into a graph); out may be b. b is a vector of n doubles or a 2-D block of n × k right-hand sides (row- or
    column-major, see _rhs_block), solved on the launches of one (g4s_sptrsv_solve_multi): column j of the result is, bit for bit, the solve of
    column j. info: the dict of g4s_trsv_info. close() releases the handle."""

    def __init__(self, handle, n, nnz, info):
        self._handle, self.n, self.nnz = handle, int(n), int(nnz)
        self.info = {n_: getattr(info, n_) for n_, _ in capi.TRSVInfo._fields_ if n_ != "reserved"}

    def solve(self, b, out=None):
        if self._handle is None:
            raise ValueError("the plan is closed")
        return _solve_rhs(self._handle, "g4s_sptrsv_solve", "g4s_sptrsv_solve_multi", b, out, self.n, "b")

    def update_values(self, values):
        """New values in the layout of the arrays the plan was analysed from (all nnz of them): a device tensor (refreshed on the current torch
        stream, asynchronous) or a numpy array (copied in, synchronous)."""
        if self._handle is None:
            raise ValueError("the plan is closed")
        on_device = isinstance(values, torch.Tensor)
        if (int(values.numel()) if on_device else int(np.asarray(values).size)) != self.nnz:
            raise ValueError(f"values must have the {self.nnz} entries of the analysed arrays")
        if on_device:
            assert values.is_cuda and values.dtype == torch.float64
            values = values.contiguous()
            capi.check(capi.load().g4s_sptrsv_update_values(self._handle, _ptr_nn(values), capi.DEVICE_POINTERS, _stream()))
        else:
            values = np.ascontiguousarray(values, np.float64)
            spare = np.zeros(1, np.float64)
            capi.check(capi.load().g4s_sptrsv_update_values(self._handle, C.c_void_p((values if values.size else spare).ctypes.data), capi.HOST_POINTERS, _stream()))

    def close(self):
        if self._handle is not None:
            capi.load().g4s_sptrsv_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _triangle_args(A, flags):
    """(rowptr, colids, values, n) of a CSR or a (rowptr, colids, values) triple; ValueError for everything that can be refused without a device"""
    for name, v in flags:
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    if isinstance(A, (tuple, list)):
        if len(A) != 3:
            raise ValueError("expected a CSR or a (rowptr, colids, values) triple")
        rowptr, colids, n = _pattern_of(tuple(A[:2]), "a triangular solve")
        values = A[2]
    else:
        rowptr, colids, n = _pattern_of(A, "a triangular solve")
        values = A.values
    on_device = isinstance(rowptr, torch.Tensor)
    size = (lambda a: int(a.numel())) if on_device else (lambda a: int(np.asarray(a).size))
    if isinstance(colids, torch.Tensor) != on_device or isinstance(values, torch.Tensor) != on_device or size(values) != size(colids):
        raise ValueError("rowptr, colids and values must be of the same kind, and values of the same length as colids")
    return rowptr, colids, values, n


def sptrsv_analyse(A, lower=True, unit_diagonal=False, return_level=False, no_chains=False):
    """The plan (TriangularPlan) of the solve T x = b with the lower (lower=False: upper) triangle T of the square matrix A (g4s_sptrsv_analyse):
    only the entries of that triangle are read, so the (D + L) of a general A is solved from A itself. A is a CSR, or a (rowptr, colids, values)
    triple of device tensors or of numpy arrays (host pointers). unit_diagonal=True ignores stored diagonal entries; without it a row that stores
    none is refused (capi.G4SError; the message names the smallest such row). return_level=True returns (plan, level), level being the int32 device
    tensor of the rows' depths in the dependency DAG. no_chains=True is the test switch G4S_TRSV_NO_CHAINS: one launch per level, the same bits.
    Synchronous. ValueError (before any GPU call) for a CSR that is not square, a tuple of the wrong length, arrays of mixed kinds, values that do
    not match colids, and flags that are not bools."""
    rowptr, colids, values, n = _triangle_args(A, (("lower", lower), ("unit_diagonal", unit_diagonal), ("return_level", return_level), ("no_chains", no_chains)))
    _require_gpu()
    flags = (0 if lower else capi.TRSV_UPPER) | (capi.TRSV_UNIT_DIAGONAL if unit_diagonal else 0) | (capi.TRSV_NO_CHAINS if no_chains else 0)
    info, null, handle = capi.TRSVInfo(), C.c_void_p(0), C.c_void_p()
    fn = capi.load().g4s_sptrsv_analyse
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and values.is_cuda
        assert rowptr.dtype == torch.int32 and colids.dtype == torch.int32 and values.dtype == torch.float64
        rowptr, colids, values = rowptr.contiguous(), colids.contiguous(), values.contiguous()
        level = torch.empty(n, dtype=torch.int32, device=rowptr.device) if return_level else None
        capi.check(fn(C.byref(handle), n, _ptr_nn(rowptr), _ptr_nn(colids), _ptr_nn(values), _ptr_nn(level) if return_level else null,
                      flags | capi.DEVICE_POINTERS, C.byref(info), _stream()))
        nnz = int(colids.numel())
    else:
        rowptr, colids, values = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32), np.ascontiguousarray(values, np.float64)
        lev = np.empty(max(n, 1), np.int32)
        spare = np.zeros(1, np.float64)                                 # an empty array is passed as a pointer that is not read
        P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
        capi.check(fn(C.byref(handle), n, P(rowptr), P(colids), P(values), P(lev) if return_level else null, flags | capi.HOST_POINTERS, C.byref(info),
                      _stream()))
        level = torch.from_numpy(lev[:n]).cuda() if return_level else None
        nnz = int(colids.size)
    plan = TriangularPlan(handle, n, nnz, info)
    return (plan, level) if return_level else plan


def spsolve_triangular(A, b, lower=True, unit_diagonal=False):
    """x (float64 device tensor) with T x = b for the lower / upper triangle T of A — scipy.sparse.linalg.spsolve_triangular's meaning, except that
    entries outside the triangle are ignored instead of refused. One analysis, one solve, the plan released.
    A: as for sptrsv_analyse; b: a device tensor or a numpy array of n doubles, or a 2-D one of n × k — a matrix right-hand side, solved as one
    block (TriangularPlan.solve); x has b's shape."""
    rowptr, colids, values, n = _triangle_args(A, (("lower", lower), ("unit_diagonal", unit_diagonal)))
    block = (b.dim() if isinstance(b, torch.Tensor) else np.asarray(b).ndim) == 2
    if block:
        if int(b.shape[0] if isinstance(b, torch.Tensor) else np.asarray(b).shape[0]) != n:
            raise ValueError(f"b must have {n} rows")
        if int(b.shape[1] if isinstance(b, torch.Tensor) else np.asarray(b).shape[1]) > capi.TRSV_MAX_RHS:
            raise ValueError(f"b has more than the {capi.TRSV_MAX_RHS} columns one call takes")
    elif (int(b.numel()) if isinstance(b, torch.Tensor) else int(np.asarray(b).size)) != n:
        raise ValueError(f"b must have {n} entries")
    _require_gpu()
    if not isinstance(b, torch.Tensor):
        b = np.ascontiguousarray(b, np.float64)
        b = torch.from_numpy(b if block else b.reshape(-1)).cuda()
    plan = sptrsv_analyse((rowptr, colids, values), lower, unit_diagonal)
    try:
        return plan.solve(b.contiguous())
    finally:
        torch.cuda.current_stream().synchronize()
        plan.close()


def gauss_seidel(A, b, x, sweeps=1, symmetric=False, plans=None):
    """`sweeps` Gauss–Seidel sweeps on A x = b, in place on x (float64 device tensor; returned): x ← x + (D + L)⁻¹ (b − A x), and with
    symmetric=True behind each of them the backward half x ← x + (D + U)⁻¹ (b − A x) — a symmetric Gauss–Seidel sweep. A is a CSR. Wiring, no kernel of
    its own: the residual is g4s_spmv (r = −1·A·x + 1·b), the corrections are solves on the lower and upper plans of A, the rest torch vector
    operations. b and x may be 2-D blocks of the same shape n × k (x row- or column-major): every column is swept, the residual through g4s_spmm,
    the corrections through the block solve. plans: a (lower, upper or None) pair of TriangularPlans of A to reuse; without it they are analysed here and released at the end."""
    if not isinstance(A, CSR):
        raise ValueError("A must be a CSR")
    if A.rows != A.cols:
        raise ValueError(f"a Gauss–Seidel sweep needs a square matrix, not {A.rows} x {A.cols}")
    if not (isinstance(sweeps, (int, np.integer)) and not isinstance(sweeps, (bool, np.bool_)) and sweeps >= 0):
        raise ValueError(f"sweeps must be a non-negative integer, not {sweeps!r}")
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError(f"symmetric must be a bool, not {symmetric!r}")
    block = isinstance(x, torch.Tensor) and x.dim() == 2
    for name, v in (("b", b), ("x", x)):
        if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and (v.shape == x.shape if block else v.dim() == 1) and v.shape[0] == A.rows):
            raise ValueError(f"{name} must be a float64 tensor of {A.rows} entries, or both of {A.rows} x k")
    if block and _spmm_ld(x, False) is None and _spmm_ld(x, True) is None:
        raise ValueError(f"x must be row-major (stride(1) == 1) or column-major (stride(0) == 1); strides {tuple(x.stride())}")
    own = plans is None
    lo, up = (A.triangular_plan(lower=True), A.triangular_plan(lower=False) if symmetric else None) if own else plans
    if symmetric and up is None:
        raise ValueError("a symmetric sweep needs the upper plan")
    try:
        if block:                                                   # the residual in x's layout: spmm and the block solve take one layout a call
            k = x.shape[1]
            r = torch.empty(k, A.rows, dtype=torch.float64, device=x.device).t() if _spmm_ld(x, False) is None else torch.empty_like(x, memory_format=torch.contiguous_format)
        else:
            r = torch.empty_like(b)
        for _ in range(int(sweeps)):
            for plan in (lo, up) if symmetric else (lo,):
                r.copy_(b)
                if block:
                    A.spmm(x, r, alpha=-1.0, beta=1.0)
                else:
                    A.spmv(x, r, alpha=-1.0, beta=1.0)
                plan.solve(r, out=r)
                x.add_(r)
    finally:
        if own:
            torch.cuda.current_stream().synchronize()
            lo.close()
            if up is not None:
                up.close()
    return x


class ILU0:
    """A g4s_ilu0_t: the factors A ≈ L U on A's own pattern and the two solve plans on them. apply(r, out=None): z = U⁻¹ (L⁻¹ r) on the current torch
    stream, waits for nothing (it can be captured into a graph); out may be r; r is a vector of n doubles or a 2-D block of n × k of them (row- or
    column-major, see _rhs_block) applied on the launches of one (g4s_ilu0_apply_multi), every column bit for bit its own apply. factor(values=None): refactorise — new values in the layout of the
    analysed arrays as a device tensor (asynchronous, capturable) or a numpy array (copied in, synchronous), None: the values the handle holds;
    returns the int32 device word of the smallest row with a zero or non-finite pivot (−1: none), which the caller reads when they like. factors():
    a device tensor of the nnz factor values, L strictly below the diagonal, U on and above it. info: the dict of g4s_ilu0_info. close() releases
    the handle."""

    def __init__(self, handle, n, nnz, info):
        self._handle, self.n, self.nnz = handle, int(n), int(nnz)
        self.info = {n_: getattr(info, n_) for n_, _ in capi.ILU0Info._fields_}

    def _open(self):
        if self._handle is None:
            raise ValueError("the factorisation is closed")

    def apply(self, r, out=None):
        self._open()
        return _solve_rhs(self._handle, "g4s_ilu0_apply", "g4s_ilu0_apply_multi", r, out, self.n, "r")

    def factor(self, values=None):
        self._open()
        on_device = isinstance(values, torch.Tensor)
        if values is not None and (int(values.numel()) if on_device else int(np.asarray(values).size)) != self.nnz:
            raise ValueError(f"values must have the {self.nnz} entries of the analysed arrays")
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        fn = capi.load().g4s_ilu0_factor
        if values is None:
            capi.check(fn(self._handle, C.c_void_p(0), capi.DEVICE_POINTERS, _ptr_nn(bad), _stream()))
        elif on_device:
            assert values.is_cuda and values.dtype == torch.float64
            capi.check(fn(self._handle, _ptr_nn(values.contiguous()), capi.DEVICE_POINTERS, _ptr_nn(bad), _stream()))
        else:
            values = np.ascontiguousarray(values, np.float64)
            spare = np.zeros(1, np.float64)
            capi.check(fn(self._handle, C.c_void_p((values if values.size else spare).ctypes.data), capi.HOST_POINTERS, _ptr_nn(bad), _stream()))
        return bad

    def factors(self):
        self._open()
        out = torch.empty(self.nnz, dtype=torch.float64, device="cuda")
        capi.check(capi.load().g4s_ilu0_get_factors(self._handle, _ptr_nn(out), capi.DEVICE_POINTERS, _stream()))
        return out

    def close(self):
        if self._handle is not None:
            capi.load().g4s_ilu0_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ilu0(A, no_chains=False):
    """The ILU(0) factorisation (ILU0) of the square matrix A (g4s_ilu0_analyse): A ≈ L U with L and U on A's own pattern. A is a CSR, or a
    (rowptr, colids, values) triple of device tensors or of numpy arrays (host pointers). Its rows must be canonical — columns strictly ascending,
    every diagonal entry stored (csr_canonical gives such rows) —; anything else is refused (capi.G4SError; the message names the smallest offending
    row). A zero or non-finite pivot is no error: info["bad_pivot"] names the smallest such row, −1 when there is none. no_chains=True is the test
    switch G4S_ILU0_NO_CHAINS: one launch per level, the same bits. Synchronous. ValueError (before any GPU call) for a CSR that is not square, a
    tuple of the wrong length, arrays of mixed kinds, values that do not match colids, and a no_chains that is not a bool."""
    rowptr, colids, values, n = _triangle_args(A, (("no_chains", no_chains),))
    _require_gpu()
    flags = capi.ILU0_NO_CHAINS if no_chains else 0
    info, handle = capi.ILU0Info(), C.c_void_p()
    fn = capi.load().g4s_ilu0_analyse
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and values.is_cuda
        assert rowptr.dtype == torch.int32 and colids.dtype == torch.int32 and values.dtype == torch.float64
        rowptr, colids, values = rowptr.contiguous(), colids.contiguous(), values.contiguous()
        capi.check(fn(C.byref(handle), n, _ptr_nn(rowptr), _ptr_nn(colids), _ptr_nn(values), flags | capi.DEVICE_POINTERS, C.byref(info), _stream()))
        nnz = int(colids.numel())
    else:
        rowptr, colids, values = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32), np.ascontiguousarray(values, np.float64)
        spare = np.zeros(1, np.float64)                                 # an empty array is passed as a pointer that is not read
        P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
        capi.check(fn(C.byref(handle), n, P(rowptr), P(colids), P(values), flags | capi.HOST_POINTERS, C.byref(info), _stream()))
        nnz = int(colids.size)
    return ILU0(handle, n, nnz, info)


def pcg(A, b, M=None, x0=None, tol=1e-8, maxiter=None):
    """Preconditioned conjugate gradients on A x = b: (x, iterations, relative residual). A is a square CSR (symmetric positive definite for the
    method to mean anything), b a float64 device tensor of its rows, M an object with apply(r, out=None) — an ILU0 of A — or None (plain CG), x0 the
    start (None: zero; it is not modified). Stops at the first iteration whose recurred residual has ‖r‖ <= tol · ‖b‖, or at maxiter (None: rows).
    Wiring, no kernel of its own: the product is g4s_spmv, the preconditioner M.apply, the dots and vector updates torch. It reads two scalars per
    iteration back, so it is synchronous and not capturable."""
    if not isinstance(A, CSR):
        raise ValueError("A must be a CSR")
    if A.rows != A.cols:
        raise ValueError(f"conjugate gradients need a square matrix, not {A.rows} x {A.cols}")
    for name, v in (("b", b),) + ((("x0", x0),) if x0 is not None else ()):
        if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.dim() == 1 and v.numel() == A.rows):
            raise ValueError(f"{name} must be a float64 tensor of {A.rows} entries")
    if M is not None and not callable(getattr(M, "apply", None)):
        raise ValueError("M must be None or have apply(r, out=None)")
    if not (isinstance(tol, (float, np.floating)) and tol > 0.0):
        raise ValueError(f"tol must be a positive float, not {tol!r}")
    if maxiter is not None and not (isinstance(maxiter, (int, np.integer)) and not isinstance(maxiter, (bool, np.bool_)) and maxiter >= 0):
        raise ValueError(f"maxiter must be None or a non-negative integer, not {maxiter!r}")
    maxiter = A.rows if maxiter is None else int(maxiter)
    b = b.contiguous()
    x = torch.zeros_like(b) if x0 is None else x0.clone().contiguous()
    r = b.clone()
    if x0 is not None:
        A.spmv(x, r, alpha=-1.0, beta=1.0)
    bnorm = float(torch.linalg.vector_norm(b))
    stop = tol * bnorm
    rnorm = float(torch.linalg.vector_norm(r))
    if bnorm == 0.0:
        return torch.zeros_like(b), 0, 0.0
    z = r.clone() if M is None else M.apply(r)
    p = z.clone()
    q = torch.empty_like(b)
    rz = torch.dot(r, z)
    it = 0
    while rnorm > stop and it < maxiter:
        A.spmv(p, q)
        alpha = rz / torch.dot(p, q)
        x.add_(p * alpha)
        r.sub_(q * alpha)
        rnorm = float(torch.linalg.vector_norm(r))
        it += 1
        if rnorm <= stop:
            break
        if M is None:
            z.copy_(r)
        else:
            M.apply(r, out=z)
        rz_new = torch.dot(r, z)
        p.mul_(rz_new / rz).add_(z)
        rz = rz_new
    return x, it, rnorm / bnorm


def _is_truss(v):
    return _is_count(v) and 2 <= v <= capi.KTRUSS_FULL


def ktruss(A, max_k=None, return_round=False, return_support=False, return_info=False):
    """truss (int32 device tensor of nnz, one per stored entry): truss[p] = the largest k such that the edge stored at entry p belongs to a subgraph in
    which every edge lies in at least k − 2 triangles (g4s_ktruss) — the edges with truss >= k are networkx.k_truss(G, k) of the graph without
    self-loops. A is a CSR, or a (rowptr, colids) pair of int32 device tensors or of numpy arrays (host pointers; the results come back on the device
    all the same), and holds the SYMMETRIC pattern of a simple undirected graph with strictly ascending rows (csr_symmetrise gives one); both copies of
    an edge get the same values, a stored diagonal entry gets truss 0, round −1 and support 0. max_k: peel the levels below it only — the edges of the
    max_k-truss then get truss = max_k and round = −1; None is the full decomposition. return_round=True adds round (the index of the peel frontier
    that removed each edge), return_support=True adds support (the triangles through each edge in A), both int32 device tensors of nnz and functions
    of the graph alone. return_info=True adds the dict of g4s_ktruss_info. Synchronous; no plan is built. ValueError (before any GPU call) for a CSR
    that is not square, a max_k that is not an integer in [2, 2^31), and return_round / return_support / return_info that are not bools."""
    if max_k is not None and not _is_truss(max_k):
        raise ValueError(f"max_k must be None or an integer in [2, 2^31), not {max_k!r}")
    for name, v in (("return_round", return_round), ("return_support", return_support), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    rowptr, colids, n = _pattern_of(A, "a k-truss decomposition")
    _require_gpu()
    cap = capi.KTRUSS_FULL if max_k is None else int(max_k)
    info, null = capi.KTrussInfo(), C.c_void_p(0)
    if isinstance(rowptr, torch.Tensor):
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        nnz = int(colids.numel())
        truss = torch.empty(nnz, dtype=torch.int32, device=rowptr.device)
        rnd = torch.empty(nnz, dtype=torch.int32, device=rowptr.device) if return_round else None
        sup = torch.empty(nnz, dtype=torch.int32, device=rowptr.device) if return_support else None
        capi.check(capi.load().g4s_ktruss(n, _ptr_nn(rowptr), _ptr_nn(colids), cap, _ptr_nn(truss), _ptr_nn(rnd) if return_round else null,
                                          _ptr_nn(sup) if return_support else null, capi.DEVICE_POINTERS, C.byref(info), _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        nnz = int(colids.size)
        out, out_r, out_s = (np.empty(max(nnz, 1), np.int32) for _ in range(3))
        P = lambda a: C.c_void_p(a.ctypes.data)
        capi.check(capi.load().g4s_ktruss(n, P(rowptr), P(colids if colids.size else out), cap, P(out), P(out_r) if return_round else null,
                                          P(out_s) if return_support else null, capi.HOST_POINTERS, C.byref(info), _stream()))
        truss = torch.from_numpy(out[:nnz]).cuda()
        rnd = torch.from_numpy(out_r[:nnz]).cuda() if return_round else None
        sup = torch.from_numpy(out_s[:nnz]).cuda() if return_support else None
    res = ((truss,) + ((rnd,) if return_round else ()) + ((sup,) if return_support else ())
           + (({n_: getattr(info, n_) for n_, _ in capi.KTrussInfo._fields_},) if return_info else ()))
    return res[0] if len(res) == 1 else res


def ktruss_subgraph(A, k):
    """The k-truss of the square device CSR A — its largest subgraph in which every edge lies in at least k − 2 triangles — as a CSR on the same n
    vertices whose values are the truss numbers capped at k (so every stored value is k). A composition: ktruss with max_k = k, which peels the levels
    below k only, then csr_select("ge", thr=k) on a CSR that shares A's pattern and carries the truss numbers as values; stored diagonal entries
    (truss 0) go. ValueError (before any GPU call) for a matrix that is not square and a k that is not an integer in [2, 2^31)."""
    if not _is_truss(k):
        raise ValueError(f"k must be an integer in [2, 2^31), not {k!r}")
    if A.rows != A.cols:
        raise ValueError(f"a k-truss subgraph needs a square matrix, not {A.rows} x {A.cols}")
    truss = ktruss(A, max_k=int(k))
    return csr_select(CSR(A.rowptr, A.colids, truss.to(torch.float64), A.rows, A.cols), "ge", thr=float(k))


def degeneracy_order(A):
    """perm (int32 device tensor of n): the vertices sorted by (peel round, id) — a stable device sort of kcore's round. Every vertex has at most
    core[v] <= degeneracy neighbours at or after its own position, so csr_permute(A, perm) is a matrix in which every row has at most `degeneracy`
    entries at or right of its diagonal: the ordering a triangle count wants. A: as for kcore."""
    _, rnd = kcore(A, return_round=True)
    return torch.sort(rnd, stable=True).indices.to(torch.int32)


def kcore_subgraph(A, k):
    """(sub, ids): the k-core of the square device CSR A — its largest subgraph in which every vertex has at least k neighbours — as the subgraph induced
    by the vertices ids (ascending; vertex ids[p] of A is vertex p of sub). A composition: kcore with max_k = k, which peels the levels below k only,
    then csr_induced_subgraph on the vertices with core >= k. ValueError (before any GPU call) for a matrix that is not square and a k that is not a
    non-negative integer below 2^31."""
    if not (_is_count(k) and k <= capi.KCORE_FULL):
        raise ValueError(f"k must be a non-negative integer below 2^31, not {k!r}")
    if A.rows != A.cols:
        raise ValueError(f"a k-core subgraph needs a square matrix, not {A.rows} x {A.cols}")
    return csr_induced_subgraph(A, kcore(A, max_k=int(k)) >= int(k))


def _is_seed(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= v < 2**32


def color(A, key=None, seed=0, largest_first=False, return_round=False, return_info=False):
    """color (int32 device tensor of n): the first-fit colouring of the graph in decreasing priority (g4s_color) — color[v] is the smallest colour not
    held by a neighbour above v, what networkx.greedy_color returns for that order on the graph without self-loops. A is a CSR, or a (rowptr, colids)
    pair of int32 device tensors or of numpy arrays (host pointers; the results come back on the device all the same), and holds the SYMMETRIC pattern
    of a simple undirected graph with strictly ascending rows (csr_symmetrise gives one); a stored diagonal entry is ignored. The priority is the pair
    (key[v], fmix32(v ^ seed)), larger first: key=None is a pure hash order, key = kcore's round is smallest-last (color_smallest_last),
    largest_first=True takes the degree as the key (key must then be None). key: n int32 values of the kind of A's arrays. return_round=True adds
    round (int32 device tensor): the depth of each vertex in the priority DAG. return_info=True adds the dict of g4s_color_info. Both outputs are
    functions of graph, key and seed alone. Synchronous; no plan is built. ValueError (before any GPU call) for a CSR that is not square, a seed that
    is not an integer in [0, 2^32), a key together with largest_first, a key of the wrong length or kind, and flags that are not bools."""
    if not _is_seed(seed):
        raise ValueError(f"seed must be an integer in [0, 2^32), not {seed!r}")
    for name, v in (("largest_first", largest_first), ("return_round", return_round), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    if largest_first and key is not None:
        raise ValueError("key must be None with largest_first=True: the degree is the key")
    rowptr, colids, n = _pattern_of(A, "a colouring")
    on_device = isinstance(rowptr, torch.Tensor)
    if key is not None:
        if isinstance(key, torch.Tensor) != on_device:
            raise ValueError("key must be of the kind of the pattern's arrays: a device tensor with device tensors, a numpy array with numpy arrays")
        if int(key.numel() if on_device else np.asarray(key).size) != n:
            raise ValueError(f"key must hold one value per vertex ({n})")
        if on_device and key.dtype != torch.int32:
            raise ValueError(f"key must be int32, not {key.dtype}")
    _require_gpu()
    flags = capi.COLOR_LARGEST_FIRST if largest_first else 0
    info, null = capi.ColorInfo(), C.c_void_p(0)
    if on_device:
        assert rowptr.is_cuda and colids.is_cuda and rowptr.dtype == torch.int32 and colids.dtype == torch.int32
        rowptr, colids = rowptr.contiguous(), colids.contiguous()
        key = key.contiguous() if key is not None else None
        col = torch.empty(n, dtype=torch.int32, device=rowptr.device)
        rnd = torch.empty(n, dtype=torch.int32, device=rowptr.device) if return_round else None
        capi.check(capi.load().g4s_color(n, _ptr_nn(rowptr), _ptr_nn(colids), _ptr_nn(key) if key is not None and n else null, int(seed), _ptr_nn(col),
                                         _ptr_nn(rnd) if return_round else null, flags | capi.DEVICE_POINTERS, C.byref(info), _stream()))
    else:
        rowptr, colids = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colids, np.int32)
        key = np.ascontiguousarray(key, np.int32) if key is not None else None
        out, out_r = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        capi.check(capi.load().g4s_color(n, P(rowptr), P(colids if colids.size else out), P(key) if key is not None and n else null, int(seed), P(out),
                                         P(out_r) if return_round else null, flags | capi.HOST_POINTERS, C.byref(info), _stream()))
        col = torch.from_numpy(out[:n]).cuda()
        rnd = torch.from_numpy(out_r[:n]).cuda() if return_round else None
    res = (col,) + ((rnd,) if return_round else ()) + (({n_: getattr(info, n_) for n_, _ in capi.ColorInfo._fields_ if n_ != "reserved"},) if return_info else ())
    return res[0] if len(res) == 1 else res


def color_smallest_last(A, seed=0, return_info=False):
    """The smallest-last colouring: color with key = kcore's peel round, i.e. greedy colouring in the reverse of the degeneracy ordering. It uses at
    most degeneracy + 1 colours. A: as for color."""
    _, rnd = kcore(A, return_round=True)
    rowptr = _pattern_of(A, "a colouring")[0]
    return color(A, key=rnd if isinstance(rowptr, torch.Tensor) else rnd.cpu().numpy(), seed=seed, return_info=return_info)


def maximal_independent_set(A, key=None, seed=0):
    """A bool device tensor of n: the greedy maximal independent set in priority order — colour class 0 of color(A, key, seed)."""
    return color(A, key=key, seed=seed) == 0


def color_classes(color):
    """(perm, offsets): perm (int32 device tensor of n) = the vertices sorted by (colour, id), ready for csr_permute; offsets (int64 device tensor of
    colours + 1) = where each colour class starts in perm. No stored off-diagonal entry of the permuted matrix lies inside a diagonal block
    [offsets[c], offsets[c + 1])². color: the int32 device tensor that color() returns."""
    if not (isinstance(color, torch.Tensor) and color.dim() == 1 and color.dtype == torch.int32):
        raise ValueError("color must be a one-dimensional int32 tensor")
    perm = torch.sort(color, stable=True).indices.to(torch.int32)
    offsets = torch.zeros(int(color.max()) + 2 if color.numel() else 1, dtype=torch.int64, device=color.device)
    if color.numel():
        offsets[1:] = torch.cumsum(torch.bincount(color), 0)
    return perm, offsets


# ------------------------------------------------------------------------------------------------ element-wise combination and select
EWISE_OPS = {"union": capi.EWISE_UNION, "intersect": capi.EWISE_INTERSECT, "difference": capi.EWISE_DIFFERENCE}
COMBINERS = {"plus": capi.COMBINE_PLUS, "times": capi.COMBINE_TIMES, "min": capi.COMBINE_MIN, "max": capi.COMBINE_MAX, "first": capi.COMBINE_FIRST,
             "second": capi.COMBINE_SECOND}
SELECT_PREDICATES = {"tril": capi.SELECT_TRIL, "triu": capi.SELECT_TRIU, "offdiag": capi.SELECT_OFFDIAG, "diag": capi.SELECT_DIAG,
                     "nonzero": capi.SELECT_NONZERO, "gt": capi.SELECT_GT, "ge": capi.SELECT_GE, "lt": capi.SELECT_LT, "le": capi.SELECT_LE}


def _name(table, value, what):
    if not isinstance(value, str) or value not in table:
        raise ValueError(f"unknown {what} {value!r}; expected one of {sorted(table)}")
    return table[value]


def csr_ewise(a, b, op="union", combine="plus", pattern_only=False, return_info=False):
    """A ∪ B ("union"), A ∩ B ("intersect") or A ∖ B ("difference": the entries of A whose position B does not store, with A's values) of two device
    CSRs of one shape, as a new device CSR (g4s_csr_ewise_symbolic / g4s_csr_ewise_numeric). combine — "plus", "times", "min", "max", "first",
    "second" — gives the value where both store a position; under union an entry of one matrix alone is copied. Rows of a and b must be strictly
    ascending; the result's are. A stored position is an entry whatever its value: explicit zeros and sums equal to 0.0 stay stored. b may be a.
    pattern_only=True reads no values: the result's values are all 1.0. Synchronous. return_info=True adds the dict of g4s_ewise_info.
    ValueError (before any GPU call) for an unknown op or combine and for shapes that differ."""
    opv, cv = _name(EWISE_OPS, op, "op"), _name(COMBINERS, combine, "combine")
    if (a.rows, a.cols) != (b.rows, b.cols):
        raise ValueError(f"element-wise {op} needs one shape, not {a.rows} x {a.cols} and {b.rows} x {b.cols}")
    _require_gpu()
    lib, dev = capi.load(), a.rowptr.device
    crp = torch.empty(a.rows + 1, dtype=torch.int32, device=dev)
    cnnz, info = C.c_int64(0), capi.EwiseInfo()
    capi.check(lib.g4s_csr_ewise_symbolic(opv, a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), _ptr_nn(b.rowptr), _ptr_nn(b.colids), _ptr_nn(crp),
                                          C.byref(cnnz), capi.DEVICE_POINTERS, C.byref(info), _stream()))
    cci = torch.empty(cnnz.value, dtype=torch.int32, device=dev)
    cva = torch.ones(cnnz.value, dtype=torch.float64, device=dev) if pattern_only else torch.empty(cnnz.value, dtype=torch.float64, device=dev)
    null = C.c_void_p(0)
    capi.check(lib.g4s_csr_ewise_numeric(opv, cv, a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), null if pattern_only else _ptr_nn(a.values),
                                         _ptr_nn(b.rowptr), _ptr_nn(b.colids), null if pattern_only else _ptr_nn(b.values), _ptr_nn(crp), _ptr_nn(cci),
                                         null if pattern_only else _ptr_nn(cva), capi.DEVICE_POINTERS, _stream()))
    c = CSR(crp, cci, cva, a.rows, a.cols)
    return (c, {n: getattr(info, n) for n, _ in capi.EwiseInfo._fields_}) if return_info else c


def csr_select(a, pred, k=0, thr=0.0):
    """The entries of the device CSR a that satisfy pred, in their stored order and with their bits, as a new device CSR (g4s_csr_select_symbolic /
    g4s_csr_select_numeric): "tril" col − row <= k, "triu" col − row >= k, "offdiag", "diag", "nonzero" value != 0, "gt" / "ge" / "lt" / "le" value
    against thr (NaN fails all four and passes "nonzero"). Rows may be in any order, with repeats. Synchronous. ValueError (before any GPU call) for
    an unknown pred, a k that is not an integer and a thr that is not a number."""
    pv = _name(SELECT_PREDICATES, pred, "pred")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an integer, not {k!r}")
    if isinstance(thr, (bool, np.bool_)) or not isinstance(thr, (int, float, np.integer, np.floating)):
        raise ValueError(f"thr must be a number, not {thr!r}")
    _require_gpu()
    lib, dev = capi.load(), a.rowptr.device
    crp = torch.empty(a.rows + 1, dtype=torch.int32, device=dev)
    cnnz = C.c_int64(0)
    capi.check(lib.g4s_csr_select_symbolic(pv, int(k), float(thr), a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), _ptr_nn(a.values), _ptr_nn(crp),
                                           C.byref(cnnz), capi.DEVICE_POINTERS, _stream()))
    cci = torch.empty(cnnz.value, dtype=torch.int32, device=dev)
    cva = torch.empty(cnnz.value, dtype=torch.float64, device=dev)
    capi.check(lib.g4s_csr_select_numeric(pv, int(k), float(thr), a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), _ptr_nn(a.values), _ptr_nn(crp),
                                          _ptr_nn(cci), _ptr_nn(cva), capi.DEVICE_POINTERS, _stream()))
    return CSR(crp, cci, cva, a.rows, a.cols)


def csr_symmetrise(a, combine="max", drop_diagonal=False):
    """A ∪ Aᵀ of a square device CSR with strictly ascending rows, as a new device CSR whose pattern is symmetric — what G4S_CC_SYMMETRIC,
    G4S_PAGERANK_SYMMETRIC, G4S_TRAVERSE_SYMMETRIC and g4s_triangle_count ask for. A composition: g4s_csr_transpose, a union with `combine` where
    both (i, j) and (j, i) are stored ("max" and "plus" give a symmetric matrix; "first" keeps A's value), then an "offdiag" select with
    drop_diagonal=True. ValueError (before any GPU call) for a matrix that is not square, an unknown combine and a drop_diagonal that is not a bool."""
    _name(COMBINERS, combine, "combine")
    if not isinstance(drop_diagonal, (bool, np.bool_)):
        raise ValueError(f"drop_diagonal must be a bool, not {drop_diagonal!r}")
    if a.rows != a.cols:
        raise ValueError(f"symmetrise needs a square matrix, not {a.rows} x {a.cols}")
    s = csr_ewise(a, a.transpose(), "union", combine)
    return csr_select(s, "offdiag") if drop_diagonal else s


# ------------------------------------------------------------------------------------------------ CSR from an edge list
DUPLICATES = {"keep": capi.DUP_KEEP, **COMBINERS}


def _coo_info(info):
    return {n: getattr(info, n) for n, _ in capi.CooInfo._fields_ if n != "reserved"}


def _coo_shape(row, col, rows, cols, symmetric):
    """rows and cols of an edge list: what was given, else the largest id + 1; one number for a symmetric list."""
    if rows is None:
        rows = int(row.max().item()) + 1 if row.numel() else 0
    if cols is None:
        cols = int(col.max().item()) + 1 if col.numel() else 0
    if symmetric:
        rows = cols = max(rows, cols)
    return int(rows), int(cols)


def csr_from_coo(row, col, val=None, rows=None, cols=None, dup="plus", symmetric=False, return_perm=False, return_info=False):
    """(rowptr, colids, values-or-None) of the rows × cols CSR that the triples (row[i], col[i], val[i]) describe — int32 / int32 / float64 device
    tensors in any order, with repeats (g4s_csr_from_coo_symbolic / g4s_csr_from_coo_numeric). dup: "keep" — every triple stays an entry, rows
    ascending, repeats in input order — or "plus", "times", "min", "max", "first", "second": one entry per position, rows strictly ascending, the
    value folded from left to right over the repeats in input order. val=None: the pattern only. rows / cols default to the largest id + 1.
    symmetric=True appends the mirrored copy (col, row, val) of every off-diagonal triple behind the originals first (the mirror of the
    reference's reader, mm/inc/CSR.h:586-623); rows and cols are then one number. return_perm=True adds perm — the index, in the (concatenated)
    list, of the triple behind every sorted position — and return_info=True the dict of g4s_coo_info. Synchronous. ValueError (before any GPU
    call) for an unknown dup, flags that are not bools and sizes that are not integers."""
    dv = _name(DUPLICATES, dup, "dup")
    for name, v in (("symmetric", symmetric), ("return_perm", return_perm), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    for name, v in (("rows", rows), ("cols", cols)):
        if v is not None and (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"{name} must be a non-negative integer or None, not {v!r}")
    if symmetric and rows is not None and cols is not None and rows != cols:
        raise ValueError(f"symmetric=True needs a square matrix, not {rows} x {cols}")
    _require_gpu()
    assert row.is_cuda and col.is_cuda and row.dtype == torch.int32 and col.dtype == torch.int32 and row.numel() == col.numel()
    assert val is None or (val.is_cuda and val.dtype == torch.float64 and val.numel() == row.numel())
    row, col = row.contiguous(), col.contiguous()
    if symmetric:
        off = row != col
        row, col = torch.cat([row, col[off]]), torch.cat([col, row[off]])
        val = None if val is None else torch.cat([val, val[off]])
    val = None if val is None else val.contiguous()
    nnz, dev = row.numel(), row.device
    rows, cols = _coo_shape(row, col, rows, cols, symmetric)
    lib = capi.load()
    crp = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(nnz, dtype=torch.int32, device=dev)
    cnnz, info, null = C.c_int64(0), capi.CooInfo(), C.c_void_p(0)
    capi.check(lib.g4s_csr_from_coo_symbolic(dv, rows, cols, nnz, _ptr_nn(row), _ptr_nn(col), _ptr_nn(crp), _ptr_nn(perm), C.byref(cnnz), capi.DEVICE_POINTERS,
                                             C.byref(info), _stream()))
    cci = torch.empty(cnnz.value, dtype=torch.int32, device=dev)
    cva = None if val is None else torch.empty(cnnz.value, dtype=torch.float64, device=dev)
    capi.check(lib.g4s_csr_from_coo_numeric(dv, rows, cols, nnz, _ptr_nn(row), _ptr_nn(col), null if val is None else _ptr_nn(val), _ptr_nn(crp), _ptr_nn(perm),
                                            _ptr_nn(cci), null if val is None else _ptr_nn(cva), capi.DEVICE_POINTERS, _stream()))
    out = (crp, cci, cva)
    if return_perm:
        out += (perm,)
    if return_info:
        out += (_coo_info(info),)
    return out


def csr_row_indices(rowptr, nnz):
    """The row of every stored entry of a CSR (g4s_csr_row_indices): an int32 device tensor of nnz — with colids and values, the matrix as a COO.
    rowptr: an int32 device tensor, zero-based, non-decreasing and ending at nnz (checked on the device). Synchronous."""
    if isinstance(nnz, (bool, np.bool_)) or not isinstance(nnz, (int, np.integer)) or nnz < 0:
        raise ValueError(f"nnz must be a non-negative integer, not {nnz!r}")
    _require_gpu()
    assert rowptr.is_cuda and rowptr.dtype == torch.int32 and rowptr.numel() >= 1
    rowptr = rowptr.contiguous()
    out = torch.empty(int(nnz), dtype=torch.int32, device=rowptr.device)
    capi.check(capi.load().g4s_csr_row_indices(rowptr.numel() - 1, int(nnz), _ptr_nn(rowptr), _ptr_nn(out), capi.DEVICE_POINTERS, _stream()))
    return out


def csr_canonical(a, dup="plus"):
    """The device CSR a with every row sorted by column and repeats merged by `dup` (a name of DUPLICATES; "keep" only sorts), as a new device CSR:
    g4s_csr_row_indices followed by csr_from_coo. What csr_ewise, spgemm_masked and triangle_count ask of their inputs. Stable: repeats are folded,
    or kept, in their stored order. ValueError (before any GPU call) for an unknown dup."""
    _name(DUPLICATES, dup, "dup")
    rp, ci, va = csr_from_coo(csr_row_indices(a.rowptr, a.nnz), a.colids, a.values, a.rows, a.cols, dup)
    return CSR(rp, ci, va, a.rows, a.cols)


# ------------------------------------------------------------------------------------------------ extract: A[I, J]
def _extract_info(info):
    return {n: getattr(info, n) for n, _ in capi.ExtractInfo._fields_ if n != "reserved"}


def _id_list(t, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_cuda:
        raise ValueError(f"{name} must be a one-dimensional int32 device tensor or None")
    return t.contiguous()


def csr_extract(a, I=None, J=None, pattern_only=False, return_src=False, return_info=False):
    """C = A[I, J] as a new device CSR of len(I) × len(J): C(p, q) is stored exactly where A(I[p], J[q]) is (g4s_csr_extract_symbolic /
    g4s_csr_extract_numeric) — MATLAB's A(I, J). I and J are int32 device tensors of ids in any order, with repeats, or None for every row / every
    column in order. Rows of a may be in any order and may repeat a column; every output row is ordered by (q, stored position in a's row), so a
    canonical a gives strictly ascending rows. pattern_only=True reads no values: the result's values are all 1.0. return_src=True adds src, the
    index into a.colids / a.values behind every entry of C (C.values == a.values[src], bit for bit); return_info=True the dict of g4s_extract_info.
    Synchronous. ValueError (before any GPU call) for flags that are not bools and for an I or J that is not a one-dimensional int32 device tensor."""
    for name, v in (("pattern_only", pattern_only), ("return_src", return_src), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    I, J = _id_list(I, "I"), _id_list(J, "J")
    _require_gpu()
    ni, nj = (a.rows if I is None else I.numel()), (a.cols if J is None else J.numel())
    lib, dev, null = capi.load(), a.rowptr.device, C.c_void_p(0)
    pi, pj = (null if I is None else _ptr_nn(I)), (null if J is None else _ptr_nn(J))
    crp = torch.empty(ni + 1, dtype=torch.int32, device=dev)
    cnnz, info = C.c_int64(0), capi.ExtractInfo()
    capi.check(lib.g4s_csr_extract_symbolic(a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), ni, pi, nj, pj, _ptr_nn(crp), C.byref(cnnz), capi.DEVICE_POINTERS,
                                            C.byref(info), _stream()))
    cci = torch.empty(cnnz.value, dtype=torch.int32, device=dev)
    cva = torch.ones(cnnz.value, dtype=torch.float64, device=dev) if pattern_only else torch.empty(cnnz.value, dtype=torch.float64, device=dev)
    src = torch.empty(cnnz.value, dtype=torch.int32, device=dev) if return_src else None
    capi.check(lib.g4s_csr_extract_numeric(a.rows, a.cols, _ptr_nn(a.rowptr), _ptr_nn(a.colids), null if pattern_only else _ptr_nn(a.values), ni, pi, nj, pj,
                                           _ptr_nn(crp), _ptr_nn(cci), null if pattern_only else _ptr_nn(cva), null if src is None else _ptr_nn(src),
                                           capi.DEVICE_POINTERS, C.byref(info), _stream()))
    out = (CSR(crp, cci, cva, ni, nj),)
    if return_src:
        out += (src,)
    if return_info:
        out += (_extract_info(info),)
    return out[0] if len(out) == 1 else out


def csr_permute(a, perm):
    """A[perm, perm] of a square device CSR: vertex perm[p] of a becomes vertex p — csr_extract(a, perm, perm). perm: an int32 device tensor of
    a.rows ids (a permutation relabels; the call itself accepts any ids). ValueError (before any GPU call) for a matrix that is not square and for
    a perm whose length is not a.rows."""
    if a.rows != a.cols:
        raise ValueError(f"permute needs a square matrix, not {a.rows} x {a.cols}")
    if perm is None or not hasattr(perm, "numel") or perm.numel() != a.rows:
        raise ValueError(f"perm must hold {a.rows} ids, one per vertex")
    return csr_extract(a, perm, perm)


def csr_induced_subgraph(a, vertices):
    """(A[ids, ids], ids): the subgraph of the square device CSR a induced by `vertices` — an int32 device tensor of ids, used in the order given,
    or a bool device mask of a.rows (its True positions in ascending order, through torch.nonzero). Vertex ids[p] of a is vertex p of the result.
    ValueError (before any GPU call) for a matrix that is not square and for a mask of the wrong length."""
    if a.rows != a.cols:
        raise ValueError(f"an induced subgraph needs a square matrix, not {a.rows} x {a.cols}")
    if getattr(vertices, "dtype", None) == torch.bool:
        if vertices.numel() != a.rows:
            raise ValueError(f"a vertex mask must hold {a.rows} flags, not {vertices.numel()}")
        vertices = torch.nonzero(vertices.reshape(-1)).reshape(-1).to(torch.int32)
    return csr_extract(a, vertices, vertices), vertices


def csr_submatrix(a, M, N, M_start=0, N_start=0):
    """The M × N block of a that starts at (M_start, N_start) — the reference's CSR(const CSR&, M_, N_, M_start, N_start) (mm/inc/CSR.h:691-733),
    argument order included — through csr_extract with torch.arange lists. ValueError (before any GPU call) for sizes that are not non-negative
    integers and for a block that leaves the matrix."""
    for name, v in (("M", M), ("N", N), ("M_start", M_start), ("N_start", N_start)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{name} must be a non-negative integer, not {v!r}")
    if M_start + M > a.rows or N_start + N > a.cols:
        raise ValueError(f"the block [{M_start}, {M_start + M}) x [{N_start}, {N_start + N}) leaves the {a.rows} x {a.cols} matrix")
    dev = a.rowptr.device
    return csr_extract(a, torch.arange(M_start, M_start + M, dtype=torch.int32, device=dev), torch.arange(N_start, N_start + N, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ synthetic inputs
def rmat_csr(n, scale, edges, seed, device="cuda", chunk=1 << 26, **kw):
    """R-MAT (0.57,0.19,0.19,0.05) on n vertices: `edges` draws, duplicates merged, rows sorted by column, values
    U(−1,1) of (seed,row,col) — SURVEY.md §8d C2. Built entirely in HBM (generator kernels + torch sort/unique)."""
    _require_gpu()
    lib = capi.load()
    keys = torch.empty(edges, dtype=torch.int64, device=device)
    for e0 in range(0, edges, chunk):
        cnt = min(chunk, edges - e0)
        capi.check(lib.g4s_synth_rmat_keys(seed, scale, n, e0, cnt, C.c_void_p(keys.data_ptr() + 8 * e0), _stream()))
    keys = torch.unique(keys, sorted=True)
    nnz = keys.numel()
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=device)
    colids = torch.empty(nnz, dtype=torch.int32, device=device)
    values = torch.empty(nnz, dtype=torch.float64, device=device)
    capi.check(lib.g4s_synth_csr_from_keys(seed, n, n, _ptr(keys), nnz, _ptr(rowptr), _ptr(colids), _ptr(values), _stream()))
    torch.cuda.synchronize()
    del keys
    return CSR(rowptr, colids, values, n, n, **kw)


def synth_vector(seed, count, i0=0, device="cuda"):
    _require_gpu()
    x = torch.empty(count, dtype=torch.float64, device=device)
    capi.check(capi.load().g4s_synth_vector(seed, i0, count, _ptr(x), _stream()))
    return x


def laplacian_csr(kind, nx, ny, nz=1, r0=0, r1=None, device="cuda", **kw):
    """Rows [r0,r1) of the 5-point (kind=5, nz=1, diag 4) or 7-point (kind=7, diag 6) Laplacian, global columns."""
    _require_gpu()
    lib = capi.load()
    n = nx * ny * nz
    r1 = n if r1 is None else r1
    m = r1 - r0
    counts = torch.empty(m, dtype=torch.int32, device=device)
    capi.check(lib.g4s_synth_laplacian_rows(kind, nx, ny, nz, r0, r1, _ptr(counts), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), 0,
                                            _stream()))
    rowptr = torch.zeros(m + 1, dtype=torch.int32, device=device)
    rowptr[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
    nnz = int(rowptr[-1].item())
    colids = torch.empty(nnz, dtype=torch.int32, device=device)
    values = torch.empty(nnz, dtype=torch.float64, device=device)
    capi.check(lib.g4s_synth_laplacian_rows(kind, nx, ny, nz, r0, r1, C.c_void_p(0), _ptr(rowptr), _ptr(colids), _ptr(values), 1,
                                            _stream()))
    torch.cuda.synchronize()
    return CSR(rowptr, colids, values, m, n, **kw)


def banded_csr(n, hb, seed, device="cuda", **kw):
    _require_gpu()
    full = n * (2 * hb + 1)
    nnz = full - hb * (hb + 1)  # each side loses 1+2+…+hb entries
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=device)
    colids = torch.empty(nnz, dtype=torch.int32, device=device)
    values = torch.empty(nnz, dtype=torch.float64, device=device)
    capi.check(capi.load().g4s_synth_banded(n, hb, seed, _ptr(rowptr), _ptr(colids), _ptr(values), _stream()))
    torch.cuda.synchronize()
    return CSR(rowptr, colids, values, n, n, **kw)
