"""Inputs for the kernels of the gather/apply graph interface (g4s_amd/csrc/graph.hip) — the element-block mat-vec, the fp64-MFMA dense products with
their gradients, the symmetric quadratic form — at every kernel instantiation and on both sides of every selection threshold, plus numpy restatements of
the three selection rules (forward / dxx dispatch, the launch geometry of dw, fixed8 against generic) and numpy.longdouble restatements of the four
operations. numpy only: no GPU, no torch.

Each restated rule returns exactly the fields of the line the library prints under G4S_DEBUG; *_line() formats them as the library does.
tests/test_graph_cases_cpu.py proves that every case has the property its name claims; tests/test_graph_kernels_gpu.py runs them."""
import functools
import zlib
from typing import NamedTuple, Optional

import numpy as np

# ---- selection thresholds, each beside the source line it mirrors (graph.hip, dense_rows_times_matrix_launch unless another function is named)
PERSIST_MIN_M = 4096             # `M >= 4096` of both resident kernels
PERSIST_MAX_NK = 128             # `N <= 128 && K <= 128`
RESIDENT2_KT = (2, 4, 7, 8)      # `(KT == 2 || KT == 4 || KT == 7 || KT == 8)`
RESIDENT2_GT = (4, 7, 13, 16)    # `(G == 4 || G == 7 || G == 13 || (G == 16 && KT <= 4))`
RESIDENT2_GT16_MAX_KT = 4        # (the same line)
RESIDENT2_LDS = 140 * 1024       # `lds2 <= 140 * 1024`, lds2 = 8 bytes · 8·G · 16·KT
RESIDENT_LDS = 96 * 1024         # `lds <= 96 * 1024`, lds = 8 bytes · 4·NS · 16·KT
PERSIST_GRID = 256               # `grid = std::min(256, (strips + 7) / 8)`: 8 waves of a workgroup take one 16-row strip each
PANEL_ROWS = 64                  # dense_rows_times_matrix_kernel: one workgroup per 64 rows
PANEL_COLS = 128                 # kGemmNC: columns of the result per pass of the panel kernel
DW_SLAB = 16                     # G4S_DW_SLAB
DW_WGS = 512                     # G4S_DW_WGS
DW_BLOCK = 128                   # dense_rows_transposed_times_rows_kernel: one workgroup per 128 × 128 block of dw
QUAD_THREADS = 256               # sym_quadratic_form_kernel: thread t owns rows t, t + 256, …
ELEM_MAX_DOF = 4                 # kMaxDof
ELEM_TERMS_PER_ROUND = 8         # elem_matvec_kernel: `for (int tb = t0; tb < t1; tb += 8)`
ELEM_NODES_PER_WG = 4            # one wavefront per node, 4 per workgroup


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the selection rules, restated
def forward_dispatch(M, N, K, wt=False, aligned16=True):
    """The kernel dense_rows_times_matrix_launch<WT> picks for result[M×K] = xx[M×N]·w[N×K] (M, K > 0) and its launch, as a dict:
    {"kernel": "resident2", "KT", "GT", "WT", "grid"} / {"kernel": "resident", "KT", "NS", "WT", "grid"} / {"kernel": "panel", "WT", "grid"}.
    aligned16: the left operand (xx, or grad for dxx) sits on a 16-byte boundary. dxx of a grad call (M, N, K) is forward_dispatch(M, K, N, wt=True)."""
    assert M > 0 and K > 0 and N >= 0
    KT, NS, G = _cdiv(K, 16), _cdiv(N, 4), _cdiv(N, 8)
    lds = 8 * 4 * NS * 16 * KT
    lds2 = 8 * 8 * G * 16 * KT
    grid = min(PERSIST_GRID, _cdiv(_cdiv(M, 16), 8))
    small = N <= PERSIST_MAX_NK and K <= PERSIST_MAX_NK and M >= PERSIST_MIN_M
    if (small and N >= 2 and N % 2 == 0 and KT in RESIDENT2_KT and G in RESIDENT2_GT and (G != 16 or KT <= RESIDENT2_GT16_MAX_KT)
            and lds2 <= RESIDENT2_LDS and aligned16):
        return {"kernel": "resident2", "KT": KT, "GT": G, "WT": int(wt), "grid": grid}
    if small and N >= 1 and lds <= RESIDENT_LDS:
        return {"kernel": "resident", "KT": KT, "NS": NS, "WT": int(wt), "grid": grid}
    return {"kernel": "panel", "WT": int(wt), "grid": _cdiv(M, PANEL_ROWS)}


def forward_line(d):
    if d["kernel"] == "resident2":
        return "g4s dense rows x matrix: resident2 KT=%d GT=%d WT=%d grid=%d" % (d["KT"], d["GT"], d["WT"], d["grid"])
    if d["kernel"] == "resident":
        return "g4s dense rows x matrix: resident KT=%d NS=%d WT=%d grid=%d" % (d["KT"], d["NS"], d["WT"], d["grid"])
    return "g4s dense rows x matrix: panel WT=%d grid=%d" % (d["WT"], d["grid"])


def strip_iterations(M):
    """(most, waves) — the most iterations of the persistent strip loop any wavefront of a resident kernel takes at M rows, and how many wavefronts
    take that many: wave w of workgroup b starts at strip 8b + w and advances by 8·grid."""
    strips = _cdiv(M, 16)
    stride = 8 * min(PERSIST_GRID, _cdiv(strips, 8))
    most = _cdiv(strips, stride)
    return most, strips - (most - 1) * stride


def dw_geometry(M, N, K):
    """The launch of dw[N×K] = xxᵀ·grad (g4s_dense_rows_times_matrix_grad; M, N, K > 0): the template argument, the rows of one range, the ranges
    that hold rows, and the grid of 128 × 128 blocks of dw (y over N, z over K)."""
    assert M > 0 and N > 0 and K > 0
    wgs = min(DW_WGS, _cdiv(M, DW_SLAB))
    rows_per_wg = _cdiv(_cdiv(M, wgs), DW_SLAB) * DW_SLAB
    return {"KT": 8 if K > DW_BLOCK else _cdiv(K, 16), "rows_per_wg": rows_per_wg, "ranges": _cdiv(M, rows_per_wg),
            "by": _cdiv(N, DW_BLOCK), "bz": _cdiv(K, DW_BLOCK)}


def dw_line(d):
    return "g4s dense dw: KT=%d rows_per_wg=%d ranges=%d blocks=%dx%d" % (d["KT"], d["rows_per_wg"], d["ranges"], d["by"], d["bz"])


def dw_row_tiles(N, block, wave):
    """`ntl` of wave `wave` in block-row `block` of dw: how many of its two 16-row tiles (wave, wave + 4) hold real rows."""
    rem = min(N - DW_BLOCK * block, DW_BLOCK)
    return sum(1 for tile in (wave, wave + 4) if 16 * tile < rem)


def max_terms(ien, nno):
    """The largest number of (element, local node) terms that scatter into one node."""
    return int(np.bincount(np.asarray(ien).ravel(), minlength=max(nno, 1)).max()) if np.asarray(ien).size else 0


def elem_dispatch(ien, nno, npe, dof):
    """g4s_elem_op_create's choice: {"kernel": "fixed8"} or {"kernel": "generic", "npe", "dof", "max_terms"}."""
    mt = max_terms(ien, nno)
    if npe == 8 and dof == 3 and mt <= 8 and nno > 0:
        return {"kernel": "fixed8"}
    return {"kernel": "generic", "npe": npe, "dof": dof, "max_terms": mt}


def elem_line(d):
    if d["kernel"] == "fixed8":
        return "g4s element mat-vec: fixed8"
    return "g4s element mat-vec: generic npe=%d dof=%d max_terms=%d" % (d["npe"], d["dof"], d["max_terms"])


# ------------------------------------------------------------------------------------------------ data
KINDS = ("int", "real")


def _rng(name, kind):
    return np.random.default_rng([zlib.crc32(name.encode()), KINDS.index(kind)])


def values(rng, shape, kind):
    """"int": asymmetric integers in [−3, 3] (every sum of the cases stays far below 2^53: exact in any order); "real": U(−1, 1)."""
    if kind == "int":
        return rng.integers(-3, 4, shape).astype(np.float64)
    return rng.uniform(-1, 1, shape)


# ------------------------------------------------------------------------------------------------ dense cases
class DenseCase(NamedTuple):
    name: str
    mode: str                    # "forward": result = xx·w;  "grad": dxx = grad·wᵀ and dw = xxᵀ·grad
    M: int
    N: int
    K: int
    kernel: Optional[str]        # the kernel of the forward / dxx product the case is built to take (None: no product is launched)
    targs: dict                  # its claimed template arguments: KT and GT (resident2), KT (resident), nothing (panel)
    misaligned: bool = False     # the left operand of that product (xx, or grad) starts 8 bytes past a 16-byte boundary
    claims: dict = {}            # what else the name promises (checked by tests/test_graph_cases_cpu.py)

    def dispatch(self):
        """The restated rule's answer for the forward / dxx product of this case, or None where none is launched."""
        if self.mode == "forward":
            return forward_dispatch(self.M, self.N, self.K, False, not self.misaligned) if self.M > 0 and self.K > 0 else None
        return forward_dispatch(self.M, self.K, self.N, True, not self.misaligned) if self.M > 0 and self.N > 0 else None

    def dw(self):
        return dw_geometry(self.M, self.N, self.K) if self.mode == "grad" and self.M > 0 and self.N > 0 and self.K > 0 else None


def dense_operands(case, kind):
    """xx[M×N], w[N×K] and, for a grad case, grad[M×K]."""
    rng = _rng(case.name, kind)
    shapes = [(case.M, case.N), (case.N, case.K)] + ([(case.M, case.K)] if case.mode == "grad" else [])
    return tuple(values(rng, s, kind) for s in shapes)


R2_K = {2: (17, 32), 4: (49, 64), 7: (97, 112), 8: (113, 128)}       # K at the low / high end of the column-tile count: low = one real column in the last tile
R2_N = {4: (26, 32), 7: (50, 56), 13: (98, 104), 16: (122, 128)}     # N at the low / high end of the group count: low = pairs past N in the last group
R2_PAIRS = tuple((kt, gt) for kt in RESIDENT2_KT for gt in RESIDENT2_GT if gt != 16 or kt <= RESIDENT2_GT16_MAX_KT)
STRIP_M = {48773: 2, 67139: 3, 98449: 4}                             # M → the most strip-loop iterations of a wavefront (grid 256)


def _dense_cases():
    out = []

    def add(name, mode, M, N, K, kernel, misaligned=False, **kw):
        targs = {k: kw.pop(k) for k in ("KT", "GT") if k in kw}
        out.append(DenseCase(name, mode, M, N, K, kernel, targs, misaligned, kw))

    def both(name, M, N, K, kernel, **kw):
        """A forward case (M, N, K) and the grad case whose dxx takes the same rule with w transposed: (M, K, N)."""
        add(name + "_fwd", "forward", M, N, K, kernel, **kw)
        add(name + "_dxx", "grad", M, K, N, kernel, **kw)

    # ---- all 14 (KT, GT) pairs of resident2, forward and with w transposed
    # (every GT meets both ends of its N range, every KT both ends of its K range, and the four combinations of ends all occur)
    for kt, gt in R2_PAIRS:
        a, b = RESIDENT2_KT.index(kt), RESIDENT2_GT.index(gt)
        both(f"r2_kt{kt}_gt{gt}", (4096, 4111)[(a + b) % 2], R2_N[gt][a % 2], R2_K[kt][b % 2], "resident2", KT=kt, GT=gt)
    # ---- resident, KT 1 … 8: odd N, a (KT, G) pair outside the resident2 set, a misaligned left operand
    for name, M, N, K, kt in (("odd_n", 4111, 1, 1, 1), ("tiny_even_n", 4096, 2, 16, 1), ("g3", 4096, 24, 17, 2), ("odd_n", 4111, 31, 33, 3),
                              ("g8", 4096, 64, 64, 4), ("odd_n", 4111, 33, 65, 5), ("even_n", 4096, 26, 80, 5), ("odd_n", 4111, 51, 81, 6),
                              ("odd_n", 4111, 99, 97, 7), ("odd_n", 4111, 95, 113, 8)):
        both(f"res_kt{kt}_{name}", M, N, K, "resident", KT=kt)
    both("align_4111_26_17_aligned", 4111, 26, 17, "resident2", KT=2, GT=4)
    both("align_4111_26_17_misaligned", 4111, 26, 17, "resident", misaligned=True, KT=2)
    # ---- the selectors
    both("sel_m4095", 4095, 100, 100, "panel")
    both("sel_m4096", 4096, 100, 100, "resident2", KT=7, GT=13)
    both("sel_lds_96_128", 4096, 96, 128, "resident", KT=8, lds=RESIDENT_LDS)
    both("sel_lds_97_128", 4096, 97, 128, "panel")
    both("sel_lds_108_112", 4096, 108, 112, "resident", KT=7)
    both("sel_lds_109_112", 4096, 109, 112, "panel")
    both("sel_lds_128_96", 4096, 128, 96, "resident", KT=6, lds=RESIDENT_LDS)
    both("sel_lds_128_97", 4096, 128, 97, "panel")
    both("sel_128_128", 4096, 128, 128, "panel")
    both("sel_122_113", 4096, 122, 113, "panel")
    both("sel_n128_k20", 4096, 128, 20, "resident2", KT=2, GT=16)
    both("sel_n129_k20", 4096, 129, 20, "panel")
    both("sel_n20_k128", 4096, 20, 128, "resident", KT=8)
    both("sel_n20_k129", 4096, 20, 129, "panel")
    both("sel_n0_m4096", 4096, 0, 20, "panel", zero_result=True)
    # ---- panel edges
    for K in (129, 144, 145, 257):                                   # K − c0 of 1, 16, 17 in the second pass, 1 in the third
        both(f"panel_k{K}", 65, 7, K, "panel", last_pass_cols=K - (K - 1) // PANEL_COLS * PANEL_COLS)
    for N in (1, 3, 4, 5, 64, 65, 130):                              # k-steps of 4; panels of 64 rows of w
        both(f"panel_n{N}", 33, N, 20, "panel")
    for M in (1, 63, 64, 65):
        both(f"panel_m{M}", M, 9, 18, "panel")
    both("panel_n0", 70, 0, 20, "panel", zero_result=True)           # an all-zero result over a NaN-filled buffer, forward and dxx (grad case K = 0)
    add("nothing_m0_fwd", "forward", 0, 5, 7, None, untouched=True)
    add("nothing_k0_fwd", "forward", 5, 7, 0, None, untouched=True)
    # ---- the persistent strip loop: 2, 3, 4 iterations for some wavefronts
    for M, it in STRIP_M.items():
        both(f"strips{it}_r2", M, 26, 17, "resident2", KT=2, GT=4, iterations=it, big=True)
        both(f"strips{it}_res", M, 27, 17, "resident", KT=2, iterations=it, big=True)
    # ---- dw
    for kt in range(1, 9):
        for K in (16 * kt - 15, 16 * kt):
            add(f"dw_kt{kt}_k{K}", "grad", 100, 20, K, "panel", dw_KT=kt)
    for K in (129, 257):
        add(f"dw_k{K}", "grad", 100, 20, K, "panel", dw_KT=8, dw_bz=_cdiv(K, 128))
    for N in (1, 16, 17, 64, 65, 128, 129, 144, 145, 192, 193, 256):
        add(f"dw_n{N}", "grad", 50, N, 20, "panel", dw_last_rows=N - (N - 1) // 128 * 128, dw_by=_cdiv(N, 128))
    add("dw_n130_k130", "grad", 40, 130, 130, "panel", dw_KT=8, dw_by=2, dw_bz=2)
    for M, rpw, ranges in ((1, 16, 1), (15, 16, 1), (16, 16, 1), (17, 16, 2), (33, 16, 3), (8191, 16, 512), (8192, 16, 512), (8193, 32, 257),
                           (16385, 48, 342), (40000, 80, 500)):
        add(f"dw_m{M}", "grad", M, 20, 20, "resident" if M >= PERSIST_MIN_M else "panel", dw_rows_per_wg=rpw, dw_ranges=ranges,
            **({"KT": 2} if M >= PERSIST_MIN_M else {}))
    return out


@functools.lru_cache(maxsize=None)
def dense_cases():
    return tuple(_dense_cases())


def dense_case(name):
    return {c.name: c for c in dense_cases()}[name]


# the pairs of cases that sit on the two sides of one selector: they differ by one in one dimension (or in the alignment alone)
DENSE_THRESHOLD_PAIRS = (("sel_m4095", "sel_m4096"), ("sel_lds_96_128", "sel_lds_97_128"), ("sel_lds_108_112", "sel_lds_109_112"),
                         ("sel_lds_128_96", "sel_lds_128_97"), ("sel_n128_k20", "sel_n129_k20"), ("sel_n20_k128", "sel_n20_k129"),
                         ("align_4111_26_17_aligned", "align_4111_26_17_misaligned"))


# ------------------------------------------------------------------------------------------------ element meshes
class Mesh(NamedTuple):
    ien: np.ndarray              # int32 [nel][npe]
    id: np.ndarray               # int32 [nno][dof]
    nno: int
    neq: int
    npe: int
    dof: int


def _natural_id(nno, dof):
    return (dof * np.arange(nno)[:, None] + np.arange(dof)[None, :]).astype(np.int32)


def fan_mesh(T, npe, dof=3, hub=0):
    """T elements of npe nodes round one hub node: the hub is local node e mod npe of element e, every other node belongs to one element."""
    nno = 1 + T * (npe - 1)
    others = iter(n for n in range(nno) if n != hub)
    ien = np.array([[hub if a == e % npe else next(others) for a in range(npe)] for e in range(T)], np.int32).reshape(T, npe)
    return Mesh(ien, _natural_id(nno, dof), nno, nno * dof, npe, dof)


def random_mesh(nel, npe, dof, nno, seed, used=None):
    """nel elements whose npe nodes are drawn without repetition from the first `used` (default: all) of nno nodes."""
    rng = np.random.default_rng(seed)
    ien = np.array([rng.choice(nno if used is None else used, npe, replace=False) for _ in range(nel)], np.int32).reshape(nel, npe)
    return Mesh(ien, _natural_id(nno, dof), nno, nno * dof, npe, dof)


def scatter_id(mesh, extra, seed):
    """The same mesh with its equations scattered into neq + extra: `extra` equations have no owner."""
    neq = mesh.nno * mesh.dof + extra
    idmap = np.random.default_rng(seed).permutation(neq)[:mesh.nno * mesh.dof].astype(np.int32).reshape(mesh.nno, mesh.dof)
    return mesh._replace(id=idmap, neq=neq)


def hex_grid_mesh(ex, ey, ez):
    from tests.helpers import hex_mesh
    ien, idmap, nno, neq = hex_mesh(ex, ey, ez)
    return Mesh(ien, idmap, nno, neq, 8, 3)


class ElemCase(NamedTuple):
    name: str
    make: object                 # () -> Mesh
    kernel: str                  # "fixed8" / "generic" / "refused"
    claims: dict


def _elem_cases():
    out = []
    add = lambda name, make, kernel, **claims: out.append(ElemCase(name, make, kernel, claims))
    for T in (1, 8, 9, 16, 17, 25):                                  # rounds of 8 terms: 1, 1, 2, 2, 3, 4; n = 12: the column loop takes c = q and, for q < 4, q + 8
        add(f"tet_fan_{T}", functools.partial(fan_mesh, T, 4, 3, min(T, 2)), "generic", max_terms=T, rounds=_cdiv(T, 8), n=12)
    add("hex_fan_8", functools.partial(fan_mesh, 8, 8), "fixed8", max_terms=8, n=24)
    add("hex_fan_9", functools.partial(fan_mesh, 9, 8), "generic", max_terms=9, rounds=2, n=24)
    for npe, dof, nel, nno in ((8, 1, 11, 13), (8, 2, 11, 13), (8, 4, 11, 13), (3, 3, 10, 7), (1, 1, 10, 7), (27, 3, 6, 30)):
        add(f"shape_{npe}_{dof}", functools.partial(random_mesh, nel, npe, dof, nno, 100 * npe + dof), "generic", n=npe * dof)
    add("unreferenced_nodes", functools.partial(random_mesh, 9, 4, 3, 21, 7, 14), "generic", unreferenced=7, n=12)
    for nno, npe in ((1, 1), (2, 2), (3, 3), (5, 4)):                # a 4-node workgroup filled unevenly
        add(f"nno_{nno}", functools.partial(random_mesh, 5, npe, 3, nno, 40 + nno), "generic", nno=nno, n=3 * npe)
    add("scattered_hex", lambda: scatter_id(hex_grid_mesh(3, 2, 2), 11, 5), "fixed8", unowned=11, n=24)
    add("scattered_tet", lambda: scatter_id(random_mesh(30, 4, 3, 17, 6), 9, 6), "generic", unowned=9, n=12)
    add("dof5_refused", functools.partial(random_mesh, 3, 2, 5, 4, 8), "refused", n=10)
    return out


@functools.lru_cache(maxsize=None)
def elem_cases():
    return tuple(_elem_cases())


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The mesh of an element case, built once per process (read-only)."""
    m = {c.name: c for c in elem_cases()}[name].make()
    m.ien.setflags(write=False)
    m.id.setflags(write=False)
    return m


def elem_case(name):
    return {c.name: c for c in elem_cases()}[name]


def elem_operands(name, kind):
    """Element matrices K[nel][n·n] (not symmetric) and u[neq]."""
    m = mesh(name)
    rng = _rng(name, kind)
    n = m.npe * m.dof
    return values(rng, (len(m.ien), n * n), kind), values(rng, m.neq, kind)


# ------------------------------------------------------------------------------------------------ quadratic-form cases
class QuadCase(NamedTuple):
    name: str
    m: int
    numbers: int
    with_b: bool


QUAD_M = (1, 2, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def quad_cases():
    return tuple(QuadCase(f"quad_m{m}_{tag}", m, numbers, with_b) for m in QUAD_M
                 for tag, numbers, with_b in (("num1", 1, False), ("num1_b", 1, True), ("num2", 2, False), ("num3", 3, False)))


def quad_operands(case, kind):
    """a[m·m·numbers], x[m], b[m] or None — signed."""
    rng = _rng(case.name, kind)
    a, x = values(rng, case.m * case.m * case.numbers, kind), values(rng, case.m, kind)
    return a, x, (values(rng, case.m, kind) if case.with_b else None)


# ------------------------------------------------------------------------------------------------ numpy.longdouble restatements
LD = np.longdouble


def ld_dense(xx, w):
    """result[e][a] = Σ_k xx[e][k]·w[k][a]."""
    return xx.astype(LD) @ w.astype(LD)


def dense_scale(xx, w):
    """Σ_k |xx[e][k]·w[k][a]| — the Σ|terms| of the tolerances (fp64 is enough for a scale)."""
    return np.abs(xx) @ np.abs(w)


def ld_dense_grad(xx, w, grad):
    """dxx[i][n] = Σ_k grad[i][k]·w[n][k];  dw[n][k] = Σ_i xx[i][n]·grad[i][k]."""
    x, ww, g = xx.astype(LD), w.astype(LD), grad.astype(LD)
    return g @ np.ascontiguousarray(ww.T), np.ascontiguousarray(x.T) @ g


def dense_grad_scales(xx, w, grad):
    return np.abs(grad) @ np.abs(w).T, np.abs(xx).T @ np.abs(grad)


def ld_element_matvec(m, K, u):
    """Au[id[ien[e][a]][i]] = Σ_e Σ_c K_e[(dof·a + i)·n + c]·u[eq_e[c]], eq_e[dof·b + d] = id[ien[e][b]][d]; equations without an owner stay 0."""
    n = m.npe * m.dof
    Au = np.zeros(m.neq, LD)
    for e in range(len(m.ien)):
        eq = m.id[m.ien[e]].ravel()
        np.add.at(Au, eq, K[e].reshape(n, n).astype(LD) @ u[eq].astype(LD))
    return Au


def elem_scale(m, K, u):
    return ld_element_matvec(m, np.abs(K), np.abs(u)).astype(np.float64)


def ld_sym_quadratic_form(m, numbers, a, x, b=None, magnitudes=False):
    """(result[0], result[1]) of g4s_sym_quadratic_form from zero (include/g4s.h): Σ_i Σ_{j<i} x_i x_j (a[num·(i+m·j)+s] + a[num·(j+m·i)+s]) +
    Σ_i x_i² a[num·(i+m·i)+s] for s = 0 and, where numbers > 1, s = 1; numbers == 1: result[1] = Σ_i x_i·b_i (0 without b).
    magnitudes=True: the sums of the absolute values of the terms, from the absolute values of the inputs (|x_i x_j|·(|a1| + |a2|))."""
    f = (lambda v: np.abs(v).astype(LD)) if magnitudes else (lambda v: v.astype(LD))
    a, x = f(np.asarray(a)), f(np.asarray(x))
    xx = np.outer(x, x)
    res = []
    for s in range(min(numbers, 2)):
        A = a[s::numbers].reshape(m, m)                              # A[j][i] = a[num·(i + m·j) + s]
        res.append(np.sum(np.tril(xx * (A + A.T), -1)) + np.sum(x * x * np.diagonal(A)))
    if numbers == 1:
        res.append(np.sum(x * f(np.asarray(b))) if b is not None else LD(0))
    return np.array(res, LD)


# ------------------------------------------------------------------------------------------------ the oracle on many rows
def oracle_dense(oracle, xx, w):
    """oracle.dense_rows_times_matrix with the row pointers built by numpy (one Python call, not one per row)."""
    M, N = xx.shape
    K = w.shape[1]
    xx = np.ascontiguousarray(xx)
    rows = (xx.ctypes.data + 8 * N * np.arange(max(M, 1), dtype=np.uint64)).astype(np.uint64)
    res = np.zeros((M, K))
    oracle.lib.oracle_dense_rows_times_matrix(M, N, K, rows.ctypes.data, np.ascontiguousarray(w), res)
    return res
